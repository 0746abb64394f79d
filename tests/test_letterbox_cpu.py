"""The Python side of the letterboxed tensor export without a
GPU: engine.letterbox_fit against the table tests/letterbox_fit_check.c prints
from the C function, engine.unletterbox, the descriptor, and the argument
validation of Engine.to_tensor(fit=), the Decoder's tensor option and
Decoder.rois(fit=)."""
import ctypes as C

import pytest

import _letterbox as LB
import test_letterbox_desc
from broadway_amd import _lib
from broadway_amd.decoder import Decoder, rois_args
from broadway_amd.engine import fit_desc, letterbox_fit, rois_desc, snap_rois, tensor_desc, unletterbox

NAMES = {v: k for k, v in _lib.TENSOR_FIT.items()}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return test_letterbox_desc.fit_table(test_letterbox_desc.run_check(tmp_path_factory.mktemp("letterbox_fit_table")))


def test_letterbox_fit_is_the_c_function(table):
    assert len(table) >= 20 and _lib.TENSOR_FIT == LB.FITS == {"stretch": 0, "letterbox": 1, "topleft": 2}
    for (cw, ch, ow, oh, how), want in table.items():
        got = letterbox_fit(cw, ch, (oh, ow), NAMES[how])
        assert got == want and all(type(v) is int for v in got), (cw, ch, ow, oh, how)
        assert LB.fit(cw, ch, (oh, ow), NAMES[how]) == want, (cw, ch, ow, oh, how)     # the GPU tests' oracle agrees
    assert letterbox_fit(1920, 1080, (640, 640)) == (640, 360, 0, 140)                  # "letterbox" is the default


@pytest.mark.parametrize("args", [(0, 2, (4, 4)), (2, -2, (4, 4)), (2.5, 2, (4, 4)), (16386, 2, (4, 4)), (2, 2, (0, 4)),
                                  (2, 2, None), (2, 2, (4, 4), "centre"), (2, 2, (4, 4), 1), ("a", 2, (4, 4))])
def test_letterbox_fit_rejects(args):
    with pytest.raises(ValueError):
        letterbox_fit(*args)


@pytest.mark.parametrize("how", ["letterbox", "topleft", "stretch"])
@pytest.mark.parametrize("window,size", [((0, 0, 1920, 1080), (640, 640)), ((100, 40, 64, 128), (224, 224)),
                                         ((6, 2, 38, 26), (40, 70)), ((2, 2, 2, 2), (7, 5))])
def test_unletterbox_round_trips_the_content_corners(window, size, how):
    """The canvas corners of the content map to the window's corners, its
    centre to the window's centre, and the result feeds snap_rois."""
    x, y, cw, ch = window
    rw, rh, px, py = letterbox_fit(cw, ch, size, how)
    back = unletterbox([(3, px, py, px + rw, py + rh), (0, px + rw / 2, py + rh / 2, px + rw, py + rh)], window, size, how)
    assert back[0] == (3, x, y, x + cw, y + ch)
    assert back[1] == (0, x + cw / 2, y + ch / 2, x + cw, y + ch)
    rois, kept = snap_rois(back, x + cw, y + ch)
    assert rois[0] == (3, x, y, cw, ch) and kept == [0, 1]
    # a box that reaches into the bars maps outside the window; snap_rois clips it to the picture
    out = unletterbox([(0, px - 1, py - 1, px + rw + 1, py + rh + 1)], window, size, how)[0]
    assert out[1] < x and out[2] < y and out[3] > x + cw and out[4] > y + ch


def test_fit_desc_builds_the_descriptor():
    import torch
    r, planes, dtype = tensor_desc((6, 2, 38, 26), size=(40, 70), dtype=torch.float32)
    d = fit_desc(r, planes, "topleft", (1, 2, 3))
    assert C.sizeof(d) == 68 and (d.fit, list(d.pad)) == (2, [1, 2, 3, 0])
    assert (d.r.oh, d.r.ow, d.r.t.cw, d.r.t.ch) == (40, 70, 38, 26)
    assert list(fit_desc(r, planes).pad) == [114, 114, 114, 0] and fit_desc(r, planes).fit == 1
    g, planes, _ = tensor_desc((6, 2, 38, 26), size=(40, 70), mode="gray")
    assert list(fit_desc(g, planes, "stretch", 9).pad) == [9, 0, 0, 0] and fit_desc(g, planes, "stretch", (9,)).fit == 0
    for how, pad, n in (("centre", 114, 3), (1, 114, 3), ("letterbox", 256, 3), ("letterbox", -1, 3), ("letterbox", 1.5, 3),
                        ("letterbox", (1, 2), 3), ("letterbox", (1, 2, 3, 0), 3), ("letterbox", (1, 2, 3), 1),
                        ("letterbox", "grey", 3), ("letterbox", None, 3), ("letterbox", True, 3)):
        with pytest.raises(ValueError):
            fit_desc(r, n, how, pad)


def test_rois_desc_judges_each_box_against_its_own_fit():
    d, arr, planes, _ = rois_desc([(0, 0, 0, 96, 64), (1, 2, 2, 16, 48)], (2, 3), 2, 96, 64, fit="letterbox", pad=(1, 2, 3))
    assert isinstance(d, _lib.TensorFitDesc) and (d.fit, list(d.pad), d.r.oh, d.r.ow, len(arr)) == (1, [1, 2, 3, 0], 2, 3, 2)
    assert isinstance(rois_desc([(0, 0, 0, 96, 64)], (2, 3), 1, 96, 64)[0], _lib.TensorResizeDesc)       # no fit: as before
    assert rois_desc([(0, 0, 0, 96, 64)], (2, 3), 1, 96, 64, pad=7)[0].fit == 1                            # pad alone: letterbox
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 96, 64)], (8, 2), 1, 96, 64, fit="letterbox")         # 96 columns into 2
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 96, 64)], (1, 8), 1, 96, 64, fit="letterbox")         # height-bound: 64 rows into 1
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 96, 64)], (8, 8), 1, 96, 64, fit="box")
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 96, 64)], (8, 8), 1, 96, 64, fit="letterbox", pad=300)
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 96, 64)], (8, 8), 1, 96, 64, mode="gray", fit="letterbox", pad=(1, 2, 3))


def test_engine_to_tensor_refuses_before_the_library_is_called():
    """Engine.to_tensor(fit=) on an object that has no library handle: the
    ValueError comes first."""
    from broadway_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 6, 4
    eng._h = None                                               # (close() and __del__ find nothing to destroy)
    for kw in (dict(fit="letterbox"), dict(pad=0), dict(fit="stretch", window=(0, 0, 16, 16)),       # no size
               dict(size=(8, 8), fit="centre"), dict(size=(8, 8), fit=1), dict(size=(8, 8), fit="letterbox", pad=256),
               dict(size=(8, 8), fit="letterbox", pad=(1, 2)), dict(size=(8, 8), mode="gray", fit="topleft", pad=(1, 2, 3)),
               dict(size=(8, 8), pad=-1), dict(size=(8, 8), fit="letterbox", rois=[]),
               dict(size=(8, 8), fit="box", rois=[(0, 0, 0, 16, 16)]),
               dict(size=(8, 2), fit="letterbox", rois=[(0, 0, 0, 96, 64)]),
               dict(size=(8, 8), fit="letterbox", pad="x", rois=[(0, 0, 0, 16, 16)])):
        with pytest.raises(ValueError):
            eng.to_tensor([0], [0], **kw)


def test_decoder_option_and_rois_argument_validation():
    import torch
    for opts in ({"fit": "letterbox"}, {"pad": 3}, {"size": (8, 8), "fit": "centre"}, {"size": (8, 8), "pad": 256},
                 {"size": (8, 8), "fit": "letterbox", "pad": (1, 2)}, {"size": (8, 8), "mode": "gray", "pad": (1, 2, 3)},
                 {"size": (8, 8), "fit": "letterbox", "padding": 3}):
        with pytest.raises(ValueError):
            Decoder({"tensor": opts})
    d, arr, planes, dtype = rois_args([(0, 0, 86, 52), (84, 50, 2, 2)], (5, 7), 86, 52, dtype=torch.float32, fit="topleft",
                                      pad=(9, 8, 7))
    assert (d.fit, list(d.pad), d.r.oh, d.r.ow, planes, dtype, len(arr)) == (2, [9, 8, 7, 0], 5, 7, 3, torch.float32, 2)
    assert (d.r.t.x, d.r.t.y, d.r.t.cw, d.r.t.ch) == (0, 0, 0, 0)
    for kw in (dict(fit="centre"), dict(pad=256), dict(fit="letterbox", pad=(1, 2)), dict(fit=2)):
        with pytest.raises(ValueError):
            rois_args([(0, 0, 86, 52)], (5, 7), 86, 52, **kw)
    with pytest.raises(ValueError):
        rois_args([(0, 0, 86, 52)], (8, 2), 86, 52, fit="letterbox")               # 86 columns into 2


def test_library_exports_the_fit_entry_points():
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_letterbox_fit", 6), ("h264mi_tensor_fit_device_pitch", 10),
                        ("h264mi_tensor_rois_fit_device_pitch", 12), ("h264mi_engine_export_tensor_fit", 8),
                        ("h264mi_engine_export_tensor_rois_fit", 10), ("H264SwDecNextPictureTensorFit", 6),
                        ("H264SwDecLastPictureTensorRoisFit", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    out = (C.c_int * 4)()
    assert L.h264mi_letterbox_fit(1920, 1080, 640, 640, 1, out) == 0 and tuple(out) == (640, 360, 0, 140)
    for bad in ((0, 2, 4, 4, 1), (2, 2, 4, 0, 1), (2, 2, 4, 4, 3), (2, 2, 4, 4, -1), (16385, 2, 4, 4, 1), (2, 2, 16385, 4, 1)):
        assert L.h264mi_letterbox_fit(*bad, out) == -1, bad
    assert L.h264mi_letterbox_fit(2, 2, 4, 4, 1, None) == -1
    assert L.h264mi_engine_abi() == 6
