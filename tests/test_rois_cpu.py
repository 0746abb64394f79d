"""The region-of-interest export without a GPU: snap_rois, the
ValueError cases of Engine.to_tensor(rois=) and Decoder.rois through their
descriptor builders, and the library's symbols."""
import ctypes as C

import pytest

from broadway_amd import _lib
from broadway_amd.decoder import rois_args
from broadway_amd.engine import rois_desc, snap_rois


def test_snap_rois_rounds_outward_clips_and_drops():
    boxes = [
        (0, 10.2, 7.9, 50.1, 33.0),         # outward: 10..52, 6..34
        (1, 11, 9, 21, 19),                 # odd integers: 10..22, 8..20
        (2, 4, 6, 8, 10),                   # even already: unchanged
        (0, -5.5, -0.1, 3.2, 2.0),          # clipped at the origin: 0..4, 0..2
        (1, 90.5, 60.5, 200.0, 100.0),      # clipped at the far corner: 90..96, 60..64
        (0, 96.0, 10.0, 120.0, 20.0),       # starts at the right edge: empty
        (0, 10.0, 70.0, 20.0, 80.0),        # below the picture: empty
        (2, -9.0, 3.0, -1.0, 9.0),          # left of the picture: empty
        (1, 20.0, 20.0, 20.0, 30.0),        # no width, on an even column: empty
        (1, 21.0, 20.0, 21.0, 30.0),        # no width, on an odd column: outward rounding gives 20..22
        (0, 30.0, 30.0, 20.0, 40.0),        # x1 < x0: empty
    ]
    rois, kept = snap_rois(boxes, 96, 64)
    assert rois == [(0, 10, 6, 42, 28), (1, 10, 8, 12, 12), (2, 4, 6, 4, 4), (0, 0, 0, 4, 2), (1, 90, 60, 6, 4),
                    (1, 20, 20, 2, 10)]
    assert kept == [0, 1, 2, 3, 4, 9]
    assert all(isinstance(v, int) for b in rois for v in b)
    assert snap_rois([], 96, 64) == ([], [])
    # what it returns is what the export accepts
    rois_desc(rois, (8, 8), 3, 96, 64)


GOOD = [(0, 0, 0, 96, 64), (1, 10, 20, 86, 44), (2, 4, 6, 2, 2)]


def test_rois_desc_builds_the_descriptor_and_the_box_array():
    import torch
    d, arr, planes, dtype = rois_desc(GOOD, (7, 5), 3, 96, 64, mode="gray", dtype=torch.uint8)
    assert isinstance(d, _lib.TensorResizeDesc) and (d.oh, d.ow, d.filter) == (7, 5, 0)
    assert (d.t.x, d.t.y, d.t.cw, d.t.ch) == (0, 0, 0, 0)        # reserved
    assert planes == 1 and dtype == torch.uint8 and len(arr) == 3
    assert [(b.pic, b.x, b.y, b.cw, b.ch) for b in arr] == GOOD
    d, _, planes, dtype = rois_desc(GOOD, (7, 5), 3, 96, 64, colour="bt709-full")
    assert planes == 3 and dtype == torch.float16 and d.t.mode == 3 << 8


@pytest.mark.parametrize("rois,size,why", [
    (GOOD, None, "rois without size"),
    ([], (8, 8), "an empty list"),
    ([(3, 0, 0, 16, 16)], (8, 8), "k == npics"),
    ([(-1, 0, 0, 16, 16)], (8, 8), "k == -1"),
    ([(0, 1, 0, 16, 16)], (8, 8), "odd x"),
    ([(0, 0, 1, 16, 16)], (8, 8), "odd y"),
    ([(0, 0, 0, 15, 16)], (8, 8), "odd cw"),
    ([(0, 0, 0, 16, 15)], (8, 8), "odd ch"),
    ([(0, 12, 20, 86, 44)], (8, 8), "over the right edge"),
    ([(0, 10, 22, 86, 44)], (8, 8), "over the bottom edge"),
    ([(0, -2, 0, 16, 16)], (8, 8), "negative x"),
    ([(0, 0, 0, 0, 16)], (8, 8), "no width"),
    ([(0, 0, 0, 66, 32)], (8, 2), "beyond 32 : 1 on x"),
    ([(0, 0, 0, 32, 34)], (1, 8), "beyond 32 : 1 on y"),
    (GOOD + [(0, 3, 0, 16, 16)], (8, 8), "one bad box last among good ones"),
    ([(0, 0, 0, 16)], (8, 8), "four numbers"),
    ([(0, 0, 0, 16.5, 16)], (8, 8), "a fraction"),
    (GOOD, (0, 8), "size 0"),
    (GOOD, (8, 16385), "size beyond 16384"),
])
def test_rois_desc_rejects(rois, size, why):
    with pytest.raises(ValueError):
        rois_desc(rois, size, 3, 96, 64)


def test_rois_desc_accepts_the_edge_cases():
    rois_desc([(0, 0, 0, 64, 32)], (8, 2), 1, 96, 64)            # exactly 32 : 1
    rois_desc([(2, 10, 20, 86, 44)], (8, 8), 3, 96, 64)          # flush right and bottom, the last picture
    rois_desc([(0, 2, 2, 2, 2)], (48, 64), 1, 96, 64)            # upscaled
    rois_desc([(0, 2.0, 2.0, 4.0, 4.0)], (3, 3), 1, 96, 64)      # whole-number floats, as snap_rois' callers may hold


def test_rois_desc_colour_rules_are_the_tensor_options():
    with pytest.raises(ValueError):
        rois_desc(GOOD, (8, 8), 3, 96, 64, colour="stream")     # an engine knows no stream
    with pytest.raises(ValueError):
        rois_desc(GOOD, (8, 8), 3, 96, 64, mode="gray", colour="bt709")
    d, *_ = rois_desc(GOOD, (8, 8), 3, 96, 64, colour="stream", unspecified="size", stream_ok=True)
    assert d.t.mode == 15 << 8 | 2 << 12


def test_engine_to_tensor_refuses_before_the_library_is_called():
    """Engine.to_tensor(rois=) on an object that has no library handle: the
    ValueError comes first."""
    from broadway_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 6, 4
    eng._h = None                                               # (close() and __del__ find nothing to destroy)
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0, 0], [0, 1, 2], rois=GOOD)                              # no size
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0, 0], [0, 1, 2], rois=GOOD, size=(8, 8), window=(0, 0, 16, 16))
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0, 0], [0, 1, 2], rois=[], size=(8, 8))
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0], [0, 1], rois=GOOD, size=(8, 8))                       # k = 2 of two pictures
    with pytest.raises(ValueError):
        eng.to_tensor([0], [0], rois=[(0, 0, 0, 98, 64)], size=(8, 8))              # wider than the picture


def test_decoder_rois_argument_validation():
    """Decoder.rois' arguments (decoder.rois_args): boxes are (x, y, cw, ch) of
    picture 0 in the delivered window."""
    import torch
    d, arr, planes, dtype = rois_args([(0, 0, 86, 52), (84, 50, 2, 2)], (5, 7), 86, 52, dtype=torch.float32)
    assert [(b.pic, b.x, b.y, b.cw, b.ch) for b in arr] == [(0, 0, 0, 86, 52), (0, 84, 50, 2, 2)]
    assert (d.oh, d.ow, planes, dtype) == (5, 7, 3, torch.float32)
    assert (d.t.x, d.t.y, d.t.cw, d.t.ch) == (0, 0, 0, 0)
    d, *_ = rois_args([(0, 0, 2, 2)], (4, 4), 86, 52, colour="stream", unspecified="bt709")
    assert d.t.mode == 15 << 8 | 1 << 12                         # the decoder knows the stream
    for boxes, size in (([], (4, 4)), ([(0, 0, 88, 52)], (4, 4)), ([(0, 0, 86, 54)], (4, 4)), ([(1, 0, 2, 2)], (4, 4)),
                        ([(0, 0, 2, 2, 2)], (4, 4)), ([(0, 0, 2, 2)], None), ([(0, 0, 2, 2)], (0, 4)), (7, (4, 4)),
                        ([(0, 0, 86, 52)], (1, 4))):
        with pytest.raises(ValueError):
            rois_args(boxes, size, 86, 52)
    with pytest.raises(ValueError):
        rois_args([(0, 0, 2, 2)], (4, 4), 86, 52, mode="yuv")
    # before the headers (no picture size yet) only the picture-independent rules are checked
    rois_args([(0, 0, 640, 480)], (224, 224), 0, 0)
    with pytest.raises(ValueError):
        rois_args([(1, 0, 640, 480)], (224, 224), 0, 0)


def test_library_exports_the_rois_entry_points():
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_rois_device_pitch", 12), ("h264mi_engine_export_tensor_rois", 10),
                        ("H264SwDecLastPictureTensorRois", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int pic, x, y, cw, ch; } h264mi_roi;
    assert C.sizeof(_lib.Roi) == 20
    assert [f[0] for f in _lib.Roi._fields_] == ["pic", "x", "y", "cw", "ch"]
    assert _lib.ROIS_MAX_PER_LAUNCH == 32
