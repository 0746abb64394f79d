"""The layout option without a GPU: the layout strings, the
descriptor builders, ``out=`` in the wrong memory order, and the library's
symbols.  Every refusal is a ValueError before the library is called."""
import ctypes as C

import pytest

from broadway_amd import _lib
from broadway_amd.decoder import Decoder, rois_args
from broadway_amd.engine import (Engine, check_out, empty_layout, fit_desc, layout_desc, rois_desc, tensor_desc,
                                 tensor_layout)

BAD_LAYOUTS = ["NHWC", "hwc", "channels_last", "", None, 1, b"nhwc"]


def test_layout_names():
    assert tensor_layout("nchw") == 0 and tensor_layout("nhwc") == 1
    for bad in BAD_LAYOUTS:
        with pytest.raises(ValueError):
            tensor_layout(bad)


def test_builders_make_the_layout_descriptor():
    import torch
    t, planes, dtype = tensor_desc((2, 4, 6, 8), layout="nhwc", colour="bt709")
    assert isinstance(t, _lib.TensorLayoutDesc) and t.layout == 1 and (planes, dtype) == (3, torch.float16)
    assert (t.f.r.t.x, t.f.r.t.y, t.f.r.t.cw, t.f.r.t.ch, t.f.r.t.mode) == (2, 4, 6, 8, 2 << 8)
    assert (t.f.r.ow, t.f.r.oh, t.f.r.filter, t.f.fit, bytes(t.f.pad)) == (0, 0, 0, 0, b"\0\0\0\0")     # the unresized export
    r, *_ = tensor_desc((2, 4, 6, 8), size=(7, 9), layout="nchw")
    assert isinstance(r, _lib.TensorLayoutDesc) and (r.layout, r.f.r.ow, r.f.r.oh, r.f.fit) == (0, 9, 7, 0)
    plain, planes, _ = tensor_desc((2, 4, 6, 8), size=(7, 9))
    assert isinstance(plain, _lib.TensorResizeDesc)                 # without layout: what it always returned
    f = fit_desc(plain, planes, "topleft", (1, 2, 3), layout="nhwc")
    assert isinstance(f, _lib.TensorLayoutDesc) and (f.layout, f.f.fit, bytes(f.f.pad)) == (1, 2, b"\1\2\3\0")
    assert isinstance(fit_desc(plain, planes, "topleft", (1, 2, 3)), _lib.TensorFitDesc)
    d, arr, planes, _ = rois_desc([(0, 0, 0, 16, 16)], (8, 8), 1, 96, 64, fit="letterbox", layout="nhwc")
    assert isinstance(d, _lib.TensorLayoutDesc) and (d.layout, d.f.fit, d.f.r.oh, len(arr)) == (1, 1, 8, 1)
    d, *_ = rois_desc([(0, 0, 0, 16, 16)], (8, 8), 1, 96, 64, layout="nhwc")
    assert (d.layout, d.f.fit, d.f.r.ow, d.f.r.t.cw) == (1, 0, 8, 0)
    assert isinstance(rois_desc([(0, 0, 0, 16, 16)], (8, 8), 1, 96, 64)[0], _lib.TensorResizeDesc)
    d, *_ = rois_args([(0, 0, 2, 2)], (4, 4), 86, 52, layout="nhwc")
    assert isinstance(d, _lib.TensorLayoutDesc) and d.layout == 1
    with pytest.raises(ValueError):
        layout_desc(_lib.Roi(), "nhwc")
    for bad in BAD_LAYOUTS[:4] + BAD_LAYOUTS[5:]:                   # (None is "no layout descriptor" for the builders)
        with pytest.raises(ValueError):
            tensor_desc((0, 0, 4, 4), layout=bad)
        with pytest.raises(ValueError):
            fit_desc(plain, 3, layout=bad)
        with pytest.raises(ValueError):
            rois_desc([(0, 0, 0, 16, 16)], (8, 8), 1, 96, 64, layout=bad)


def test_empty_layout_is_the_usual_shape_with_channels_last_strides():
    import torch
    t = empty_layout((2, 3, 4, 6), torch.float16, torch.device("cpu"), "nhwc")
    assert tuple(t.shape) == (2, 3, 4, 6) and t.stride() == (72, 1, 18, 3)
    assert t.is_contiguous(memory_format=torch.channels_last) and t.permute(0, 2, 3, 1).is_contiguous()
    p = empty_layout((3, 4, 6), torch.uint8, torch.device("cpu"), "nhwc")
    assert tuple(p.shape) == (3, 4, 6) and p.stride() == (1, 18, 3)
    assert empty_layout((2, 3, 4, 6), torch.float16, torch.device("cpu"), "nchw").is_contiguous()


def test_out_in_the_other_layout_is_refused():
    import torch
    cpu, shape = torch.device("cpu"), (2, 3, 4, 6)
    nhwc = empty_layout(shape, torch.float16, cpu, "nhwc")
    nchw = torch.empty(shape, dtype=torch.float16)
    check_out(nhwc, shape, torch.float16, cpu, "nhwc")
    check_out(nchw, shape, torch.float16, cpu, "nchw")
    check_out(nchw.contiguous(memory_format=torch.channels_last), shape, torch.float16, cpu, "nhwc")
    for out, layout in ((nchw, "nhwc"), (nhwc, "nchw"), (nhwc[:, :, :, ::2], "nhwc"),
                        (torch.empty((2, 4, 6, 3), dtype=torch.float16), "nhwc"),
                        (nhwc.float(), "nhwc"), (nhwc, "hwc")):
        with pytest.raises(ValueError):
            check_out(out, shape, torch.float16, cpu, layout)


def test_engine_to_tensor_refuses_before_the_library_is_called():
    """Engine.to_tensor on an object that has no library handle: the ValueError
    comes first, in every form."""
    eng = Engine.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 6, 4
    eng._h = None                                               # (close() and __del__ find nothing to destroy)
    for bad in BAD_LAYOUTS:
        for kw in ({}, {"size": (8, 8)}, {"size": (8, 8), "fit": "letterbox"},
                   {"size": (8, 8), "rois": [(0, 0, 0, 16, 16)]}):
            with pytest.raises(ValueError):
                eng.to_tensor([0], [0], layout=bad, **kw)


def test_decoder_refuses_before_the_library_is_called():
    for bad in BAD_LAYOUTS:
        with pytest.raises(ValueError):
            Decoder({"tensor": {"layout": bad}})
    with pytest.raises(ValueError):
        Decoder({"tensor": {"layuot": "nhwc"}})
    dec = Decoder.__new__(Decoder)
    dec._info = _lib.H264SwDecInfo()
    for bad in BAD_LAYOUTS:
        with pytest.raises(ValueError):
            dec.rois([(0, 0, 2, 2)], (4, 4), layout=bad)


def test_library_exports_the_layout_entry_points():
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_layout_device_pitch", 12), ("h264mi_engine_export_tensor_layout", 10),
                        ("H264SwDecNextPictureTensorLayout", 6), ("H264SwDecLastPictureTensorRoisLayout", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert _lib.TENSOR_LAYOUTS == {"nchw": 0, "nhwc": 1}
