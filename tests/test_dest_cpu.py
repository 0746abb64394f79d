"""The Python surface of the strided destinations without a GPU:
engine.dest_of_view turns a view's strides into an h264mi_tensor_dest or names
the stride it cannot express, engine.empty_clip allocates NCTHW and
channels_last_3d clips, and the library declares the new entry points."""
import pytest

torch = pytest.importorskip("torch")

from broadway_amd import _lib                               # noqa: E402
from broadway_amd.engine import dest_of_view, empty_clip    # noqa: E402

CPU = torch.device("cpu")
F16 = torch.float16


def fields(view, shape, layout="nchw"):
    d, out_stride = dest_of_view(view, shape, view.dtype, CPU, layout)
    return (d.row, d.plane, d.frame, d.clip, d.reserved), out_stride


def test_views_become_descriptors_in_bytes():
    x = torch.zeros((3, 5, 8, 10), dtype=F16)
    assert fields(x[:, 1:4], (3, 3, 8, 10)) == ((20, 160, 0, 1, 0), 800)                    # a channel slice
    clip = torch.zeros((3, 4, 8, 10), dtype=F16)
    assert fields(clip[:, :3].permute(1, 0, 2, 3), (3, 3, 8, 10)) == ((20, 640, 0, 1, 0), 160)     # item below plane
    canvas = torch.zeros((3, 16, 40), dtype=F16)
    grid = canvas.unflatten(2, (4, 10)).unflatten(1, (2, 8)).permute(1, 0, 3, 2, 4)         # (2, 3, 4, 8, 10)
    assert fields(grid, (2, 3, 4, 8, 10)) == ((80, 1280, 20, 4, 0), 640)                    # frame below row
    y = torch.zeros((3, 8, 12, 3), dtype=F16)
    assert fields(y.permute(0, 3, 1, 2)[..., :10], (3, 3, 8, 10), "nhwc") == ((72, 0, 0, 1, 0), 576)
    col = torch.zeros((2, 8, 1, 7), dtype=F16)[..., :3].permute(0, 3, 1, 2)               # one column: its stride is free
    assert col.stride(3) == 7 and fields(col, (2, 3, 8, 1), "nhwc") == ((14, 0, 0, 1, 0), 112)
    one = torch.zeros((1, 1, 1, 10), dtype=torch.float32)
    assert fields(one, (1, 1, 1, 10)) == ((0, 0, 0, 1, 0), 0)                              # no stride to speak of


def test_clips_are_ncthw_or_channels_last_3d():
    a = empty_clip((2, 3, 3, 8, 10), F16, CPU)
    assert a.is_contiguous() and fields(a, (2, 3, 3, 8, 10)) == ((20, 480, 160, 3, 0), 1440)
    b = empty_clip((2, 3, 3, 8, 10), F16, CPU, "nhwc")
    like = torch.empty((2, 3, 3, 8, 10), dtype=F16).contiguous(memory_format=torch.channels_last_3d)
    assert tuple(b.shape) == (2, 3, 3, 8, 10) and b.stride() == like.stride()
    assert fields(b, (2, 3, 3, 8, 10), "nhwc") == ((60, 0, 480, 3, 0), 1440)


@pytest.mark.parametrize("what,make,layout", [
    ("column stride 2", lambda: torch.zeros((2, 3, 8, 20), dtype=F16)[..., ::2], "nchw"),
    ("item stride 0", lambda: torch.zeros((1, 3, 8, 10), dtype=F16).expand(2, 3, 8, 10), "nchw"),
    ("plane stride 0", lambda: torch.zeros((2, 1, 8, 10), dtype=F16).expand(2, 3, 8, 10), "nchw"),
    ("float32", lambda: torch.zeros((2, 3, 8, 10), dtype=torch.float32), "nchw"),
    ("plane stride 80", lambda: torch.zeros((2, 3, 8, 10), dtype=F16), "nhwc"),
    ("row stride 5", lambda: torch.zeros((2, 3, 8, 10), dtype=F16).as_strided((2, 3, 8, 10), (240, 80, 5, 1)), "nchw"),
])
def test_inexpressible_views_name_the_stride(what, make, layout):
    v = make()
    with pytest.raises(ValueError, match=what):
        dest_of_view(v, (2, 3, 8, 10), F16, CPU, layout)


def test_wrong_shape_is_refused():
    with pytest.raises(ValueError):
        dest_of_view(torch.zeros((2, 3, 8, 12), dtype=F16), (2, 3, 8, 10), F16, CPU)


def test_library_declares_the_entry_points():
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_dest_device_pitch", 13), ("h264mi_tensor_warps_dest_device_pitch", 13),
                        ("h264mi_engine_export_tensor_dest", 11), ("h264mi_engine_export_tensor_warps_dest", 11),
                        ("H264SwDecNextPictureTensorDest", 7)):
        assert len(getattr(L, name).argtypes) == nargs, name


def test_decoder_option_validation():
    from broadway_amd.decoder import Decoder
    for bad in ({"step": 2}, {"clip": 0}, {"clip": 3, "step": 0}, {"clip": 2.0}, {"clip": True}):
        with pytest.raises(ValueError):
            Decoder({"tensor": bad})
