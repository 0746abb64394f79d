"""Letterboxed tensor export (resize.hip k_tensor_resize's FIT rows, DESIGN
3.5l): a window, or every box of a list, scaled with its aspect ratio kept
into a canvas (oh, ow), the rest of the canvas the element of a pad sample --
h264mi_tensor_fit_device_pitch, h264mi_tensor_rois_fit_device_pitch,
h264mi_engine_export_tensor_fit / _rois_fit (Engine.to_tensor(fit=)),
H264SwDecNextPictureTensorFit (the Decoder's tensor option) and
H264SwDecLastPictureTensorRoisFit (Decoder.rois(fit=)).

Every comparison is exact equality of bytes against tests/_letterbox.py's
oracle: tests/_resize.py's resize (tests/_colour.py's for a colour set) at the
content size, placed by the fit restated there, in a canvas of
tests/_tensor.py's conversion of the pad sample.  The pictures are
tests/test_rois.py's layouts: 48 x 32 with chroma pitch 128, and 256 x 32."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import _crop
import _letterbox as LB
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CASES = _crop.cases()
CAP = 32                    # rows per kernel launch (H264MI_ROIS_MAX_PER_LAUNCH)
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}
ORDER = [2, 0, 2]           # the picture list of every kernel test
BOXES = [(0, (6, 2, 38, 26)), (1, (2, 2, 2, 2)), (2, (44, 30, 4, 2)), (1, (0, 0, 46, 32))]    # tests/test_rois.py's
PAD = (114, 7, 250)         # a different sample per plane
SENTINEL = 0xA5
FRONT = 64

# (layout, window, canvas (oh, ow), fit) -> the (rw, rh, px, py) the issue's geometry names; the tile is 32 x 16
GEOMETRIES = [
    # content edges inside tiles 0 and 1, tile 2 (columns 64..69) all bar, three tile rows
    ("48x32_pitch128", (6, 2, 38, 26), (40, 70), "letterbox", (58, 40, 6, 0)),
    # content narrower than a tile, bars on both sides, the tile boundary crossed off the 32-grid, up-scaling
    ("48x32_pitch128", (2, 2, 2, 2), (40, 70), "letterbox", (40, 40, 15, 0)),
    # one-row content, 64 taps on both axes
    ("256x32_packed", (0, 0, 256, 32), (3, 8), "letterbox", (8, 1, 0, 1)),
    # the 2-column last group
    ("256x32_packed", (130, 0, 126, 32), (3, 8), "letterbox", (8, 2, 0, 0)),
    # a tall box in a wide canvas, and a wide box in a tall one, at the top left: bars right, or bottom, only
    ("48x32_pitch128", (6, 2, 10, 26), (20, 70), "topleft", (8, 20, 0, 0)),
    ("48x32_pitch128", (0, 4, 46, 10), (37, 35), "topleft", (35, 8, 0, 0)),
    # bars above and below the content inside one tile: 6 x 3 in the middle of 6 x 9
    ("48x32_pitch128", (4, 4, 12, 6), (9, 6), "letterbox", (6, 3, 0, 3)),
]


def case_stream(name):
    c = CASES[name]
    s = gen.generate(c["config"], c["seed"], **c["overrides"])
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_tensor.py: the decoder instances here pool engines."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


def _mi():
    from broadway_amd import _lib
    return _lib.mi()


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 random pictures in the (width, cpitch) layout (read-only)."""
    rng = np.random.default_rng(31)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def make_desc(size, mode, dtype, consts="unit", colour=0, filt=0, window=(0, 0, 0, 0), how="letterbox", pad=PAD, pad3=0):
    from broadway_amd import _lib
    d = _lib.TensorFitDesc()
    t = d.r.t
    t.x, t.y, t.cw, t.ch = window
    t.mode = {"rgb": 0, "gray": 1}[mode] | colour << 8
    t.dtype = T.DTYPES.index(dtype) if dtype in T.DTYPES else dtype
    scale, bias = T.CONSTS[consts]
    t.scale[:] = scale
    t.bias[:] = bias
    d.r.oh, d.r.ow = size
    d.r.filter = filt
    d.fit = LB.FITS[how] if how in LB.FITS else how
    d.pad[:] = tuple(pad[:T.MODES[mode]]) + (0,) * (3 - T.MODES[mode]) + (pad3,)
    return d


def make_rois(boxes):
    from broadway_amd import _lib
    return (_lib.Roi * max(len(boxes), 1))(*[_lib.Roi(k, *win) for k, win in boxes])


def run_fit(pics, order, w, h, cp, size, mode, dtype, consts="unit", colour=0, window=None, boxes=None, how="letterbox",
            pad=PAD, in_pad=0, out_pad=0, skew=0, pad3=0, host_out=False):
    """h264mi_tensor_fit_device_pitch (window) or
    h264mi_tensor_rois_fit_device_pitch (boxes) on pictures `order` of `pics`;
    returns rc, the whole output buffer (FRONT + skew sentinel bytes, then
    canvases out_stride apart, then 64 sentinel bytes), the first canvas's
    offset, out_stride and a canvas's bytes."""
    import torch
    L = _mi()
    es = T.ELEM[dtype]
    oh, ow = size
    nbytes = T.MODES[mode] * oh * ow * es
    in_stride = pics[0].size + in_pad
    out_stride = nbytes + out_pad
    host = np.zeros(in_stride * len(pics), dtype=np.uint8)
    for k, p in enumerate(pics):
        host[k * in_stride:k * in_stride + p.size] = p
    d_in = torch.from_numpy(host).to("cuda")
    offs = (C.c_size_t * len(order))(*[k * in_stride for k in order])
    first = FRONT + skew
    n = len(order) if boxes is None else len(boxes)
    d_out = torch.full((first + out_stride * n + 64,), SENTINEL, dtype=torch.uint8, device="cpu" if host_out else "cuda")
    assert d_out.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    if boxes is None:
        desc = make_desc(size, mode, dtype, consts, colour, window=window, how=how, pad=pad, pad3=pad3)
        rc = L.h264mi_tensor_fit_device_pitch(d_in.data_ptr(), offs, len(order), w, h, cp, C.byref(desc),
                                              d_out.data_ptr() + first, out_stride, st)
    else:
        desc = make_desc(size, mode, dtype, consts, colour, how=how, pad=pad, pad3=pad3)
        rc = L.h264mi_tensor_rois_fit_device_pitch(d_in.data_ptr(), offs, len(order), w, h, cp, C.byref(desc),
                                                   make_rois(boxes), len(boxes), d_out.data_ptr() + first, out_stride, st)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


def same(got, want):
    """Exact equality; what differs is printed before the assertion fails."""
    if got.shape == want.shape and np.array_equal(got, want):
        return True
    if got.shape != want.shape:
        print(f"shapes differ: {got.shape} {want.shape}")
    else:
        bad = np.flatnonzero(got != want)
        print(f"{bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()} "
              f"want {want[bad[:8]].tolist()}")
    return False


def check_canvases(pics, out, first, stride, nbytes, w, h, cp, rows, size, mode, dtype, consts, how, pad=PAD, colour=0):
    """Canvas r of `rows` = [(picture, window), ...] equals the oracle -- so
    every element of it was written --, and no byte outside the canvases changed."""
    assert (out[:first] == SENTINEL).all()
    for r, (k, win) in enumerate(rows):
        o = first + r * stride
        want = LB.expect(pics[k], w, h, cp, win, size, mode, dtype, consts, how, pad, colour)
        assert same(out[o:o + nbytes], want), (r, k, win, size, how)
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), (r, k, win, size)
    assert (out[first + len(rows) * stride:] == SENTINEL).all()


def consts_of(dtype):
    return ["unit"] if dtype == "uint8" else ["unit", "imagenet"]        # uint8 ignores scale and bias


def test_the_geometries_are_the_ones_named():
    """(CPU) the oracle's fit of each geometry, and the tiles they are meant to hit."""
    for _, win, size, how, place in GEOMETRIES:
        assert LB.fit(win[2], win[3], size, how) == place, (win, size, how)
    rw, rh, px, py = GEOMETRIES[0][4]
    assert 0 < px < 32 and px + rw == 64 < 70 and rh > 32           # left edge in tile 0, tile 2 all bar, 3 tile rows
    rw, rh, px, py = GEOMETRIES[1][4]
    assert 0 < px and px + rw > 32 and px + rw < 64                 # one tile holds a left bar, the next a right bar


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_geometries_vs_oracle(pictures, mode, dtype):
    """Single-window export over ORDER; non-unit scale and bias ("imagenet"),
    so that the pad element is not the pad byte; colour sets 0..3."""
    L = _mi()
    for pic, win, size, how, place in GEOMETRIES:
        w, h, cp = PICS[pic]
        got = (C.c_int * 4)()
        assert L.h264mi_letterbox_fit(win[2], win[3], size[1], size[0], LB.FITS[how], got) == 0 and tuple(got) == place
        for consts in consts_of(dtype):
            for colour in ((0, 1, 2, 3) if mode == "rgb" and consts == consts_of(dtype)[-1] else (0,)):
                rc, out, first, stride, nbytes = run_fit(pictures[pic], ORDER, w, h, cp, size, mode, dtype, consts, colour,
                                                         window=win, how=how)
                assert rc == 0, (pic, win, size, how, consts, colour)
                check_canvases(pictures[pic], out, first, stride, nbytes, w, h, cp, [(k, win) for k in ORDER], size, mode,
                               dtype, consts, how, colour=colour)


@pytest.mark.gpu
def test_topleft_bars_are_right_and_bottom_only(pictures):
    """The first rh rows and rw columns are content (the resized export's
    bytes), everything right of and below them is one pad element per plane."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    for pic, win, size, how, (rw, rh, px, py) in GEOMETRIES:
        if how != "topleft":
            continue
        w, h, cp = PICS[pic]
        rc, out, first, stride, nbytes = run_fit(pictures[pic], [1], w, h, cp, size, "rgb", "float32", "imagenet",
                                                 window=win, how=how)
        assert rc == 0 and (px, py) == (0, 0) and (rw < size[1]) != (rh < size[0])
        canvas = out[first:first + nbytes].view(np.float32).reshape(3, size[0], size[1])
        rd = _lib.TensorResizeDesc.from_buffer_copy(make_desc((rh, rw), "rgb", "float32", "imagenet", window=win).r)
        d_in = torch.from_numpy(np.array(pictures[pic][1])).to("cuda")
        inner = torch.zeros((3, rh, rw), dtype=torch.float32, device="cuda")
        assert L.h264mi_tensor_resize_device_pitch(d_in.data_ptr(), (C.c_size_t * 1)(0), 1, w, h, cp, C.byref(rd),
                                                   inner.data_ptr(), inner.numel() * 4, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(canvas[:, :rh, :rw].view(np.uint32), inner.cpu().numpy().view(np.uint32))
        scale, bias = T.CONSTS["imagenet"]
        for p in range(3):
            elem = np.float32(np.float64(PAD[p]) * np.float64(np.float32(scale[p])) + np.float64(np.float32(bias[p])))
            assert (canvas[p, rh:, :] == elem).all() and (canvas[p, :, rw:] == elem).all()
            assert elem != PAD[p]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_stretch_is_the_resized_export(pictures, dtype):
    """fit = STRETCH == h264mi_tensor_resize_device_pitch's bytes; at the
    identity size == h264mi_tensor_device_pitch's."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    pic = "48x32_pitch128"
    w, h, cp = PICS[pic]
    pics = pictures[pic]
    d_in = torch.from_numpy(np.array(pics[1])).to("cuda")
    zero = (C.c_size_t * 1)(0)
    win = (6, 2, 38, 26)
    for mode in sorted(T.MODES):
        for size in ((40, 70), (7, 5), (win[3], win[2])):
            rc, out, first, _, nbytes = run_fit(pics, [1], w, h, cp, size, mode, dtype, "imagenet", window=win,
                                                how="stretch")
            assert rc == 0
            rd = _lib.TensorResizeDesc.from_buffer_copy(make_desc(size, mode, dtype, "imagenet", window=win).r)
            one = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            assert L.h264mi_tensor_resize_device_pitch(d_in.data_ptr(), zero, 1, w, h, cp, C.byref(rd), one.data_ptr(),
                                                       nbytes, st) == 0
            torch.cuda.synchronize()
            assert same(out[first:first + nbytes], one.cpu().numpy()), (mode, size)
            assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all()
        td = _lib.TensorDesc.from_buffer_copy(rd.t)
        plain = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        assert L.h264mi_tensor_device_pitch(d_in.data_ptr(), zero, 1, w, h, cp, C.byref(td), plain.data_ptr(), nbytes,
                                            st) == 0
        torch.cuda.synchronize()
        assert same(out[first:first + nbytes], plain.cpu().numpy()), mode


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_padded_strides_write_every_element_and_nothing_else(pictures, mode, dtype):
    """Input pictures 37 bytes apart; out_stride padded by 5 elements, by 48
    bytes, and by 48 bytes with d_out one element past a 16-byte boundary;
    single window and list."""
    es = T.ELEM[dtype]
    pic, win, size, how, _ = GEOMETRIES[0]
    w, h, cp = PICS[pic]
    for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
        rc, out, first, stride, nbytes = run_fit(pictures[pic], ORDER, w, h, cp, size, mode, dtype, "imagenet", window=win,
                                                 how=how, in_pad=37, out_pad=out_pad, skew=skew)
        assert rc == 0 and stride == nbytes + out_pad and first == FRONT + skew
        check_canvases(pictures[pic], out, first, stride, nbytes, w, h, cp, [(k, win) for k in ORDER], size, mode, dtype,
                       "imagenet", how)
        rc, out, first, stride, nbytes = run_fit(pictures[pic], ORDER, w, h, cp, (9, 12), mode, dtype, "imagenet",
                                                 boxes=BOXES, in_pad=37, out_pad=out_pad, skew=skew)
        assert rc == 0
        check_canvases(pictures[pic], out, first, stride, nbytes, w, h, cp, [(ORDER[k], b) for k, b in BOXES], (9, 12),
                       mode, dtype, "imagenet", "letterbox")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["letterbox", "topleft", "stretch"])
@pytest.mark.parametrize("mode,dtype", [("rgb", "float16"), ("gray", "uint8"), ("rgb", "bfloat16")])
def test_list_box_is_the_single_window_export(pictures, mode, dtype, how):
    """BOXES over ORDER into (40, 70) and (7, 5): each box has its own fit, and
    box r's bytes are the single-window fit export's of that window (and the
    oracle's)."""
    import torch
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    pic = "48x32_pitch128"
    w, h, cp = PICS[pic]
    pics = pictures[pic]
    d_in = [torch.from_numpy(np.array(p)).to("cuda") for p in pics]
    zero = (C.c_size_t * 1)(0)
    for size in ((40, 70), (7, 5)):
        rc, out, first, stride, nbytes = run_fit(pics, ORDER, w, h, cp, size, mode, dtype, "imagenet", colour=0, boxes=BOXES,
                                                 how=how)
        assert rc == 0
        check_canvases(pics, out, first, stride, nbytes, w, h, cp, [(ORDER[k], b) for k, b in BOXES], size, mode, dtype,
                       "imagenet", how)
        for r, (k, win) in enumerate(BOXES):
            fd = make_desc(size, mode, dtype, "imagenet", window=win, how=how)
            one = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            assert L.h264mi_tensor_fit_device_pitch(d_in[ORDER[k]].data_ptr(), zero, 1, w, h, cp, C.byref(fd),
                                                    one.data_ptr(), nbytes, st) == 0
            torch.cuda.synchronize()
            assert same(out[first + r * stride:first + r * stride + nbytes], one.cpu().numpy()), (size, r)
    assert len({LB.fit(b[2], b[3], (40, 70), "letterbox") for _, b in BOXES}) == 3              # three different fits


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("gray", "uint8"), ("rgb", "float16")])
def test_list_longer_than_one_launch(pictures, mode, dtype):
    """33 boxes, all different, of four widths: the 33rd is the second
    launch, with its own placement table."""
    pic = "48x32_pitch128"
    w, h, cp = PICS[pic]
    pics = pictures[pic]
    boxes = [(r % 3, (2 * (r % 18), 2 * (r // 18) + 2 * (r % 5), 6 + 2 * (r % 4), 4)) for r in range(CAP + 1)]
    assert len(set(boxes)) == CAP + 1 and all(x + cw <= w and y + 4 <= h for _, (x, y, cw, _) in boxes)
    rc, out, first, stride, nbytes = run_fit(pics, ORDER, w, h, cp, (5, 5), mode, dtype, "imagenet", boxes=boxes,
                                             in_pad=37, out_pad=5 * T.ELEM[dtype])
    assert rc == 0
    check_canvases(pics, out, first, stride, nbytes, w, h, cp, [(ORDER[k], b) for k, b in boxes], (5, 5), mode, dtype,
                   "imagenet", "letterbox")


@pytest.mark.gpu
def test_refusals_launch_nothing(pictures):
    """-1 and an output that is all sentinel: one bad box, pad[3] != 0, an
    unknown fit, a STREAM colour, a window that breaks 32 : 1 on its major
    axis, a list's reserved window set, a host d_out."""
    pic = "256x32_packed"
    w, h, cp = PICS[pic]
    pics = pictures[pic]
    good = [(0, (0, 0, 256, 32)), (1, (130, 0, 126, 32)), (2, (4, 6, 2, 2))]

    def run(**kw):
        args = dict(size=(3, 8), mode="rgb", dtype="float16")
        args.update(kw)
        return run_fit(pics, ORDER, w, h, cp, args.pop("size"), args.pop("mode"), args.pop("dtype"), **args)

    rc, out, first, stride, nbytes = run(boxes=good)
    assert rc == 0                                       # the arguments below are one step away
    check_canvases(pics, out, first, stride, nbytes, w, h, cp, [(ORDER[k], b) for k, b in good], (3, 8), "rgb", "float16",
                   "unit", "letterbox")
    assert run(window=(0, 0, 256, 32))[0] == 0
    refused = {
        "bad_box_last": dict(boxes=good[:2] + [(2, (3, 6, 2, 2))]),
        "bad_box_pic": dict(boxes=good[:2] + [(3, (4, 6, 2, 2))]),
        "box_33_to_1": dict(boxes=good, size=(3, 7)),               # 256 columns into 7
        "window_33_to_1": dict(window=(0, 0, 256, 32), size=(3, 7)),
        "pad3_list": dict(boxes=good, pad3=1),
        "pad3_window": dict(window=(0, 0, 256, 32), pad3=1),
        "fit_3_list": dict(boxes=good, how=3),
        "fit_minus_1_window": dict(window=(0, 0, 256, 32), how=-1),
        "stream_colour_list": dict(boxes=good, colour=15),
        "stream_colour_window": dict(window=(0, 0, 256, 32), colour=15),
        "window_odd": dict(window=(1, 0, 16, 16)),
        "window_empty": dict(window=(0, 0, 0, 0)),
        "host_out_list": dict(boxes=good, host_out=True),
        "host_out_window": dict(window=(0, 0, 256, 32), host_out=True),
        "skewed_out": dict(boxes=good, skew=1),
        "empty_list": dict(boxes=[]),
    }
    for name, kw in sorted(refused.items()):
        rc, out, *_ = run(**kw)
        assert rc == -1, name
        assert (out == SENTINEL).all(), name             # nothing was launched


def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
def test_engine_to_tensor_fit_is_the_stateless_call_on_the_slot():
    """Engine.to_tensor(fit=) with a caller stream and out=, with and without
    rois=: the stateless call's bytes on the frame slots, and the oracle's on
    the reference decoder's pictures; a decode into one of the named slots
    queued right behind the export does not change the exported bytes; a
    STREAM colour is refused at this level."""
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import Capture, Engine
    name = "crop_ltrb_6x4"          # the smallest case: 96 x 64
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16) == (96, 64)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    L = eng._L
    side = torch.cuda.Stream()
    size = (20, 50)
    win = sps_window(CASES[name])
    rois = [(1, 6, 2, 86, 52), (0, 0, 0, 96, 64), (1, 90, 60, 4, 2), (0, 2, 2, 2, 2), (0, 10, 20, 26, 38)]
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    first = slots[:again].index(slots[again])
    other = next((k for k in range(again) if k != first), first)
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    held = [first, other]                               # (no slot was reused yet: they hold these pictures)
    scale, bias = T.CONSTS["imagenet"]
    # the stateless calls on the slots, before anything overwrites them
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    base = min(eng.frame_ptr(0, slots[k]) for k in held)
    offs = (C.c_size_t * 2)(*[eng.frame_ptr(0, slots[k]) - base for k in held])
    fd = make_desc(size, "rgb", "float32", "imagenet", colour=3, window=win, how="letterbox", pad=(1, 2, 3))
    per = 3 * size[0] * size[1] * 4
    want_whole = torch.zeros(2 * per, dtype=torch.uint8, device="cuda")
    assert L.h264mi_tensor_fit_device_pitch(base, offs, 2, w, h, eng.chroma_pitch, C.byref(fd), want_whole.data_ptr(),
                                            per, st) == 0
    fl = make_desc(size, "rgb", "float32", "imagenet", colour=3, how="topleft", pad=(1, 2, 3))
    want_list = torch.zeros(len(rois) * per, dtype=torch.uint8, device="cuda")
    assert L.h264mi_tensor_rois_fit_device_pitch(base, offs, 2, w, h, eng.chroma_pitch, C.byref(fl),
                                                 make_rois([(r[0], r[1:]) for r in rois]), len(rois),
                                                 want_list.data_ptr(), per, st) == 0
    torch.cuda.synchronize()
    out = torch.empty((2, 3) + size, dtype=torch.float32, device="cuda")
    kw = dict(size=size, dtype=torch.float32, scale=scale, bias=bias, colour="bt709-full", pad=(1, 2, 3))
    got = eng.to_tensor([0, 0], [slots[k] for k in held], window=win, out=out, stream=side, fit="letterbox", **kw)
    boxes = eng.to_tensor([0, 0], [slots[k] for k in held], rois=rois, stream=side, fit="topleft", **kw)
    eng.decode([0], [cap.pictures[again]])              # overwrites slots[first]: it waits for the exports
    gray = eng.to_tensor([0], [slots[again]], window=win, size=(13, 11), mode="gray", dtype=torch.uint8, fit="letterbox")
    torch.cuda.synchronize()
    assert got is out and eng.errors() == 0
    assert same(tensor_bytes(out), want_whole.cpu().numpy())
    assert tuple(boxes.shape) == (len(rois), 3) + size and same(tensor_bytes(boxes), want_list.cpu().numpy())
    for r, k in enumerate(held):
        assert same(tensor_bytes(out[r]), LB.frame_expect(frames[k], w, h, win, size, "rgb", "float32", "imagenet",
                                                          "letterbox", (1, 2, 3), colour=3)), r
    for r, (k, x, y, cw, ch) in enumerate(rois):
        assert same(tensor_bytes(boxes[r]), LB.frame_expect(frames[held[k]], w, h, (x, y, cw, ch), size, "rgb", "float32",
                                                            "imagenet", "topleft", (1, 2, 3), colour=3)), r
    assert tuple(gray.shape) == (1, 1, 13, 11)
    assert same(tensor_bytes(gray), LB.frame_expect(frames[again], w, h, win, (13, 11), "gray", "uint8", "unit",
                                                    "letterbox", (114,)))
    # STREAM at engine level: -1, nothing written
    sentinel = torch.full((per,), SENTINEL, dtype=torch.uint8, device="cuda")
    one_stream, one_slot = (C.c_int * 1)(0), (C.c_int * 1)(slots[again])
    for desc, extra in ((make_desc(size, "rgb", "float32", colour=15, window=win), ()),
                        (make_desc(size, "rgb", "float32", colour=15), (make_rois([(0, win)]), 1))):
        call = L.h264mi_engine_export_tensor_rois_fit if extra else L.h264mi_engine_export_tensor_fit
        assert call(eng._h, 1, one_stream, one_slot, C.byref(desc), *extra, sentinel.data_ptr(), per, st) == -1
    torch.cuda.synchronize()
    assert (sentinel == SENTINEL).all()
    with pytest.raises(RuntimeError):
        eng.to_tensor([0], [eng.nslots], size=size, fit="letterbox")       # the library refuses the slot
    assert _lib.TENSOR_FIT == LB.FITS


def run_decoder(stream, opts, on_picture):
    """Decoder(opts) over the stream's NAL units; on_picture(dec, k, buf, w, h)
    runs inside onPictureDecoded.  Returns the number of pictures."""
    dec = Decoder(opts)
    count = [0]

    def cb(buf, w, h, infos):
        on_picture(dec, count[0], buf, w, h)
        count[0] += 1

    dec.onPictureDecoded = cb
    for nal in split_annexb(stream):
        dec.decode(nal)
    dec.close()
    return count[0]


@pytest.mark.gpu
def test_decoder_option_and_rois_over_the_crop_window():
    """Decoder({"tensor": {"size", "fit", "pad"}}): the SPS crop window
    letterboxed, and Decoder.rois(fit=) with boxes in that window's
    coordinates, against the oracle at the crop-offset coordinates."""
    import torch
    name = "crop_ltrb_6x4"
    win = sps_window(CASES[name])
    assert win == (6, 2, 86, 52)
    frames, _, w, h, _ = O.decode(case_stream(name))
    boxes = [(0, 0, 20, 12), (82, 48, 4, 4), (0, 0, 86, 52), (10, 4, 8, 40)]
    size = (24, 24)
    got = []

    def on_picture(dec, k, buf, pw, ph):
        assert (pw, ph) == (30, 40) and tuple(buf.shape) == (3, 40, 30)
        got.append((buf, dec.rois(boxes, size, dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD,
                                  fit="letterbox", pad=PAD),
                    dec.rois(boxes[:2], size, mode="gray", dtype=torch.uint8, fit="topleft")))

    opts = {"tensor": {"size": (40, 30), "fit": "letterbox", "pad": PAD, "dtype": torch.float32,
                       "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD}}
    n = run_decoder(case_stream(name), opts, on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) and len(got) == n
    assert LB.fit(86, 52, (40, 30), "letterbox") == (30, 18, 0, 11)
    for k, (whole, t, g) in enumerate(got):
        assert same(tensor_bytes(whole), LB.frame_expect(frames[k], w, h, win, (40, 30), "rgb", "float32", "imagenet",
                                                         "letterbox", PAD)), k
        assert tuple(t.shape) == (4, 3) + size and t.dtype == torch.float16 and t.is_cuda
        assert tuple(g.shape) == (2, 1) + size and g.dtype == torch.uint8
        for r, (x, y, cw, ch) in enumerate(boxes):
            at = (x + win[0], y + win[1], cw, ch)
            assert same(tensor_bytes(t[r]), LB.frame_expect(frames[k], w, h, at, size, "rgb", "float16", "imagenet",
                                                            "letterbox", PAD)), (k, r)
            if r < 2:
                assert same(tensor_bytes(g[r]), LB.frame_expect(frames[k], w, h, at, size, "gray", "uint8", "unit",
                                                                "topleft", (114,))), (k, r)


@pytest.mark.gpu
def test_decoder_colour_stream_resolves_from_the_window_not_the_canvas():
    """colour="stream" on a stream whose VUI names BT.709 full range, and by
    size (unspecified="size") on a stream that names nothing: a 1280-wide
    canvas does not make the 86 x 52 window BT.709."""
    import json
    import os
    import torch
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour.json")) as f:
        golden = json.load(f)
    c = golden["cases"]["m1_full"]
    s = gen.generate(golden["config"], c["seed"], **dict(golden["base_overrides"], **c["overrides"]))
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    frames, _, w, h, _ = O.decode(s)
    win = (6, 2, 86, 52)            # the streams of tests/golden/colour.json carry crop_ltrb_6x4's window
    seen = []

    def on_picture(dec, k, buf, pw, ph):
        whole = dec.tensor_colour
        t = dec.rois([(0, 0, 86, 52), (2, 2, 8, 6)], (9, 9), dtype=torch.uint8, colour="stream", fit="letterbox")
        seen.append((buf, whole, dec.tensor_colour, t))

    n = run_decoder(s, {"tensor": {"colour": "stream", "dtype": torch.uint8, "size": (9, 20), "fit": "topleft"}}, on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) > 0
    for k, (buf, whole, mine, t) in enumerate(seen):
        assert whole == mine == "bt709-full", k
        assert same(tensor_bytes(buf), LB.frame_expect(frames[k], w, h, win, (9, 20), "rgb", "uint8", "unit", "topleft",
                                                       (114,) * 3, colour=3)), k
        for r, (x, y, cw, ch) in enumerate([(0, 0, 86, 52), (2, 2, 8, 6)]):
            want = LB.frame_expect(frames[k], w, h, (x + 6, y + 2, cw, ch), (9, 9), "rgb", "uint8", "unit", "letterbox",
                                   (114,) * 3, colour=3)
            assert same(tensor_bytes(t[r]), want), (k, r)
    # no VUI: by size, from the 86 x 52 window (BT.601: the reference set), though the canvas is 1280 wide
    name = "crop_ltrb_6x4"
    frames, _, w, h, _ = O.decode(case_stream(name))
    seen = []
    n = run_decoder(case_stream(name), {"tensor": {"colour": "stream", "unspecified": "size", "dtype": torch.uint8,
                                                   "size": (2, 1280), "fit": "letterbox", "pad": 9}},
                    lambda dec, k, buf, pw, ph: seen.append((buf, dec.tensor_colour)))
    torch.cuda.synchronize()
    assert n == len(frames) == len(seen)
    for k, (buf, colour) in enumerate(seen):
        assert colour == "reference", k
        assert same(tensor_bytes(buf), LB.frame_expect(frames[k], w, h, win, (2, 1280), "rgb", "uint8", "unit",
                                                       "letterbox", (9,) * 3)), k


@pytest.mark.gpu
def test_decoder_calls_refuse_a_bad_descriptor_before_a_picture_is_taken():
    """H264SwDecNextPictureTensorFit: PARAM_ERR for pad[3] != 0, an unknown fit
    and a window beyond 32 : 1, each leaving the picture in the DPB for the
    good call that follows; H264SwDecLastPictureTensorRoisFit: PARAM_ERR for
    one bad box, PIC_RDY for the good list."""
    import torch
    from broadway_amd import _lib
    name = "crop_ltrb_6x4"
    nals = split_annexb(case_stream(name))
    frames, _, w, h, _ = O.decode(case_stream(name))
    dec = Decoder()                                      # (its own loop below takes the pictures)
    L = dec._L
    st = torch.cuda.current_stream().cuda_stream
    size = (8, 8)
    out = torch.full((3 * 8 * 8,), 7, dtype=torch.float16, device="cuda")
    lst = torch.full((2 * 3 * 8 * 8,), 7, dtype=torch.float16, device="cuda")
    pic = _lib.H264SwDecPicture()
    good = make_desc(size, "rgb", "float16")             # cw == 0: the crop window
    bad = [make_desc(size, "rgb", "float16", pad3=1), make_desc(size, "rgb", "float16", how=3),
           make_desc((8, 2), "rgb", "float16")]          # 86 columns into 2
    P, RDY = _lib.H264SWDEC_PARAM_ERR, _lib.H264SWDEC_PIC_RDY
    delivered = 0
    inp, o = _lib.H264SwDecInput(), _lib.H264SwDecOutput()
    for nal in nals:
        buf = (C.c_uint8 * len(nal)).from_buffer_copy(nal)
        inp.pStream, inp.dataLen = C.cast(buf, C.POINTER(C.c_uint8)), len(nal)
        while inp.dataLen > 0:
            ret = L.H264SwDecDecode(dec._inst, C.byref(inp), C.byref(o))
            used = C.cast(o.pStrmCurrPos, C.c_void_p).value - C.cast(inp.pStream, C.c_void_p).value
            if ret == _lib.H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY:
                inp.dataLen -= used
                inp.pStream = o.pStrmCurrPos
                continue
            inp.dataLen = 0
            if ret not in (_lib.H264SWDEC_PIC_RDY, _lib.H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY):
                continue
            for d in bad:
                assert L.H264SwDecNextPictureTensorFit(dec._inst, C.byref(pic), 0, C.byref(d), out.data_ptr(), st) == P
            torch.cuda.synchronize()
            assert (out == 7).all()
            while L.H264SwDecNextPictureTensorFit(dec._inst, C.byref(pic), 0, C.byref(good), out.data_ptr(), st) == RDY:
                torch.cuda.synchronize()
                assert same(tensor_bytes(out), LB.frame_expect(frames[delivered], w, h, (6, 2, 86, 52), size, "rgb",
                                                               "float16", "unit", "letterbox", PAD)), delivered
                delivered += 1
                ld = make_desc(size, "rgb", "float16")
                rois = [(0, (0, 0, 86, 52)), (0, (84, 50, 2, 2))]
                call = lambda boxes, d=ld: L.H264SwDecLastPictureTensorRoisFit(dec._inst, C.byref(d), make_rois(boxes),
                                                                             len(boxes), lst.data_ptr(), st)
                assert call(rois[:1] + [(0, (85, 50, 2, 2))]) == P and call(rois[:1] + [(1, (84, 50, 2, 2))]) == P
                assert call(rois, make_desc(size, "rgb", "float16", pad3=2)) == P
                assert call(rois, make_desc(size, "rgb", "float16", how=7)) == P
                torch.cuda.synchronize()
                assert (lst == 7).all()
                assert call(rois) == RDY
                torch.cuda.synchronize()
                assert same(tensor_bytes(lst[:lst.numel() // 2]),
                            LB.frame_expect(frames[delivered - 1], w, h, (6, 2, 86, 52), size, "rgb", "float16", "unit",
                                            "letterbox", PAD))
                lst.fill_(7)
                out.fill_(7)
    assert delivered >= 2
    dec.close()
