"""Resized tensor export over a list of regions of interest (resize.hip
k_tensor_resize's ROIS rows): K boxes over N pictures, every box
resized to one (oh, ow), from one launch per 32 boxes --
h264mi_tensor_rois_device_pitch, h264mi_engine_export_tensor_rois
(Engine.to_tensor(rois=)) and H264SwDecLastPictureTensorRois (Decoder.rois).

Every comparison is exact equality of bytes: against tests/_resize.py's oracle
per box (tests/_colour.py's for a colour set), and against the single-window
export of the same window."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import _colour as K
import _crop
import _resize as R
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CASES = _crop.cases()
CAP = 32                    # boxes per kernel launch (H264MI_ROIS_MAX_PER_LAUNCH)
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}       # test_resize.py's layouts
ORDER = [2, 0, 2]           # the picture list of every kernel test
# (k, (x, y, cw, ch)): k indexes ORDER
BOXES = [(0, (6, 2, 38, 26)), (1, (2, 2, 2, 2)), (2, (44, 30, 4, 2)), (1, (0, 0, 46, 32))]
SIZES = [(7, 5), (9, 64)]
WIDE_BOXES = [(0, (0, 0, 256, 32)), (2, (130, 0, 126, 32))]     # 32 : 1 on x, 64 taps
WIDE_SIZE = (3, 8)
SENTINEL = 0xA5
FRONT = 64


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
    """name -> 3 random pictures in the (width, cpitch) layout (read-only);
    test_resize.py's."""
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def make_desc(size, mode, dtype, consts="unit", colour=0, filt=0, window=(0, 0, 0, 0)):
    from broadway_amd import _lib
    d = _lib.TensorResizeDesc()
    d.t.x, d.t.y, d.t.cw, d.t.ch = window
    d.t.mode = {"rgb": 0, "gray": 1}[mode] | colour << 8
    d.t.dtype = T.DTYPES.index(dtype) if dtype in T.DTYPES else dtype
    scale, bias = T.CONSTS[consts]
    d.t.scale[:] = scale
    d.t.bias[:] = bias
    d.oh, d.ow = size
    d.filter = filt
    return d


def make_rois(boxes):
    from broadway_amd import _lib
    return (_lib.Roi * max(len(boxes), 1))(*[_lib.Roi(k, *win) for k, win in boxes])


def run_rois(pics, order, w, h, cp, boxes, size, mode, dtype, consts="unit", colour=0, in_pad=0, out_pad=0, skew=0,
             filt=0, null=(), stride=None, window=(0, 0, 0, 0), nrois=None, host_out=False):
    """h264mi_tensor_rois_device_pitch over `boxes` on pictures `order` of
    `pics`; returns rc, the whole output buffer (FRONT + skew sentinel bytes,
    then boxes out_stride apart, then 64 sentinel bytes), the first box's
    offset, out_stride and a box's bytes (test_resize.py's run_resize)."""
    import torch
    L = _mi()
    es = T.ELEM.get(dtype, 2)
    oh, ow = size
    nbytes = T.MODES[mode] * oh * ow * es if 0 < oh <= 512 and 0 < ow <= 512 else 16
    in_stride = pics[0].size + in_pad
    out_stride = nbytes + out_pad if stride is None else stride
    host = np.zeros(in_stride * len(pics), dtype=np.uint8)
    for k, p in enumerate(pics):
        host[k * in_stride:k * in_stride + p.size] = p
    d_in = torch.from_numpy(host).to("cuda")
    offs = (C.c_size_t * len(order))(*[k * in_stride for k in order])
    first = FRONT + skew
    nb = max(len(boxes), 1)
    d_out = torch.full((first + max(out_stride, nbytes) * nb + 64,), SENTINEL, dtype=torch.uint8,
                       device="cpu" if host_out else "cuda")
    assert d_out.data_ptr() % 16 == 0
    desc = make_desc(size, mode, dtype, consts, colour, filt, window)
    rc = L.h264mi_tensor_rois_device_pitch(None if "in" in null else d_in.data_ptr(),
                                           None if "offs" in null else offs, len(order), w, h, cp,
                                           None if "desc" in null else C.byref(desc),
                                           None if "rois" in null else make_rois(boxes),
                                           len(boxes) if nrois is None else nrois,
                                           None if "out" in null else d_out.data_ptr() + first, out_stride,
                                           torch.cuda.current_stream().cuda_stream)
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


def box_expect(pic, w, h, cp, win, size, mode, dtype, consts, colour=0):
    """The oracle's bytes of one box: tests/_resize.py's, or for a colour set
    tests/_colour.py's (the same resize over that set's samples)."""
    if colour == 0:
        return R.expect(pic, w, h, cp, win, size, mode, dtype, consts)
    return K.expect(pic, w, h, cp, tuple(win), colour, dtype, consts, size=size)


def check_list(pics, out, first, stride, nbytes, w, h, cp, boxes, size, mode, dtype, consts, colour=0, order=ORDER):
    """Every box equals the oracle and no byte outside the K outputs changed."""
    assert (out[:first] == SENTINEL).all()
    for r, (k, win) in enumerate(boxes):
        o = first + r * stride
        want = box_expect(pics[order[k]], w, h, cp, win, size, mode, dtype, consts, colour)
        assert same(out[o:o + nbytes], want), (r, k, win, size)
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), (r, k, win, size)
    assert (out[first + len(boxes) * stride:] == SENTINEL).all()


def consts_of(dtype):
    return ["unit"] if dtype == "uint8" else ["unit", "imagenet"]        # uint8 ignores scale and bias


def lists_of(pic):
    """(boxes, size) lists of a layout: the mixed list at both sizes, and on
    the wide layout the 32 : 1 pair."""
    return [(BOXES, s) for s in SIZES] + ([(WIDE_BOXES, WIDE_SIZE)] if PICS[pic][0] == 256 else [])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_mixed_list_in_one_launch_vs_oracle(pictures, mode, dtype):
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        for boxes, size in lists_of(pic):
            for consts in consts_of(dtype):
                for colour in ((0, 3) if mode == "rgb" else (0,)):       # 3: bt709-full
                    rc, out, first, stride, nbytes = run_rois(pictures[pic], ORDER, w, h, cp, boxes, size, mode, dtype,
                                                              consts, colour)
                    assert rc == 0, (pic, size, consts, colour)
                    check_list(pictures[pic], out, first, stride, nbytes, w, h, cp, boxes, size, mode, dtype, consts,
                               colour)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_box_is_the_single_window_export(pictures, dtype):
    """Box r of the batch == h264mi_tensor_resize_device_pitch on the same
    picture, window and size; a list of one identity-size box ==
    h264mi_tensor_device_pitch."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        pics = pictures[pic]
        d_in = [torch.from_numpy(np.array(p)).to("cuda") for p in pics]
        zero = (C.c_size_t * 1)(0)
        for mode in sorted(T.MODES):
            for boxes, size in lists_of(pic):
                rc, out, first, stride, nbytes = run_rois(pics, ORDER, w, h, cp, boxes, size, mode, dtype, "imagenet")
                assert rc == 0
                for r, (k, win) in enumerate(boxes):
                    rd = make_desc(size, mode, dtype, "imagenet", window=win)
                    one = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                    assert L.h264mi_tensor_resize_device_pitch(d_in[ORDER[k]].data_ptr(), zero, 1, w, h, cp, C.byref(rd),
                                                               one.data_ptr(), nbytes, st) == 0
                    o = first + r * stride
                    assert same(out[o:o + nbytes], one.cpu().numpy()), (pic, mode, size, r)
            win = (6, 2, 38, 26)
            size = (win[3], win[2])
            td = _lib.TensorDesc.from_buffer_copy(make_desc(size, mode, dtype, "imagenet", window=win).t)
            nb = T.MODES[mode] * win[2] * win[3] * T.ELEM[dtype]
            plain = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            assert L.h264mi_tensor_device_pitch(d_in[0].data_ptr(), zero, 1, w, h, cp, C.byref(td), plain.data_ptr(), nb,
                                                st) == 0
            rc, out, first, _, nbytes = run_rois(pics, ORDER, w, h, cp, [(1, win)], size, mode, dtype, "imagenet")
            assert rc == 0 and nbytes == nb
            assert same(out[first:first + nb], plain.cpu().numpy()), (pic, mode)
            assert (out[:first] == SENTINEL).all() and (out[first + nb:] == SENTINEL).all(), (pic, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("gray", "uint8"), ("rgb", "float16")])
def test_list_longer_than_one_launch(pictures, mode, dtype):
    """33 boxes, all different: a 6 x 4 window slid by 2 over the three
    pictures; the 33rd is the second launch."""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    boxes = [(r % 3, (2 * (r % 21), 2 * (r // 21) + 2 * (r % 5), 6, 4)) for r in range(CAP + 1)]
    assert len(set(boxes)) == CAP + 1 and all(x + 6 <= w and y + 4 <= h for _, (x, y, _, _) in boxes)
    rc, out, first, stride, nbytes = run_rois(pics, ORDER, w, h, cp, boxes, (3, 3), mode, dtype, "imagenet", in_pad=37,
                                              out_pad=5 * T.ELEM[dtype])
    assert rc == 0
    check_list(pics, out, first, stride, nbytes, w, h, cp, boxes, (3, 3), mode, dtype, "imagenet")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_padded_strides_write_nothing_else(pictures, mode, dtype):
    """Input pictures 37 bytes apart; out_stride padded by 5 elements, by 48
    bytes, and by 48 bytes with d_out one element past a 16-byte boundary."""
    es = T.ELEM[dtype]
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_rois(pictures[pic], ORDER, w, h, cp, BOXES, (7, 5), mode, dtype,
                                                      "imagenet", in_pad=37, out_pad=out_pad, skew=skew)
            assert rc == 0, (pic, out_pad, skew)
            assert stride == nbytes + out_pad and first == FRONT + skew
            check_list(pictures[pic], out, first, stride, nbytes, w, h, cp, BOXES, (7, 5), mode, dtype, "imagenet")


# the refused rows of tests/test_rois_desc.py's grid, on three pictures of 96 x 64: (boxes, (oh, ow), keywords)
GOOD4 = [(0, (0, 0, 96, 64)), (1, (10, 20, 86, 44)), (2, (4, 6, 2, 2)), (0, (2, 2, 16, 16))]
REFUSED = {
    "pic_npics": ([(3, (0, 0, 16, 16))], (8, 8), {}),
    "pic_minus_1": ([(-1, (0, 0, 16, 16))], (8, 8), {}),
    "x_odd": ([(0, (1, 0, 16, 16))], (8, 8), {}),
    "y_odd": ([(0, (0, 1, 16, 16))], (8, 8), {}),
    "cw_odd": ([(0, (0, 0, 15, 16))], (8, 8), {}),
    "ch_odd": ([(0, (0, 0, 16, 15))], (8, 8), {}),
    "right_plus_1": ([(1, (10, 20, 87, 44))], (8, 8), {}),
    "right_plus_2": ([(1, (12, 20, 86, 44))], (8, 8), {}),
    "bottom_plus_1": ([(1, (10, 20, 86, 45))], (8, 8), {}),
    "bottom_plus_2": ([(1, (10, 22, 86, 44))], (8, 8), {}),
    "cw_0": ([(0, (0, 0, 0, 16))], (8, 8), {}),
    "ch_negative": ([(0, (0, 4, 16, -2))], (8, 8), {}),
    "cw_32x_plus_2": ([(0, (0, 0, 66, 32))], (8, 2), {}),
    "ch_32x_plus_2": ([(0, (0, 0, 32, 34))], (1, 8), {}),
    "nrois_0": (GOOD4, (8, 8), {"nrois": 0}),
    "nrois_negative": (GOOD4, (8, 8), {"nrois": -1}),
    "bad_box_last": (GOOD4[:3] + [(0, (3, 2, 16, 16))], (8, 8), {}),
    "reserved_window_set": (GOOD4, (8, 8), {"window": (0, 0, 96, 64)}),
    "reserved_x_set": (GOOD4, (8, 8), {"window": (2, 0, 0, 0)}),
    "reserved_y_set": (GOOD4, (8, 8), {"window": (0, 2, 0, 0)}),
    "ow_0": (GOOD4, (8, 0), {}),
    "filter_1": (GOOD4, (8, 8), {"filt": 1}),
    "dtype_i16": (GOOD4, (8, 8), {"dtype": 4}),
}


@pytest.mark.gpu
def test_refusals_launch_nothing():
    import test_rois_desc
    assert sorted(REFUSED) == sorted(k for k, v in test_rois_desc.ROIS.items() if v == test_rois_desc.R)
    w, h, cp = 96, 64, 48
    rng = np.random.default_rng(29)
    pics = [rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for _ in range(3)]
    order = [0, 1, 2]

    def run(boxes, size, **kw):
        args = dict(mode="rgb", dtype="float16")
        args.update(kw)
        return run_rois(pics, order, w, h, cp, boxes, size, args.pop("mode"), args.pop("dtype"), **args)

    rc, out, first, stride, nbytes = run(GOOD4, (8, 8))
    assert rc == 0                                       # the arguments below are one step away
    check_list(pics, out, first, stride, nbytes, w, h, cp, GOOD4, (8, 8), "rgb", "float16", "unit", order=order)
    rc, out, *_ = run([(0, (0, 0, 64, 32))], (8, 2))     # exactly 32 : 1 is accepted
    assert rc == 0
    for name, (boxes, size, kw) in sorted(REFUSED.items()):
        rc, out, *_ = run(boxes, size, **kw)
        assert rc == -1, name
        assert (out == SENTINEL).all(), name             # nothing was launched
    for null in ("in", "offs", "desc", "rois", "out"):
        rc, out, *_ = run(GOOD4, (8, 8), null=(null,))
        assert rc == -1 and (out == SENTINEL).all(), null
    rc, out, *_ = run(GOOD4, (8, 8), host_out=True)      # d_out on no device
    assert rc == -1 and (out == SENTINEL).all()
    rc, out, *_ = run(GOOD4, (8, 8), skew=1)             # d_out not a multiple of the element size
    assert rc == -1 and (out == SENTINEL).all()
    rc, out, *_ = run(GOOD4, (8, 8), stride=3 * 8 * 8 * 2 + 1)
    assert rc == -1 and (out == SENTINEL).all()
    rc, out, *_ = run(GOOD4, (8, 8), colour=15)          # STREAM: the engine-level calls know no stream
    assert rc == -1 and (out == SENTINEL).all()


def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def frame_expect(frame, w, h, win, size, mode, dtype, consts, colour=0):
    if mode == "rgb" and colour:
        return K.frame_expect(frame, w, h, win, colour, dtype, consts, size=size)
    x, y, cw, ch = win
    scale, bias = T.CONSTS[consts]
    c = T.samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode)
    return T.convert(R.resize_planes(c, size[0], size[1]), dtype, scale, bias)


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
def test_engine_to_tensor_rois_vs_reference_decoder():
    """Boxes over two slots with a caller stream and out=, against the
    reference decoder's pictures; a decode into one of the named slots queued
    right behind the export does not change the exported bytes."""
    import torch
    from broadway_amd.engine import Capture, Engine
    name = "crop_ltrb_6x4"          # the smallest case: 96 x 64
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16) == (96, 64)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    size = (7, 5)
    rois = [(1, 6, 2, 86, 52), (0, 0, 0, 96, 64), (1, 90, 60, 4, 2), (0, 2, 2, 2, 2), (0, 10, 20, 38, 26)]
    # the first later picture that is decoded into the slot of an earlier one
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    first = slots[:again].index(slots[again])
    other = next((k for k in range(again) if k != first), first)
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    held = [first, other]                               # (no slot was reused yet: they hold these pictures)
    out = torch.empty((len(rois), 3) + size, dtype=torch.float32, device="cuda")
    scale, bias = T.CONSTS["imagenet"]
    got = eng.to_tensor([0, 0], [slots[k] for k in held], rois=rois, size=size, dtype=torch.float32, scale=scale,
                        bias=bias, out=out, stream=side, colour="bt709-full")
    eng.decode([0], [cap.pictures[again]])              # overwrites slots[first]: it waits for the export
    gray = eng.to_tensor([0], [slots[again]], rois=[(0, 6, 2, 86, 52)], size=(13, 11), mode="gray", dtype=torch.uint8)
    torch.cuda.synchronize()
    assert got is out and eng.errors() == 0
    per = 3 * size[0] * size[1] * 4
    for r, (k, x, y, cw, ch) in enumerate(rois):
        want = frame_expect(frames[held[k]], w, h, (x, y, cw, ch), size, "rgb", "float32", "imagenet", colour=3)
        assert same(tensor_bytes(out[r]), want), r
    assert tensor_bytes(out).size == per * len(rois)
    assert tuple(gray.shape) == (1, 1, 13, 11)
    assert same(tensor_bytes(gray), frame_expect(frames[again], w, h, (6, 2, 86, 52), (13, 11), "gray", "uint8", "unit"))
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0], [0, 1], rois=rois, size=size, out=torch.empty((len(rois), 3, 5, 7), device="cuda",
                                                                          dtype=torch.float16))
    with pytest.raises(RuntimeError):
        eng.to_tensor([0, 0], [0, eng.nslots], rois=rois, size=size)        # the library refuses the slot


def run_decoder(stream, opts, on_picture):
    """Decoder(opts) over the stream's NAL units; on_picture(dec, k, buf, w, h)
    runs inside onPictureDecoded.  Returns the decoder, closed."""
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
@pytest.mark.parametrize("opts", [{"tensor": {"size": (13, 11)}}, {}], ids=["tensor", "plain"])
def test_decoder_rois_in_the_callback(opts):
    """Boxes in the delivered (crop) window's coordinates: one at its origin,
    one flush with its far corner; equal to the oracle at the crop-offset
    coordinates."""
    import torch
    name = "crop_ltrb_6x4"
    win = sps_window(CASES[name])
    assert win == (6, 2, 86, 52)
    frames, _, w, h, _ = O.decode(case_stream(name))
    boxes = [(0, 0, 20, 12), (82, 48, 4, 4), (0, 0, 86, 52)]
    size = (5, 9)
    got = []

    def on_picture(dec, k, buf, pw, ph):
        got.append(dec.rois(boxes, size, dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD))
        got.append(dec.rois(boxes[:2], size, mode="gray", dtype=torch.uint8))

    n = run_decoder(case_stream(name), dict(opts), on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) and len(got) == 2 * n
    for k in range(n):
        t, g = got[2 * k], got[2 * k + 1]
        assert tuple(t.shape) == (3, 3) + size and t.dtype == torch.float16 and t.is_cuda
        assert tuple(g.shape) == (2, 1) + size and g.dtype == torch.uint8
        for r, (x, y, cw, ch) in enumerate(boxes):
            at = (x + win[0], y + win[1], cw, ch)
            assert same(tensor_bytes(t[r]), frame_expect(frames[k], w, h, at, size, "rgb", "float16", "imagenet")), (k, r)
            if r < 2:
                assert same(tensor_bytes(g[r]), frame_expect(frames[k], w, h, at, size, "gray", "uint8", "unit")), (k, r)


@pytest.mark.gpu
def test_decoder_rois_colour_stream_is_the_whole_picture_tensors():
    """colour="stream" on a stream whose VUI names BT.709 full range: the set
    decoder.tensor_colour names for the whole-picture tensor, and its bytes."""
    import json
    import os
    import torch
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour.json")) as f:
        golden = json.load(f)
    c = golden["cases"]["m1_full"]
    s = gen.generate(golden["config"], c["seed"], **dict(golden["base_overrides"], **c["overrides"]))
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    frames, _, w, h, _ = O.decode(s)
    seen = []

    def on_picture(dec, k, buf, pw, ph):
        whole = dec.tensor_colour
        t = dec.rois([(0, 0, pw, ph), (2, 2, 8, 6)], (6, 7), dtype=torch.uint8, colour="stream")
        seen.append((whole, dec.tensor_colour, t, pw, ph))

    n = run_decoder(s, {"tensor": {"colour": "stream", "dtype": torch.uint8}}, on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) > 0
    x0, y0, cw0, ch0 = 6, 2, 86, 52                     # the streams of tests/golden/colour.json carry crop_ltrb_6x4's window
    assert {(pw, ph) for _, _, _, pw, ph in seen} == {(cw0, ch0)} and (w, h) == (96, 64)
    for k, (whole, mine, t, pw, ph) in enumerate(seen):
        assert whole == mine == "bt709-full", k
        for r, (x, y, cw, ch) in enumerate([(0, 0, pw, ph), (2, 2, 8, 6)]):
            want = frame_expect(frames[k], w, h, (x + x0, y + y0, cw, ch), (6, 7), "rgb", "uint8", "unit", colour=3)
            assert same(tensor_bytes(t[r]), want), (k, r)


@pytest.mark.gpu
def test_decoder_rois_return_codes():
    """H264SwDecLastPictureTensorRois: OK before any picture and after the
    next H264SwDecDecode, PARAM_ERR for a box over the crop edge and for pic =
    1, PIC_RDY on success; Decoder.rois raises RuntimeError where the call
    answers OK."""
    import torch
    from broadway_amd import _lib
    name = "crop_ltrb_6x4"          # two slices a picture: the NAL after a picture's last delivers nothing
    nals = split_annexb(case_stream(name))
    dec = Decoder()
    L = dec._L
    out = torch.full((2 * 3 * 4 * 4,), 7, dtype=torch.float16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    desc = make_desc((4, 4), "rgb", "float16")

    def call(boxes):
        return L.H264SwDecLastPictureTensorRois(dec._inst, C.byref(desc), make_rois(boxes), len(boxes), out.data_ptr(), st)

    good = [(0, (0, 0, 86, 52)), (0, (84, 50, 2, 2))]
    assert call(good) == _lib.H264SWDEC_OK                          # before the headers
    with pytest.raises(RuntimeError):
        dec.rois([(0, 0, 2, 2)], (4, 4))
    inside = []

    def cb(buf, w, h, infos):
        inside.append((call(good), call([(0, (0, 0, 88, 52))]), call([(0, (0, 2, 86, 52))]), call([(0, (84, 50, 4, 2))]),
                       call([(1, (0, 0, 2, 2))]), call(good[:1] + [(0, (1, 0, 2, 2))]), call([])))

    dec.onPictureDecoded = cb
    delivered_at = []
    for k, nal in enumerate(nals):
        before = len(inside)
        dec.decode(nal)
        if len(inside) > before:
            delivered_at.append(k)
            assert call(good) == _lib.H264SWDEC_PIC_RDY             # until the next decode
        elif delivered_at:
            assert call(good) == _lib.H264SWDEC_OK, k               # after the next H264SwDecDecode
            with pytest.raises(RuntimeError):
                dec.rois([(0, 0, 2, 2)], (4, 4))
    torch.cuda.synchronize()
    assert len(delivered_at) >= 2 and len(delivered_at) < len(nals) - 2
    P = _lib.H264SWDEC_PARAM_ERR
    assert set(inside) == {(_lib.H264SWDEC_PIC_RDY, P, P, P, P, P, P)}
    dec.close()
