"""Affine-warped tensor export (warp.hip k_tensor_warp): K warps
over N pictures, each a 2x3 Q16 inverse map from an (oh, ow) output into one
window, bilinear in integers, from one launch per 32 warps --
h264mi_tensor_warps_device_pitch, h264mi_engine_export_tensor_warps
(Engine.to_tensor(warps=)) and H264SwDecLastPictureTensorWarps (Decoder.warps).

Every comparison is exact equality of bytes: against tests/_warp.py's oracle
(whose geometry tests/test_warp_geom.py ties to common/warp_geom.h), and for the
identity against the unresized export of the same window.  Every kernel test
puts sentinels before, between and after the outputs."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import _crop
import _tensor as T
import _warp as W
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb
from broadway_amd.engine import rotated_box_warp

CASES = _crop.cases()
CAP = 32                    # warps per kernel launch (H264MI_WARPS_MAX_PER_LAUNCH)
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}       # test_rois.py's layouts
ORDER = [2, 0, 2]           # the picture list of every kernel test
SUB = (6, 2, 38, 26)        # a proper sub-window: neighbours just outside it exist and must not be read
SIZES = [(7, 5), (9, 64), (33, 17)]     # each crosses 32 x 8 tile edges with partial tiles
PAD = (114, 7, 250)
SENTINEL = 0xA5
FRONT = 64
Q = 65536
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


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
    test_rois.py's."""
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def mixed(win, size):
    """The mixed list of a window and size, [(k, m), ...] with k into ORDER."""
    _, _, cw, ch = win
    oh, ow = size
    mats = [
        W.IDENTITY,
        (Q, 0, Q // 2, 0, Q, Q // 2),                                       # half a sample right and down
        (0, -Q, (cw - 1) * Q, Q, 0, 0),                                     # a quarter turn
        rotated_box_warp(cw / 2, ch / 2, 1.3 * cw, 1.3 * ch, 30, size),     # 30 degrees, 1.3 times the window: corners outside
        rotated_box_warp(cw / 2, ch / 2, 3 * ow, 3 * oh, -17, size),        # a 3 : 1 shrink, turned
        (-Q + 77, 0, (cw - 1) * Q - 12345, 123, -Q, (ch - 1) * Q + 4321),   # a flip: negative coefficients, floor shifts
    ]
    return [(r % 3, m) for r, m in enumerate(mats)]


def make_desc(size, mode, dtype, window, consts="unit", colour=0, border=0, pad=(0, 0, 0), layout=0, filt=0):
    from broadway_amd import _lib
    d = _lib.TensorWarpDesc()
    d.t.x, d.t.y, d.t.cw, d.t.ch = window
    d.t.mode = {"rgb": 0, "gray": 1}[mode] | colour << 8
    d.t.dtype = T.DTYPES.index(dtype) if dtype in T.DTYPES else dtype
    scale, bias = T.CONSTS[consts]
    d.t.scale[:] = scale
    d.t.bias[:] = bias
    d.oh, d.ow = size
    d.filter, d.border, d.layout = filt, border, layout
    d.pad[:] = tuple(pad) + (0,) * (4 - len(pad))
    return d


def make_warps(warps):
    from broadway_amd import _lib
    return (_lib.Warp * max(len(warps), 1))(*[_lib.Warp(k, (C.c_int * 6)(*m)) for k, m in warps])


def run_warps(pics, order, w, h, cp, warps, size, mode, dtype, window, consts="unit", colour=0, border=0, pad=(0, 0, 0),
              layout=0, in_pad=0, out_pad=0, skew=0, filt=0, null=(), stride=None, nwarps=None, host_out=False):
    """h264mi_tensor_warps_device_pitch over `warps` on pictures `order` of
    `pics`; returns rc, the whole output buffer (FRONT + skew sentinel bytes,
    then warps out_stride apart, then 64 sentinel bytes), the first warp's
    offset, out_stride and a warp's bytes (test_rois.py's run_rois)."""
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
    nb = max(len(warps), 1)
    d_out = torch.full((first + max(out_stride, nbytes) * nb + 64,), SENTINEL, dtype=torch.uint8,
                       device="cpu" if host_out else "cuda")
    assert d_out.data_ptr() % 16 == 0
    desc = make_desc(size, mode, dtype, window, consts, colour, border, pad, layout, filt)
    rc = L.h264mi_tensor_warps_device_pitch(None if "in" in null else d_in.data_ptr(),
                                            None if "offs" in null else offs, len(order), w, h, cp,
                                            None if "desc" in null else C.byref(desc),
                                            None if "warps" in null else make_warps(warps),
                                            len(warps) if nwarps is None else nwarps,
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


def check_list(pics, out, first, stride, nbytes, w, h, cp, warps, size, mode, dtype, window, consts="unit", colour=0,
               border=0, pad=(0, 0, 0), layout=0, order=ORDER):
    """Every warp equals the oracle and no byte outside the K outputs changed."""
    assert (out[:first] == SENTINEL).all()
    for r, (k, m) in enumerate(warps):
        o = first + r * stride
        want = W.expect(pics[order[k]], w, h, cp, window, m, size, mode, dtype, consts, colour, border, pad, hwc=layout == 1)
        assert same(out[o:o + nbytes], want), (r, k, m, size, window, border)
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), (r, k, m, size)
    assert (out[first + len(warps) * stride:] == SENTINEL).all()


def consts_of(dtype):
    return ["unit"] if dtype == "uint8" else ["unit", "imagenet"]        # uint8 ignores scale and bias


def windows_of(pic):
    w, h, _ = PICS[pic]
    return [(0, 0, w, h), SUB]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_identity_is_the_unresized_export(pictures, mode, dtype):
    """The identity at (ch, cw) == h264mi_tensor_device_pitch of the window --
    and interleaved == h264mi_tensor_layout_device_pitch's --, under either
    border (no border tap has weight), colours 0 and 3."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    zero = (C.c_size_t * 1)(0)
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        pics = pictures[pic]
        d_in = torch.from_numpy(np.array(pics[ORDER[1]])).to("cuda")
        for win in windows_of(pic):
            size = (win[3], win[2])
            nb = T.MODES[mode] * win[2] * win[3] * T.ELEM[dtype]
            for colour in ((0, 3) if mode == "rgb" else (0,)):
                for layout in ((0, 1) if mode == "rgb" else (0,)):
                    ld = _lib.TensorLayoutDesc()
                    ld.f.r.t = make_desc(size, mode, dtype, win, "imagenet", colour).t
                    ld.layout = layout
                    plain = torch.zeros(nb, dtype=torch.uint8, device="cuda")
                    if layout:
                        assert L.h264mi_tensor_layout_device_pitch(d_in.data_ptr(), zero, 1, w, h, cp, C.byref(ld), None, 0,
                                                                   plain.data_ptr(), nb, st) == 0
                    else:
                        assert L.h264mi_tensor_device_pitch(d_in.data_ptr(), zero, 1, w, h, cp, C.byref(ld.f.r.t),
                                                            plain.data_ptr(), nb, st) == 0
                    for border, pad in ((0, PAD), (1, (0, 0, 0))):
                        rc, out, first, _, nbytes = run_warps(pics, ORDER, w, h, cp, [(1, W.IDENTITY)], size, mode, dtype,
                                                              win, "imagenet", colour, border, pad, layout)
                        assert rc == 0 and nbytes == nb
                        assert same(out[first:first + nb], plain.cpu().numpy()), (pic, win, colour, layout, border)
                        assert (out[:first] == SENTINEL).all() and (out[first + nb:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_mixed_list_in_one_launch_vs_oracle(pictures, mode, dtype):
    """Identity, half-sample shift, quarter turn, a 30-degree rotation with its
    corners outside, a 3 : 1 shrink with rotation and a flip, in one launch, on
    the whole picture and on a proper sub-window, both borders, pad (114, 7,
    250), on unit and imagenet constants; colour 3 and the interleaved layout on
    the unit constants."""
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        for win in windows_of(pic):
            for size in SIZES:
                warps = mixed(win, size)
                for border, pad in ((0, PAD), (1, (0, 0, 0))):
                    variants = [(c, 0, 0) for c in consts_of(dtype)]
                    if mode == "rgb":
                        variants += [("unit", 3, 0), ("unit", 0, 1)]
                    for consts, colour, layout in variants:
                        rc, out, first, stride, nbytes = run_warps(pictures[pic], ORDER, w, h, cp, warps, size, mode, dtype,
                                                                   win, consts, colour, border, pad, layout)
                        assert rc == 0, (pic, win, size, consts, colour, border)
                        check_list(pictures[pic], out, first, stride, nbytes, w, h, cp, warps, size, mode, dtype, win,
                                   consts, colour, border, pad, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("gray", "uint8"), ("rgb", "float16")])
def test_far_outside_and_degenerate_matrices(pictures, mode, dtype):
    """All zero (one point), m2 = INT32_MAX and m0 = INT32_MIN (far outside),
    every coefficient extreme, and maps that leave the window after the first
    tile, to the right and downwards: pad elements or edge samples, as the
    oracle says.  (tests/test_warp_geom.py proves on the CPU that none of them
    names a position outside the window.)"""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    warps = [(0, (0, 0, 0, 0, 0, 0)), (1, (Q, 0, INT_MAX, 0, Q, 0)), (2, (INT_MIN, 0, 0, 0, Q, 0)),
             (0, (INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX)), (1, (2 * Q, 0, 0, 0, Q, 0)),
             (2, (Q, 0, 0, 0, 5 * Q, 0)), (0, (Q, 0, -40 * Q, 0, Q, -9 * Q)), (1, (0, 0, 3 * Q + 100, 0, 0, -Q // 3))]
    for win in windows_of("48x32_pitch128"):
        for size in ((9, 64), (33, 17)):
            for border, pad in ((0, PAD), (1, (0, 0, 0))):
                rc, out, first, stride, nbytes = run_warps(pics, ORDER, w, h, cp, warps, size, mode, dtype, win, "imagenet",
                                                           0, border, pad)
                assert rc == 0
                check_list(pics, out, first, stride, nbytes, w, h, cp, warps, size, mode, dtype, win, "imagenet", 0,
                           border, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("gray", "uint8"), ("rgb", "float16"), ("rgb", "float32")])
def test_list_longer_than_one_launch_and_padded_strides(pictures, mode, dtype):
    """33 distinct warps (the 33rd is the second launch), input pictures 37
    bytes apart; out_stride padded by 5 elements, by 48 bytes, and by 48 bytes
    with d_out one element past a 16-byte boundary: nothing else is written."""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    warps = [(r % 3, rotated_box_warp(8 + r, 6 + r % 20, 12 + r % 7, 9, 11 * r, (5, 6))) for r in range(CAP + 1)]
    assert len(set(warps)) == CAP + 1
    es = T.ELEM[dtype]
    for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
        rc, out, first, stride, nbytes = run_warps(pics, ORDER, w, h, cp, warps, (5, 6), mode, dtype, SUB, "imagenet", 0, 0,
                                                   PAD, in_pad=37, out_pad=out_pad, skew=skew)
        assert rc == 0 and stride == nbytes + out_pad and first == FRONT + skew
        check_list(pics, out, first, stride, nbytes, w, h, cp, warps, (5, 6), mode, dtype, SUB, "imagenet", 0, 0, PAD)


# the refused rows of tests/test_warp_desc.py's grid, on three pictures of 96 x 64: keywords over the good call
GOOD4 = [(0, W.IDENTITY), (1, (0, 0, 0, 0, 0, 0)), (2, (INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX)),
         (0, (-Q, 0, 95 * Q, 0, -Q, 63 * Q))]
WHOLE = (0, 0, 96, 64)
REFUSED = {
    "nwarps_0": {"nwarps": 0},
    "nwarps_negative": {"nwarps": -1},
    "pic_npics_last": {"warps": GOOD4[:3] + [(3, W.IDENTITY)]},
    "pic_minus_1_last": {"warps": GOOD4[:3] + [(-1, W.IDENTITY)]},
    "window_empty": {"window": (0, 0, 0, 0)},
    "x_odd": {"window": (1, 0, 94, 64)},
    "y_odd": {"window": (0, 1, 96, 62)},
    "cw_odd": {"window": (0, 0, 95, 64)},
    "ch_odd": {"window": (0, 0, 96, 63)},
    "right_plus_2": {"window": (2, 0, 96, 64)},
    "bottom_plus_2": {"window": (0, 2, 96, 64)},
    "x_negative": {"window": (-2, 0, 8, 64)},
    "ch_negative": {"window": (0, 0, 96, -2)},
    "ow_0": {"size": (8, 0)},
    "oh_0": {"size": (0, 8)},
    "ow_max_plus_1": {"size": (8, 16385)},
    "oh_max_plus_1": {"size": (16385, 8)},
    "filter_1": {"filt": 1},
    "border_2": {"border": 2},
    "border_minus_1": {"border": -1},
    "pad3_set": {"pad": (114, 7, 250, 1)},
    "replicate_with_pad": {"border": 1},
    "replicate_with_pad2": {"border": 1, "pad": (0, 0, 250)},
    "layout_2": {"layout": 2},
    "dtype_i16": {"dtype": 4},
    "dtype_minus_1": {"dtype": -1},
    "window_16386": {"window": (0, 0, 16386, 2), "geom": (16400, 16, 8200)},
}


@pytest.mark.gpu
def test_refusals_launch_nothing():
    import test_warp_desc
    assert sorted(REFUSED) == sorted(k for k, v in test_warp_desc.WARPS.items() if v == test_warp_desc.R)
    rng = np.random.default_rng(29)
    made = {}

    def run(**kw):
        args = dict(warps=GOOD4, size=(8, 8), mode="rgb", dtype="float16", window=WHOLE, pad=PAD)
        args.update(kw)
        w, h, cp = args.pop("geom", (96, 64, 48))
        if (w, h) not in made:
            made[(w, h)] = [rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for _ in range(3)]
        return run_warps(made[(w, h)], [0, 1, 2], w, h, cp, args.pop("warps"), args.pop("size"), args.pop("mode"),
                         args.pop("dtype"), args.pop("window"), **args), made[(w, h)]

    (rc, out, first, stride, nbytes), pics = run()
    assert rc == 0                                       # the arguments below are one step away
    check_list(pics, out, first, stride, nbytes, 96, 64, 48, GOOD4, (8, 8), "rgb", "float16", WHOLE, pad=PAD, order=[0, 1, 2])
    (rc, out, *_), _ = run(window=(0, 0, 16384, 2), geom=(16400, 16, 8200))      # exactly 16384 a side is accepted
    assert rc == 0
    for name, kw in sorted(REFUSED.items()):
        (rc, out, *_), _ = run(**kw)
        assert rc == -1, name
        assert (out == SENTINEL).all(), name             # nothing was launched
    for null in ("in", "offs", "desc", "warps", "out"):
        (rc, out, *_), _ = run(null=(null,))
        assert rc == -1 and (out == SENTINEL).all(), null
    (rc, out, *_), _ = run(host_out=True)                # d_out on no device
    assert rc == -1 and (out == SENTINEL).all()
    (rc, out, *_), _ = run(skew=1)                       # d_out not a multiple of the element size
    assert rc == -1 and (out == SENTINEL).all()
    (rc, out, *_), _ = run(stride=3 * 8 * 8 * 2 + 1)
    assert rc == -1 and (out == SENTINEL).all()
    (rc, out, *_), _ = run(colour=15)                    # STREAM: the engine-level calls know no stream
    assert rc == -1 and (out == SENTINEL).all()


def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
def test_engine_to_tensor_warps_vs_reference_decoder():
    """Warps over two slots with a caller stream, out= and colour
    "bt709-full", against the reference decoder's pictures; a decode into one
    of the named slots queued right behind the export does not change the
    exported bytes; a bad slot is a RuntimeError, a wrong out a ValueError."""
    import torch
    from broadway_amd.engine import Capture, Engine
    name = "crop_ltrb_6x4"          # the smallest case: 96 x 64
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16) == (96, 64)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    size = (9, 13)
    win = (6, 2, 86, 52)
    warps = [(1, W.IDENTITY), (0, rotated_box_warp(43, 26, 40, 30, 30, size)), (1, rotated_box_warp(80, 45, 30, 30, -45, size)),
             (0, (0, -Q, 85 * Q, Q, 0, 0)), (0, (Q, 0, Q // 2, 0, Q, -Q // 2))]
    # the first later picture that is decoded into the slot of an earlier one
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    first = slots[:again].index(slots[again])
    other = next((k for k in range(again) if k != first), first)
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    held = [first, other]                               # (no slot was reused yet: they hold these pictures)
    out = torch.empty((len(warps), 3) + size, dtype=torch.float32, device="cuda")
    scale, bias = T.CONSTS["imagenet"]
    got = eng.to_tensor([0, 0], [slots[k] for k in held], warps=warps, size=size, window=win, dtype=torch.float32,
                        scale=scale, bias=bias, out=out, stream=side, colour="bt709-full", pad=PAD)
    eng.decode([0], [cap.pictures[again]])              # overwrites slots[first]: it waits for the export
    gray = eng.to_tensor([0], [slots[again]], warps=[(0, rotated_box_warp(48, 32, 60, 40, 10, (11, 7)))], size=(11, 7),
                         mode="gray", dtype=torch.uint8, border="replicate", layout="nhwc")
    torch.cuda.synchronize()
    assert got is out and eng.errors() == 0
    for r, (k, m) in enumerate(warps):
        want = W.frame_expect(frames[held[k]], w, h, win, m, size, "rgb", "float32", "imagenet", 3, W.CONSTANT, PAD)
        assert same(tensor_bytes(out[r]), want), r
    assert tuple(gray.shape) == (1, 1, 11, 7)
    assert same(tensor_bytes(gray), W.frame_expect(frames[again], w, h, (0, 0, 96, 64), rotated_box_warp(48, 32, 60, 40, 10, (11, 7)),
                                                   (11, 7), "gray", "uint8", "unit", 0, W.REPLICATE))
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0], [0, 1], warps=warps, size=size, out=torch.empty((len(warps), 3, 13, 9), device="cuda",
                                                                            dtype=torch.float16))
    with pytest.raises(RuntimeError):
        eng.to_tensor([0, 0], [0, eng.nslots], warps=warps, size=size)      # the library refuses the slot


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
@pytest.mark.parametrize("opts", [{"tensor": {"size": (13, 11)}}, {}], ids=["tensor", "plain"])
def test_decoder_warps_in_the_callback(opts):
    """A rotated box over the delivered (crop) window equals the oracle at the
    crop-offset window; REPLICATE at the crop edge repeats the crop window's
    edge, not the picture's rows and columns beyond it (a map that runs off
    every side of the window), and a caller's window inside it is moved by the
    crop offset."""
    import torch
    name = "crop_ltrb_6x4"
    win = sps_window(CASES[name])
    assert win == (6, 2, 86, 52)
    frames, _, w, h, _ = O.decode(case_stream(name))
    size = (12, 10)
    box = rotated_box_warp(43, 26, 50, 36, 25, size)
    off = (Q * 11, 0, -7 * Q, 0, Q * 6, -4 * Q + 300)       # columns -7 .. 92 of 86 and rows -4 .. 62 of 52: off all four sides
    inner = (4, 2, 80, 48)
    got = []

    def on_picture(dec, k, buf, pw, ph):
        got.append(dec.warps([box, off], size, dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD, pad=PAD))
        got.append(dec.warps([off, box], size, mode="gray", dtype=torch.uint8, border="replicate"))
        got.append(dec.warps([off], size, window=inner, dtype=torch.uint8, border="replicate", layout="nhwc"))

    n = run_decoder(case_stream(name), dict(opts), on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) and len(got) == 3 * n
    at = (inner[0] + win[0], inner[1] + win[1], inner[2], inner[3])
    for k in range(n):
        t, g, i = got[3 * k:3 * k + 3]
        assert tuple(t.shape) == (2, 3) + size and t.dtype == torch.float16 and t.is_cuda
        assert tuple(g.shape) == (2, 1) + size and g.dtype == torch.uint8 and tuple(i.shape) == (1, 3) + size
        for r, m in enumerate((box, off)):
            assert same(tensor_bytes(t[r]), W.frame_expect(frames[k], w, h, win, m, size, "rgb", "float16", "imagenet", 0,
                                                           W.CONSTANT, PAD)), (k, r)
            assert same(tensor_bytes(g[1 - r]), W.frame_expect(frames[k], w, h, win, m, size, "gray", "uint8", "unit", 0,
                                                               W.REPLICATE)), (k, r)
        want = W.frame_expect(frames[k], w, h, at, off, size, "rgb", "uint8", "unit", 0, W.REPLICATE)
        assert same(tensor_bytes(i[0]), want), k        # (.contiguous() of a channels_last tensor: the planar bytes)
        # (this stream tells the two apart: with the two picture rows above the crop window let in, the bytes differ)
        above = W.frame_expect(frames[k], w, h, (win[0], 0, win[2], win[3] + win[1]),
                               (off[0], 0, off[2], 0, off[4], off[5] + win[1] * Q), size, "gray", "uint8", "unit", 0, W.REPLICATE)
        assert not np.array_equal(tensor_bytes(g[0]), above), k


@pytest.mark.gpu
def test_decoder_warps_return_codes():
    """H264SwDecLastPictureTensorWarps: OK before any picture and after the
    next H264SwDecDecode, PARAM_ERR for a window over the crop edge, pic = 1, no
    warps and a bad border, PIC_RDY on success; Decoder.warps raises
    RuntimeError where the call answers OK."""
    import torch
    from broadway_amd import _lib
    name = "crop_ltrb_6x4"          # two slices a picture: the NAL after a picture's last delivers nothing
    nals = split_annexb(case_stream(name))
    dec = Decoder()
    L = dec._L
    out = torch.full((2 * 3 * 4 * 4,), 7, dtype=torch.float16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(warps, window=(0, 0, 0, 0), **kw):
        desc = make_desc((4, 4), "rgb", "float16", window, **kw)
        return L.H264SwDecLastPictureTensorWarps(dec._inst, C.byref(desc), make_warps(warps), len(warps), out.data_ptr(), st)

    good = [(0, W.IDENTITY), (0, (INT_MIN, INT_MAX, 0, 0, 0, INT_MIN))]
    assert call(good) == _lib.H264SWDEC_OK                          # before the headers
    assert call(good, border=2) == _lib.H264SWDEC_PARAM_ERR         # a bad descriptor even then
    with pytest.raises(RuntimeError):
        dec.warps([W.IDENTITY], (4, 4))
    inside = []

    def cb(buf, w, h, infos):
        inside.append((call(good), call(good, (4, 2, 82, 50)), call(good, (4, 2, 84, 50)), call(good, (4, 2, 82, 52)),
                       call(good, (1, 0, 4, 4)), call([(1, W.IDENTITY)]), call(good[:1] + [(-1, W.IDENTITY)]), call([]),
                       call(good, border=2)))

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
                dec.warps([W.IDENTITY], (4, 4))
    torch.cuda.synchronize()
    assert len(delivered_at) >= 2 and len(delivered_at) < len(nals) - 2
    P, Y = _lib.H264SWDEC_PARAM_ERR, _lib.H264SWDEC_PIC_RDY
    assert set(inside) == {(Y, Y, P, P, P, P, P, P, P)}
    dec.close()
