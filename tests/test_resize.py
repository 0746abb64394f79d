"""Resized tensor export (resize.hip): the crop window's planes
filtered to (oh, ow) by an antialiased triangle filter in integer arithmetic,
then converted as the unresized export converts --
h264mi_tensor_resize_device_pitch, h264mi_engine_export_tensor_resized
(Engine.to_tensor(size=)) and H264SwDecNextPictureTensorResized (Decoder's
``tensor: {"size": ...}``).

The oracle (tests/_resize.py) restates the arithmetic in Python integers on top
of tests/_tensor.py.  Every comparison with it is exact equality of bytes."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import _crop
import _resize as R
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CASES = _crop.cases()
CAP = 32                    # pictures per kernel launch (TENSOR_MAX_PICS)


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


# ------------------------------------------------------------------ CPU ----
# (ch, cw, oh, ow)
TORCH_SHAPES = [(26, 38, 7, 5), (32, 46, 32, 46), (26, 38, 52, 76), (26, 38, 9, 64), (52, 86, 13, 11), (2, 2, 5, 3),
                (32, 256, 3, 8), (32, 46, 31, 45), (64, 64, 2, 2)]


def test_oracle_is_torch_antialiased_bilinear():
    """The integer arithmetic is torch's antialiased bilinear interpolation
    (float64, half-pixel centres) with one final rounding: within half a
    sample plus the 6-bit intermediate's 1/64."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    for ch, cw, oh, ow in TORCH_SHAPES:
        plane = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        got = R.resize(plane, oh, ow)
        ref = F.interpolate(torch.from_numpy(plane.astype(np.float64))[None, None], size=(oh, ow), mode="bilinear",
                            antialias=True, align_corners=False)[0, 0].numpy()
        worst = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"({ch},{cw})->({oh},{ow}): max |oracle - torch| = {worst:.4f}")
        assert worst <= 0.5 + 1 / 64, (ch, cw, oh, ow)
        if (oh, ow) == (ch, cw):
            assert np.array_equal(got, plane)


@pytest.mark.parametrize("n,m", [(1920, 224), (1080, 224), (256, 8), (2, 64), (46, 45), (3840, 120)])
def test_taps_invariants(n, m):
    tp = R.taps(n, m)
    assert len(tp) == m
    most = 0
    for first, q in tp:
        assert 0 <= first and first + q.size <= n and q.size >= 1        # contiguous by construction, inside [0, n)
        assert (q >= 0).all() and int(q.sum()) == 16384
        most = max(most, q.size)
    assert most <= R.MAX_TAPS
    if (n, m) in ((256, 8), (3840, 120)):
        assert most == R.MAX_TAPS


def test_library_exports_the_resize_entry_points():
    from broadway_amd import _lib
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_resize_device_pitch", 10), ("h264mi_engine_export_tensor_resized", 8),
                        ("H264SwDecNextPictureTensorResized", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { h264mi_tensor_desc t; int ow, oh, filter; }
    assert C.sizeof(_lib.TensorResizeDesc) == 60
    assert _lib.TensorResizeDesc.ow.offset == 48 and _lib.TensorResizeDesc.oh.offset == 52
    assert _lib.TensorResizeDesc.filter.offset == 56


def test_python_surface_rejects_bad_sizes():
    from broadway_amd import _lib
    from broadway_amd.engine import tensor_desc
    with pytest.raises(ValueError):
        Decoder({"tensor": {"size": (4, 4)}, "rgb": True})
    for size in ((0, 4), (4,), (4, 0), (4, 16385), (1, 2, 3)):
        with pytest.raises(ValueError):
            tensor_desc((0, 0, 4, 4), size=size)
    d, planes, _ = tensor_desc((2, 4, 6, 8), mode="gray", size=(3, 5))
    assert isinstance(d, _lib.TensorResizeDesc) and (d.oh, d.ow, d.filter, planes) == (3, 5, 0, 1)
    assert (d.t.x, d.t.y, d.t.cw, d.t.ch) == (2, 4, 6, 8)
    assert isinstance(tensor_desc((2, 4, 6, 8))[0], _lib.TensorDesc)        # without size: today's object


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}
# (window, (oh, ow))
RESIZES = [((6, 2, 38, 26), (7, 5)), ((6, 2, 38, 26), (52, 76)), ((6, 2, 38, 26), (9, 64)), ((0, 0, 46, 32), (31, 45)),
           ((2, 2, 2, 2), (5, 3)), ((2, 2, 2, 2), (1, 1)), ((44, 30, 4, 2), (3, 3))]
WIDE_RESIZES = [((0, 0, 256, 32), (3, 8)), ((130, 0, 126, 32), (5, 9))]
BAD_WINDOWS = [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 50, 32), (46, 0, 4, 2),
               (0, 30, 2, 4), (-2, 0, 4, 4), (0, 0, 0, 2), (0, 0, 2, 0)]       # test_tensor.py's
SENTINEL = 0xA5
FRONT = 64


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 random pictures in the (width, cpitch) layout (read-only);
    test_tensor.py's."""
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def make_desc(win, size, mode, dtype, consts="unit", filt=0):
    from broadway_amd import _lib
    d = _lib.TensorResizeDesc()
    d.t.x, d.t.y, d.t.cw, d.t.ch = win
    d.t.mode = {"rgb": 0, "gray": 1}.get(mode, mode)
    d.t.dtype = T.DTYPES.index(dtype) if dtype in T.DTYPES else dtype
    scale, bias = T.CONSTS[consts]
    d.t.scale[:] = scale
    d.t.bias[:] = bias
    d.oh, d.ow = size
    d.filter = filt
    return d


def run_resize(pics, order, w, h, cp, win, size, mode, dtype, consts="unit", in_pad=0, out_pad=0, skew=0, filt=0,
               null=(), stride=None):
    """h264mi_tensor_resize_device_pitch over pictures `order` of `pics`;
    returns rc, the whole output buffer (FRONT + skew sentinel bytes, then
    pictures out_stride apart, then 64 sentinel bytes), the first picture's
    offset, out_stride and a picture's bytes (test_tensor.py's run_tensor)."""
    import torch
    L = _mi()
    es = T.ELEM.get(dtype, 1)
    oh, ow = size
    nbytes = T.MODES.get(mode, 3) * oh * ow * es if 0 < oh <= 512 and 0 < ow <= 512 else 16
    in_stride = pics[0].size + in_pad
    out_stride = nbytes + out_pad if stride is None else stride
    host = np.zeros(in_stride * len(pics), dtype=np.uint8)
    for k, p in enumerate(pics):
        host[k * in_stride:k * in_stride + p.size] = p
    d_in = torch.from_numpy(host).to("cuda")
    n = len(order)
    offs = (C.c_size_t * n)(*[k * in_stride for k in order])
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    desc = make_desc(win, size, mode, dtype, consts, filt)
    rc = L.h264mi_tensor_resize_device_pitch(None if "in" in null else d_in.data_ptr(),
                                             None if "offs" in null else offs, n, w, h, cp,
                                             None if "desc" in null else C.byref(desc),
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


def consts_of(dtype):
    return ["unit"] if dtype == "uint8" else ["unit", "imagenet"]        # uint8 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_kernel_vs_oracle(pictures, mode, dtype):
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        p = pictures[pic][0]
        for win, size in RESIZES + (WIDE_RESIZES if w == 256 else []):
            for consts in consts_of(dtype):
                rc, out, first, stride, nbytes = run_resize([p], [0], w, h, cp, win, size, mode, dtype, consts)
                assert rc == 0, (pic, win, size, consts)
                want = R.expect(p, w, h, cp, win, size, mode, dtype, consts)
                assert same(out[first:first + nbytes], want), (pic, win, size, consts)
                assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (pic, win, size)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_identity_size_is_the_unresized_export(pictures, pic, dtype):
    """(oh, ow) == (ch, cw): the bytes of h264mi_tensor_device_pitch on the
    same input."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    w, h, cp = PICS[pic]
    p = pictures[pic][0]
    d_in = torch.from_numpy(np.array(p)).to("cuda")
    offs = (C.c_size_t * 1)(0)
    for win in [(0, 0, w, h), (6, 2, 38, 26), (2, 2, 2, 2)]:
        for mode in sorted(T.MODES):
            rd = make_desc(win, (win[3], win[2]), mode, dtype, "imagenet")
            td = _lib.TensorDesc.from_buffer_copy(rd.t)
            nbytes = T.MODES[mode] * win[2] * win[3] * T.ELEM[dtype]
            plain = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            assert L.h264mi_tensor_device_pitch(d_in.data_ptr(), offs, 1, w, h, cp, C.byref(td), plain.data_ptr(),
                                                nbytes, torch.cuda.current_stream().cuda_stream) == 0
            rc, out, first, _, nb = run_resize([p], [0], w, h, cp, win, (win[3], win[2]), mode, dtype, "imagenet")
            assert rc == 0 and nb == nbytes
            assert same(out[first:first + nb], plain.cpu().numpy()), (win, mode)
            assert (out[:first] == SENTINEL).all() and (out[first + nb:] == SENTINEL).all(), (win, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_kernel_batched_padded_strides_write_nothing_else(pictures, mode, dtype):
    """Picture list [2, 0, 2] of three pictures 37 bytes apart; out_stride
    padded by 5 elements, by 48 bytes, and by 48 bytes with d_out one element
    past a 16-byte boundary: every picture is right and no pad byte changes."""
    es = T.ELEM[dtype]
    order = [2, 0, 2]
    win, size = (6, 2, 38, 26), (7, 5)
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_resize(pictures[pic], order, w, h, cp, win, size, mode, dtype,
                                                        "imagenet", in_pad=37, out_pad=out_pad, skew=skew)
            assert rc == 0, (pic, out_pad, skew)
            assert (out[:first] == SENTINEL).all(), (pic, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                want = R.expect(pictures[pic][i], w, h, cp, win, size, mode, dtype, "imagenet")
                assert same(out[o:o + nbytes], want), (pic, out_pad, skew, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (pic, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (pic, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_kernel_list_longer_than_one_launch(pictures, dtype):
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win, size = (6, 2, 38, 26), (7, 5)
    rc, out, first, stride, nbytes = run_resize(pics, order, w, h, cp, win, size, "rgb", dtype, "imagenet", in_pad=37,
                                                out_pad=5 * T.ELEM[dtype])
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], R.expect(pics[i], w, h, cp, win, size, "rgb", dtype, "imagenet")), k
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
def test_kernel_rejects_bad_arguments(pictures):
    good_win, good_size = (2, 2, 4, 4), (3, 5)

    def refused(pic="48x32_pitch128", **kw):
        w, h, cp = PICS[pic]
        args = dict(win=good_win, size=good_size, mode="rgb", dtype="float16")
        args.update(kw)
        win, size, mode, dtype = args.pop("win"), args.pop("size"), args.pop("mode"), args.pop("dtype")
        rc, out, *_ = run_resize(pictures[pic][:1], [0], w, h, cp, win, size, mode, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    w, h, cp = PICS["48x32_pitch128"]
    rc, out, first, _, nbytes = run_resize(pictures["48x32_pitch128"][:1], [0], w, h, cp, good_win, good_size, "rgb",
                                           "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    for bad in (0, -1, 16385):
        refused(size=(bad, 5))
        refused(size=(3, bad))
    rc, out, first, _, nbytes = run_resize(pictures["256x32_packed"][:1], [0], 256, 32, 128, (0, 0, 256, 32), (3, 8),
                                           "gray", "uint8")
    assert rc == 0                                       # 32 : 1 is the cap,
    refused(pic="256x32_packed", win=(0, 0, 256, 32), size=(3, 7))              # beyond it is refused
    refused(filt=1)
    for win in BAD_WINDOWS:
        for mode in sorted(T.MODES):
            refused(win=win, mode=mode)
    for null in ("in", "offs", "desc", "out"):
        refused(null=(null,))
    refused(dtype="float16", skew=1)                     # d_out not a multiple of the element size
    refused(dtype="bfloat16", skew=1)
    refused(dtype="float32", skew=2)
    refused(dtype="float16", stride=3 * 3 * 5 * 2 + 1)   # nor out_stride
    refused(dtype="float32", stride=3 * 3 * 5 * 4 + 2)


def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def frame_expect(frame, w, h, win, size, mode, dtype, consts):
    x, y, cw, ch = win
    scale, bias = T.CONSTS[consts]
    c = T.samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode)
    return T.convert(R.resize_planes(c, size[0], size[1]), dtype, scale, bias)


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crop_ltrb_6x4", "crop_r_16x3"])
def test_engine_to_tensor_resized_vs_reference_decoder(name):
    """Every picture exported resized right behind its launch, on a side
    stream and with one synchronisation at the end; the DPB reuses slots over
    these streams, so an export that did not order itself against the next
    launch would hold a later picture."""
    import torch
    from broadway_amd.engine import Capture, Engine
    c = CASES[name]
    win = sps_window(c)
    size = (13, 11)
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    kinds = [("rgb", torch.float16, "imagenet"), ("rgb", torch.uint8, "unit"), ("gray", torch.bfloat16, "unit"),
             ("rgb", torch.float32, "unit"), ("gray", torch.float32, "imagenet")]
    got = []
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        mode, dtype, consts = kinds[k % len(kinds)]
        scale, bias = T.CONSTS[consts]
        got.append(eng.to_tensor([0], [pic.cur_slot], window=win, mode=mode, dtype=dtype, scale=scale, bias=bias,
                                 stream=side, size=size))
    if name == "crop_ltrb_6x4":
        assert len({pic.cur_slot for pic in cap.pictures}) < cap.npics       # a slot was reused
    torch.cuda.synchronize()
    assert eng.errors() == 0
    for k, t in enumerate(got):
        mode, dtype, consts = kinds[k % len(kinds)]
        assert tuple(t.shape) == (1, T.MODES[mode]) + size and t.dtype == dtype and t.is_cuda
        want = frame_expect(frames[k], w, h, win, size, mode, str(dtype).split(".")[1], consts)
        assert same(tensor_bytes(t), want), k
    # out=: the resized shape is the one that fits
    slot = cap.pictures[-1].cur_slot
    out = torch.empty((1, 3) + size, dtype=torch.float16, device="cuda")
    assert eng.to_tensor([0], [slot], window=win, out=out, size=size) is out
    torch.cuda.synchronize()
    assert same(tensor_bytes(out), frame_expect(frames[-1], w, h, win, size, "rgb", "float16", "unit"))
    for bad in (torch.empty((1, 3, win[3], win[2]), dtype=torch.float16, device="cuda"),
                torch.empty((1, 3, size[1], size[0]), dtype=torch.float16, device="cuda"),
                torch.empty((1, 3) + size, dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            eng.to_tensor([0], [slot], window=win, out=bad, size=size)
    with pytest.raises(RuntimeError):
        eng.to_tensor([0], [slot], window=(0, 0, w, 2), size=(1, 1))      # beyond 32 : 1 on the x axis


def decode_js(nals, opts):
    got, dims = [], []
    dec = Decoder(opts)
    dec.onPictureDecoded = lambda buf, w, h, infos: (got.append(buf), dims.append((w, h)))
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, dims


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(26, 43), (104, 172)])
def test_decoder_tensor_size_option_vs_reference(size):
    import torch
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    assert win[2:] == (86, 52)
    frames, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    nals = split_annexb(case_stream("crop_ltrb_6x4"))
    got, dims = decode_js(nals, {"tensor": {"dtype": torch.float16, "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD,
                                            "size": size}})
    gray, gdims = decode_js(nals, {"tensor": {"dtype": torch.uint8, "mode": "gray", "size": size}})
    assert len(got) == len(gray) == len(frames) and set(dims) == set(gdims) == {(size[1], size[0])}
    for k, (t, g) in enumerate(zip(got, gray)):
        assert t.dtype == torch.float16 and tuple(t.shape) == (3,) + size and t.is_cuda
        assert g.dtype == torch.uint8 and tuple(g.shape) == (1,) + size and g.is_cuda
        assert same(tensor_bytes(t), frame_expect(frames[k], w, h, win, size, "rgb", "float16", "imagenet")), k
        assert same(tensor_bytes(g), frame_expect(frames[k], w, h, win, size, "gray", "uint8", "unit")), k
