"""Decoded pictures as device tensors (tensor.hip): planar RGB / luma of the
crop window as uint8, fp16, bf16 or fp32 in the caller's device memory --
h264mi_tensor_device_pitch, h264mi_engine_export_tensor (Engine.to_tensor) and
H264SwDecNextPictureTensor (Decoder's ``tensor`` option).

The oracle (tests/_tensor.py) is numpy / torch-CPU on top of _crop.crop_i420
and oracle.yuv2rgba.  Every comparison is exact equality of bytes."""
import ctypes as C
import hashlib
from fractions import Fraction

import numpy as np
import pytest

import oracle as O
import _crop
import _golden
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb
from broadway_amd.engine import tensor_affine

CASES = _crop.cases()
SMALL = ["crop_ltrb_6x4", "crop_r_16x3"]
CAP = 32                    # pictures per kernel launch (TENSOR_MAX_PICS)


def case_stream(name):
    c = CASES[name]
    s = gen.generate(c["config"], c["seed"], **c["overrides"])
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


def head_nals(stream, case):
    nals = split_annexb(stream)
    if len(case["frames"]) == case["frames_total"]:
        return nals
    return nals[:2 + case["overrides"].get("slices", 4) * len(case["frames"])]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_crop.py: the decoder instances here pool engines of
    several sizes; test_swdec_pooled_engines_vs_reference counts on finding
    room for its own."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


# ------------------------------------------------------------------ CPU ----
def test_exactness_premise():
    """For every constant set of these tests, all 256 samples and all three
    planes, float64(c) * float64(scale) + float64(bias) is exact (an 8-bit x
    24-bit product plus a 24-bit addend), so the oracle's one rounding to fp32
    is the rounding of a fused multiply-add."""
    for name, (scale, bias) in T.CONSTS.items():
        for p in range(3):
            s, b = np.float64(np.float32(scale[p])), np.float64(np.float32(bias[p]))
            assert float(s) == scale[p] and float(b) == bias[p], name       # fp32-representable
            for c in range(256):
                exact = Fraction(c) * Fraction(float(s)) + Fraction(float(b))
                assert Fraction(float(np.float64(c) * s + b)) == exact, (name, p, c)


def test_tensor_affine_matches_the_formula():
    scale, bias = tensor_affine(T.IMAGENET_MEAN, T.IMAGENET_STD)
    for p in range(3):
        m, s = T.IMAGENET_MEAN[p], T.IMAGENET_STD[p]
        assert scale[p] == float(np.float32(1.0 / (255.0 * s))) and bias[p] == float(np.float32(-m / s))
        assert float(np.float32(scale[p])) == scale[p] and float(np.float32(bias[p])) == bias[p]
    assert tensor_affine((0, 0, 0), (1, 1, 1)) == ((float(np.float32(1 / 255)),) * 3, (0.0,) * 3)
    with pytest.raises(ValueError):
        tensor_affine((0.5, 0.5), (1, 1, 1))


@pytest.mark.parametrize("other", ["rgb", "crop"])
def test_decoder_rejects_tensor_with_rgb_or_crop(other):
    with pytest.raises(ValueError):
        Decoder({"tensor": True, other: True})
    with pytest.raises(ValueError):
        Decoder({"tensor": {"dtype": None}, other: True})


def test_library_exports_the_tensor_entry_points():
    from broadway_amd import _lib
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_device_pitch", 10), ("h264mi_engine_export_tensor", 8),
                        ("H264SwDecNextPictureTensor", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int x, y, cw, ch, mode, dtype; float scale[3], bias[3]; }
    assert C.sizeof(_lib.TensorDesc) == 6 * 4 + 6 * 4
    assert _lib.TensorDesc.scale.offset == 24 and _lib.TensorDesc.bias.offset == 36


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}
# (6, 2, 32, 26): 16-byte rows for every element type from x = 2 mod 4, x / 2 odd
WINDOWS = [None, (2, 2, 2, 2), (6, 2, 38, 26), (0, 0, 46, 32), (44, 30, 4, 2), (6, 2, 32, 26)]
WIDE_WINDOWS = [(252, 30, 4, 2), (130, 0, 126, 32)]
SENTINEL = 0xA5
FRONT = 64


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 random pictures in the (width, cpitch) layout (read-only)."""
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def make_desc(win, mode, dtype, consts="unit"):
    from broadway_amd import _lib
    d = _lib.TensorDesc()
    d.x, d.y, d.cw, d.ch = win
    d.mode = {"rgb": 0, "gray": 1}.get(mode, mode)
    d.dtype = T.DTYPES.index(dtype) if dtype in T.DTYPES else dtype
    scale, bias = T.CONSTS[consts]
    d.scale[:] = scale
    d.bias[:] = bias
    return d


def run_tensor(pics, order, w, h, cp, win, mode, dtype, consts="unit", in_pad=0, out_pad=0, skew=0, desc=None,
               cpitch=None, npics=None, null=(), stride=None):
    """h264mi_tensor_device_pitch over pictures `order` of `pics`; returns rc,
    the whole output buffer (FRONT + skew sentinel bytes, then pictures
    out_stride apart, then 64 sentinel bytes), the first picture's offset,
    out_stride and a picture's bytes."""
    import torch
    L = _mi()
    es = T.ELEM.get(dtype, 1)
    nbytes = T.MODES.get(mode, 3) * win[2] * win[3] * es if win[2] > 0 and win[3] > 0 else 16
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
    desc = desc if desc is not None else make_desc(win, mode, dtype, consts)
    rc = L.h264mi_tensor_device_pitch(None if "in" in null else d_in.data_ptr(), None if "offs" in null else offs,
                                      n if npics is None else npics, w, h, cp if cpitch is None else cpitch,
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
    return ["unit"] if dtype == "uint8" else sorted(T.CONSTS)       # uint8 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_vs_oracle(pictures, pic, mode, dtype):
    w, h, cp = PICS[pic]
    p = pictures[pic][0]
    for win in WINDOWS + (WIDE_WINDOWS if w == 256 else []):
        win = win or (0, 0, w, h)
        for consts in consts_of(dtype):
            rc, out, first, stride, nbytes = run_tensor([p], [0], w, h, cp, win, mode, dtype, consts)
            assert rc == 0, (win, consts)
            assert same(out[first:first + nbytes], T.expect(p, w, h, cp, win, mode, dtype, consts)), (win, consts)
            assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (win, consts)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_batched_padded_strides_write_nothing_else(pictures, pic, mode, dtype):
    """Picture list [2, 0, 2] of three pictures 37 bytes apart; out_stride
    padded by 5 elements (never a multiple of 16 bytes: the general path), by
    48 bytes (16-byte rows keep the 16-byte stores) and by 48 bytes with d_out
    one element past a 16-byte boundary: every picture is right and no pad
    byte changes, the first one past each picture included."""
    w, h, cp = PICS[pic]
    es = T.ELEM[dtype]
    order = [2, 0, 2]
    for win in [(6, 2, 38, 26), (0, 0, w, h), (2, 2, 2, 2), (6, 2, 32, 26)]:
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_tensor(pictures[pic], order, w, h, cp, win, mode, dtype, "imagenet",
                                                        in_pad=37, out_pad=out_pad, skew=skew)
            assert rc == 0, (win, out_pad, skew)
            assert (out[:first] == SENTINEL).all(), (win, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                want = T.expect(pictures[pic][i], w, h, cp, win, mode, dtype, "imagenet")
                assert same(out[o:o + nbytes], want), (win, out_pad, skew, k)
                assert out[o + nbytes] == SENTINEL, (win, out_pad, skew, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (win, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (win, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_kernel_list_longer_than_one_launch(pictures, dtype):
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win = (2, 2, 2, 2)
    rc, out, first, stride, nbytes = run_tensor(pics, order, w, h, cp, win, "rgb", dtype, "imagenet", in_pad=37)
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], T.expect(pics[i], w, h, cp, win, "rgb", dtype, "imagenet")), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_u8_is_the_crop_kernels_output(pictures, pic):
    """U8 / RGB = the de-interleaved bytes of h264mi_crop_device_pitch's RGBA
    on the same input; U8 / GRAY = the luma plane of its I420."""
    import torch
    L = _mi()
    w, h, cp = PICS[pic]
    p = pictures[pic][0]
    d_in = torch.from_numpy(np.array(p)).to("cuda")
    for win in [(0, 0, w, h), (6, 2, 38, 26), (2, 2, 2, 2)]:
        x, y, cw, ch = win
        crops = []
        for rgba in (1, 0):
            d = torch.zeros(cw * ch * 4, dtype=torch.uint8, device="cuda")
            assert L.h264mi_crop_device_pitch(d_in.data_ptr(), d.data_ptr(), w, h, cp, x, y, cw, ch, rgba, 1, 0, 0,
                                              torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            crops.append(d.cpu().numpy())
        rc, out, first, _, nbytes = run_tensor([p], [0], w, h, cp, win, "rgb", "uint8")
        want = crops[0].reshape(ch, cw, 4)[:, :, :3].transpose(2, 0, 1).reshape(-1)
        assert rc == 0 and np.array_equal(out[first:first + nbytes], want), win
        rc, out, first, _, nbytes = run_tensor([p], [0], w, h, cp, win, "gray", "uint8")
        assert rc == 0 and np.array_equal(out[first:first + nbytes], crops[1][:cw * ch]), win


BAD_WINDOWS = [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 50, 32), (46, 0, 4, 2),
               (0, 30, 2, 4), (-2, 0, 4, 4), (0, 0, 0, 2), (0, 0, 2, 0)]       # test_crop.py's


@pytest.mark.gpu
def test_kernel_rejects_bad_arguments(pictures):
    w, h, cp = PICS["48x32_pitch128"]
    p = pictures["48x32_pitch128"][:1]
    good = (2, 2, 4, 4)

    def refused(**kw):
        args = dict(win=good, mode="rgb", dtype="float16")
        args.update(kw)
        win, mode, dtype = args.pop("win"), args.pop("mode"), args.pop("dtype")
        rc, out, *_ = run_tensor(p, [0], w, h, cp, win, mode, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    rc, out, first, _, nbytes = run_tensor(p, [0], w, h, cp, good, "rgb", "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    for win in BAD_WINDOWS:
        for mode in sorted(T.MODES):
            refused(win=win, mode=mode)
    for null in ("in", "offs", "desc", "out"):
        refused(null=(null,))
    for mode in (2, -1):
        refused(mode=mode)
    for dtype in (4, -1):
        refused(dtype=dtype)
    refused(npics=0)
    refused(npics=-1)
    refused(cpitch=w // 2 - 1)
    refused(dtype="float16", skew=1)                     # d_out not a multiple of the element size
    refused(dtype="bfloat16", skew=1)
    refused(dtype="float32", skew=2)
    refused(dtype="float16", stride=3 * 4 * 4 * 2 + 1)   # nor out_stride
    refused(dtype="float32", stride=3 * 4 * 4 * 4 + 2)


def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def frame_expect(frame, w, h, win, mode, dtype, consts):
    x, y, cw, ch = win
    scale, bias = T.CONSTS[consts]
    return T.convert(T.samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode), dtype, scale, bias)


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_to_tensor_vs_reference_decoder(name):
    """Every picture exported right behind its launch, on a side stream and
    with no synchronisation until the end; the DPB reuses slots over these
    streams, so an export that did not order itself against the next launch
    would hold a later picture."""
    import torch
    from broadway_amd.engine import Capture, Engine
    c = CASES[name]
    win = sps_window(c)
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    assert (eng.chroma_pitch == w // 2) == (name == "crop_r_16x3")      # one padded slot layout, one packed
    side = torch.cuda.Stream()
    kinds = [("rgb", torch.float16, "imagenet"), ("rgb", torch.uint8, "unit"), ("gray", torch.bfloat16, "identity"),
             ("rgb", torch.float32, "unit"), ("gray", torch.float32, "imagenet")]
    got = []
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        mode, dtype, consts = kinds[k % len(kinds)]
        scale, bias = T.CONSTS[consts]
        got.append(eng.to_tensor([0], [pic.cur_slot], window=win, mode=mode, dtype=dtype, scale=scale, bias=bias,
                                 stream=side))
    if name == "crop_ltrb_6x4":
        assert len({pic.cur_slot for pic in cap.pictures}) < cap.npics       # a slot was reused
    torch.cuda.synchronize()
    assert eng.errors() == 0
    for k, t in enumerate(got):
        mode, dtype, consts = kinds[k % len(kinds)]
        assert tuple(t.shape) == (1, T.MODES[mode], win[3], win[2]) and t.dtype == dtype and t.is_cuda
        want = frame_expect(frames[k], w, h, win, mode, str(dtype).split(".")[1], consts)
        assert same(tensor_bytes(t), want), k
    # mean / std are tensor_affine's scale / bias; the default is 1 / 255
    slot = cap.pictures[-1].cur_slot
    a = eng.to_tensor([0], [slot], window=win, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD)
    b = eng.to_tensor([0], [slot])
    torch.cuda.synchronize()
    assert same(tensor_bytes(a), frame_expect(frames[-1], w, h, win, "rgb", "float16", "imagenet"))
    assert same(tensor_bytes(b), frame_expect(frames[-1], w, h, (0, 0, w, h), "rgb", "float16", "unit"))


@pytest.mark.gpu
def test_engine_to_tensor_batch_of_two_streams_and_out_checks():
    import torch
    from broadway_amd.engine import Capture, Engine
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    streams = [case_stream("crop_ltrb_6x4"), gen.generate(c["config"], c["seed"] + 1, **c["overrides"])]
    refs = [O.decode(s) for s in streams]
    caps = [Capture(s) for s in streams]
    w, h = refs[0][2], refs[0][3]
    eng = Engine(caps[0].w_mbs, caps[0].h_mbs, 2, max(cp.nslots for cp in caps))
    side = torch.cuda.Stream()
    got = []
    for k in range(min(cp.npics for cp in caps)):
        pics = [cp.pictures[k] for cp in caps]
        eng.decode([0, 1], pics)
        # (stream 1 first: the batch is a list of (stream, slot) pairs in any order)
        got.append(eng.to_tensor([1, 0], [pics[1].cur_slot, pics[0].cur_slot], window=win, dtype=torch.uint8,
                                 stream=side))
    torch.cuda.synchronize()
    assert eng.errors() == 0
    for k, t in enumerate(got):
        assert tuple(t.shape) == (2, 3, win[3], win[2])
        for j, s in enumerate((1, 0)):
            assert same(tensor_bytes(t[j]), frame_expect(refs[s][0][k], w, h, win, "rgb", "uint8", "unit")), (k, s)
    # out=: filled in place when it fits; refused on a wrong shape, dtype, device or layout
    slot = caps[0].pictures[-1].cur_slot
    shape = (1, 3, win[3], win[2])
    out = torch.empty(shape, dtype=torch.float16, device="cuda")
    assert eng.to_tensor([0], [slot], window=win, out=out) is out
    torch.cuda.synchronize()
    assert same(tensor_bytes(out), frame_expect(refs[0][0][-1], w, h, win, "rgb", "float16", "unit"))
    for bad in (torch.empty((1, 3, win[3], win[2] + 2), dtype=torch.float16, device="cuda"),
                torch.empty(shape, dtype=torch.float32, device="cuda"),
                torch.empty(shape, dtype=torch.float16, device="cpu"),
                torch.empty((1, 3, win[2], win[3]), dtype=torch.float16, device="cuda").transpose(2, 3)):
        with pytest.raises(ValueError):
            eng.to_tensor([0], [slot], window=win, out=bad)
    for kw in (dict(streams=[2], slots=[0]), dict(streams=[0], slots=[eng.nslots]),
               dict(streams=[0], slots=[0], window=(1, 0, 2, 2))):
        with pytest.raises(RuntimeError):
            eng.to_tensor(**kw)


def decode_js(nals, opts):
    got, dims = [], []
    dec = Decoder(opts)
    # (a host picture is a view of the decoder's buffer: copied here; a tensor is the caller's)
    dec.onPictureDecoded = lambda buf, w, h, infos: (got.append(bytes(buf) if isinstance(buf, np.ndarray) else buf),
                                                     dims.append((w, h)))
    for nal in nals:
        dec.decode(nal)
    flag = int(dec.info().croppingFlag)
    dec.close()
    return got, dims, flag


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_decoder_tensor_option_vs_reference(name):
    import torch
    c = CASES[name]
    cw, ch = c["cropParams"]["cropOutWidth"], c["cropParams"]["cropOutHeight"]
    nals = head_nals(case_stream(name), c)
    crop, cdims, flag = decode_js(nals, {"crop": True})
    crop = [bytes(f) for f in crop]
    assert flag == 1 and _golden.md5s(crop) == c["frames"]          # the cropped I420 the fixture pins
    got, dims, _ = decode_js(nals, {"tensor": {"dtype": torch.uint8, "mode": "rgb"}})
    assert len(got) == len(c["frames"]) and set(dims) == {(cw, ch)}
    for k, t in enumerate(got):
        assert tuple(t.shape) == (3, ch, cw) and t.dtype == torch.uint8 and t.is_cuda
        assert same(tensor_bytes(t), T.samples(crop[k], cw, ch, "rgb").reshape(-1)), k


@pytest.mark.gpu
def test_decoder_tensor_fp16_imagenet():
    import torch
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    frames, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    nals = split_annexb(case_stream("crop_ltrb_6x4"))
    got, dims, _ = decode_js(nals, {"tensor": {"dtype": torch.float16, "mean": T.IMAGENET_MEAN,
                                               "std": T.IMAGENET_STD}})
    dflt, _, _ = decode_js(nals, {"tensor": True})
    assert len(got) == len(dflt) == len(frames) and set(dims) == {(86, 52)}
    for k, (t, d) in enumerate(zip(got, dflt)):
        assert t.dtype == d.dtype == torch.float16 and tuple(t.shape) == tuple(d.shape) == (3, 52, 86)
        assert same(tensor_bytes(t), frame_expect(frames[k], w, h, win, "rgb", "float16", "imagenet")), k
        assert same(tensor_bytes(d), frame_expect(frames[k], w, h, win, "rgb", "float16", "unit")), k


@pytest.mark.gpu
def test_decoder_tensor_without_a_crop_window_is_the_whole_picture():
    import torch
    c = _golden.cases()["small_ip_8x6_2sl"]
    nals = split_annexb(_golden.stream(c))
    plain, pdims, flag = decode_js(nals, {})
    plain = [bytes(f) for f in plain]
    got, dims, _ = decode_js(nals, {"tensor": {"dtype": torch.uint8, "mode": "gray"}})
    rgb, rdims, _ = decode_js(nals, {"tensor": {"dtype": torch.uint8}})
    assert flag == 0 and len(plain) > 0 and len(got) == len(rgb) == len(plain) and dims == rdims == pdims
    w, h = pdims[0]
    for k, f in enumerate(plain):
        assert same(tensor_bytes(got[k]), T.samples(f, w, h, "gray").reshape(-1)), k
        assert same(tensor_bytes(rgb[k]), T.samples(f, w, h, "rgb").reshape(-1)), k


@pytest.mark.gpu
def test_switching_between_tensor_and_plain_output():
    """An instance drained as tensors stops queueing the host copy behind
    each launch; a caller that goes back to NextPicture still gets every
    picture (read on demand)."""
    import torch
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    full, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    got = []
    dec = Decoder({"tensor": {"dtype": torch.uint8}})
    as_tensor = dec._tensor

    def on_picture(buf, pw, ph, infos):
        got.append((buf if torch.is_tensor(buf) else bytes(buf), pw, ph))
        dec._tensor = as_tensor if len(got) in (1, 4) else None      # tensors: pictures 0, 1 and 4; plain: 2 and 3

    dec.onPictureDecoded = on_picture
    for nal in split_annexb(case_stream("crop_ltrb_6x4")):
        dec.decode(nal)
    dec.close()
    assert len(got) == len(full) == 5
    for k, (buf, pw, ph) in enumerate(got):
        if k in (0, 1, 4):
            assert (pw, ph) == (86, 52) and torch.is_tensor(buf), k
            assert same(tensor_bytes(buf), frame_expect(full[k], w, h, win, "rgb", "uint8", "unit")), k
        else:
            assert (pw, ph) == (w, h) and buf == full[k], k


@pytest.mark.gpu
def test_decoder_tensor_on_a_shared_engine():
    """Two instances of one picture size on one batched engine
    (h264mi_set_share): each exports its own lane's slots, under the engine's
    lock, and gets its own pictures."""
    import threading
    import torch
    L = _mi()
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    streams = [case_stream("crop_ltrb_6x4"), gen.generate(c["config"], c["seed"] + 1, **c["overrides"])]
    refs = [O.decode(s) for s in streams]
    results, errors = {}, []

    def run(k):
        try:
            results[k] = decode_js(split_annexb(streams[k]), {"tensor": {"dtype": torch.uint8}})
        except Exception as ex:          # surfaced by the main thread
            errors.append((k, ex))

    b0, p0 = C.c_ulonglong(), C.c_ulonglong()
    L.h264mi_share_stats(0, C.byref(b0), C.byref(p0))
    assert L.h264mi_set_share(2) == 0
    try:
        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=60)
        assert not any(t.is_alive() for t in th), "decoder thread hung"
    finally:
        L.h264mi_set_share(0)
    assert not errors, errors
    b1, p1 = C.c_ulonglong(), C.c_ulonglong()
    L.h264mi_share_stats(0, C.byref(b1), C.byref(p1))
    assert p1.value - p0.value == sum(len(r[0]) for r in refs)          # the shared engine reconstructed them
    for k in range(2):
        frames, _, w, h, _ = refs[k]
        got, dims, _ = results[k]
        assert len(got) == len(frames) and set(dims) == {(win[2], win[3])}
        for i, t in enumerate(got):
            assert same(tensor_bytes(t), frame_expect(frames[i], w, h, win, "rgb", "uint8", "unit")), (k, i)
