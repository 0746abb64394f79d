"""The colour sets of the RGB tensor exports: BT.601 / BT.709,
limited / full range, chosen by the caller (bits 8..11 of the descriptor's
mode) or resolved from the delivered picture's VUI
(H264MI_TENSOR_COLOUR_STREAM), through h264mi_tensor[_resize]_device_pitch,
Engine.to_tensor and the Decoder's ``tensor`` option; the generator's VUI
knobs; the host side on the CPU stand-in of the engine
(tests/colour_host_check.c, built with AddressSanitizer + UBSan).

The oracle (tests/_colour.py) derives the six integers of a set with
fractions.Fraction and converts in numpy integers; set 0 is pinned to
oracle.yuv2rgba.  Every comparison of tensors is exact equality of bytes."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import _colour as K
import _crop
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "colour.json")) as _f:
    GOLDEN = json.load(_f)
CASES = GOLDEN["cases"]
CROP = _crop.cases()["crop_ltrb_6x4"]
WIN = (6, 2, 86, 52)            # its SPS crop window, of 96 x 64
RGB, GRAY = 0, 1


def vui_stream(name):
    c = CASES[name]
    s = gen.generate(GOLDEN["config"], c["seed"], **dict(GOLDEN["base_overrides"], **c["overrides"]))
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


def plain_stream(name):
    c = CASES[name]
    ov = {k: v for k, v in c["overrides"].items() if not k.startswith("vui_")}
    return gen.generate(GOLDEN["config"], c["seed"], **dict(GOLDEN["base_overrides"], **ov))


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_tensor.py."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


def _mi():
    from broadway_amd import _lib
    return _lib.mi()


# ------------------------------------------------------------------ CPU ----
def test_table_is_the_documented_one():
    """The Fraction-derived integers against the table of include/h264mi.h and
    DESIGN 3.5f (ky, yoff, crv, cgu, cgv, cbu); k0 = 512 - ky * yoff, and set 0
    has no rounding term."""
    doc = {0: (1192, 16, 1634, 400, 832, 2066), 1: (1024, 0, 1436, 352, 731, 1815),
           2: (1192, 16, 1836, 218, 546, 2163), 3: (1024, 0, 1613, 192, 479, 1900)}
    for cid, (ky, yoff, crv, cgu, cgv, cbu) in doc.items():
        assert K.coeffs(cid) == (ky, (512 if cid else 0) - ky * yoff, crv, cgu, cgv, cbu), cid
    with open(os.path.join(ROOT, "include", "h264mi.h")) as f:
        text = " ".join(f.read().split())
    for row in ("1192 16 1634 400 832 2066", "1024 0 1436 352 731 1815", "1192 16 1836 218 546 2163",
                "1024 0 1613 192 479 1900"):
        assert row in text, row


def test_library_table_is_the_fraction_table():
    L = _mi()
    out = (C.c_int * 6)()
    for cid in range(4):
        assert L.h264mi_tensor_colour_coeffs(cid, C.byref(out)) == 0 and tuple(out) == K.coeffs(cid), cid
    for cid in (-1, 4, 15, 256):
        assert L.h264mi_tensor_colour_coeffs(cid, C.byref(out)) == -1, cid
    assert L.h264mi_tensor_colour_coeffs(0, None) == -1


def test_intermediates_fit_24_bits():
    for cid in range(4):
        ky, k0, crv, cgu, cgv, cbu = K.coeffs(cid)
        for y in (0, 255):
            a0 = ky * y + k0
            for u in (-128, 127):
                for v in (-128, 127):
                    for t in (a0, crv * v + k0, k0 - cgu * u, k0 - cgu * u - cgv * v, cbu * u + k0, a0 + crv * v,
                              a0 - cgu * u - cgv * v, a0 + cbu * u):
                        assert -(1 << 23) <= t < (1 << 23), (cid, y, u, v)


def test_set_0_is_the_reference_converter():
    """_colour.samples_colour with set 0 == _tensor.samples (oracle.yuv2rgba)
    on random pictures and on the extremes picture."""
    rng = np.random.default_rng(5)
    for cw, ch in ((2, 2), (38, 26), (96, 64)):
        p = rng.integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)
        assert np.array_equal(K.samples_colour(p, cw, ch, 0), T.samples(p, cw, ch, "rgb")), (cw, ch)
    p, w, h, _ = K.extremes_picture()
    assert np.array_equal(K.samples_colour(p, w, h, 0), T.samples(p, w, h, "rgb"))


@pytest.mark.parametrize("cid", [1, 2, 3])
def test_integer_sets_are_within_one_of_the_matrix_formula(cid):
    """All 2^24 (Y, U, V): the integer result differs from the float64 matrix
    formula, rounded to nearest and clamped, by at most 1.  Derived, not
    measured: the rounding of the coefficients moves the unrounded value by
    at most (0.5 / 1024) * (255 + 2 * 128) < 0.25, and the integer form rounds
    that to nearest (the + 512 before the shift); two values less than 0.25
    apart round to integers at most 1 apart."""
    ky, yoff, crv, cgu, cgv, cbu = (float(c) for c in K.rational(cid))
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    uf, vf = u - 128.0, v - 128.0
    worst = 0
    for y in range(256):
        a = ky * (y - yoff)
        want = [np.clip(np.rint(a + crv * vf), 0, 255), np.clip(np.rint(a - cgu * uf - cgv * vf), 0, 255),
                np.clip(np.rint(a + cbu * uf), 0, 255)]
        got = K.rgb_of(np.full_like(u, y), u, v, cid)
        worst = max(worst, max(int(np.abs(g - w.astype(np.int64)).max()) for g, w in zip(got, want)))
    assert worst <= 1, worst


def test_generator_knobs_zero_leave_the_stream_unchanged():
    base = dict(GOLDEN["base_overrides"])
    s = gen.generate(GOLDEN["config"], 61, vui_matrix=0, vui_full_range=0, **base)
    assert hashlib.sha256(s).hexdigest() == CROP["stream_sha256"]
    # a full-range flag has nowhere to go without a VUI
    assert gen.generate(GOLDEN["config"], 61, vui_matrix=0, vui_full_range=1, **base) == s
    for name, c in CASES.items():
        assert hashlib.sha256(plain_stream(name)).hexdigest() == c["plain_sha256"], name
    assert CASES["m1"]["plain_sha256"] == CROP["stream_sha256"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_vui_streams_decode_to_the_pictures_without_vui(name):
    c = CASES[name]
    s = vui_stream(name)
    assert len(s) == c["stream_bytes"] and s != plain_stream(name)
    frames, errs, w, h, _ = O.decode(s)
    plain = O.decode(plain_stream(name))[0]
    assert errs == 0 and (w, h) == (96, 64)
    assert [O.md5(f) for f in frames] == c["frames"] == [O.md5(f) for f in plain]
    if os.path.exists(_crop.REFDEC):
        assert [O.md5(f) for f in O.refdec_frames(s)] == c["frames"]


@pytest.mark.parametrize("kw", [dict(colour="bt2020"), dict(colour=2), dict(colour="stream"),
                                dict(colour="bt709", mode="gray"), dict(colour="reference", mode="gray"),
                                dict(colour="bt709", unspecified="bt709"), dict(unspecified="bt709")])
def test_tensor_desc_rejects(kw):
    from broadway_amd.engine import tensor_desc
    with pytest.raises(ValueError):
        tensor_desc((0, 0, 2, 2), **kw)
    with pytest.raises(ValueError):
        tensor_desc((0, 0, 2, 2), size=(2, 2), **kw)


def test_python_colour_arguments():
    from broadway_amd import _lib
    from broadway_amd.engine import Engine, tensor_desc
    for k, name in enumerate(K.NAMES):
        assert tensor_desc((0, 0, 2, 2), colour=name)[0].mode == K.mode(k)
        assert tensor_desc((0, 0, 2, 2), colour=name, size=(3, 3))[0].t.mode == K.mode(k)
    assert tensor_desc((0, 0, 2, 2))[0].mode == tensor_desc((0, 0, 2, 2), colour=None)[0].mode == RGB
    assert tensor_desc((0, 0, 2, 2), mode="gray")[0].mode == GRAY
    for name, u in K.UNSPEC.items():
        d = tensor_desc(None, colour="stream", unspecified=name, stream_ok=True)[0]
        assert d.mode == K.mode(K.STREAM, u)
    assert tensor_desc(None, colour="stream", stream_ok=True)[0].mode == K.mode(K.STREAM, 0)
    with pytest.raises(ValueError):
        tensor_desc(None, colour="stream", unspecified="bt2020", stream_ok=True)
    assert _lib.TENSOR_COLOURS == dict({n: k for k, n in enumerate(K.NAMES)}, stream=K.STREAM)
    # Engine.to_tensor checks before it touches the library (no engine exists here)
    for kw in (dict(colour="stream"), dict(colour="bt709", mode="gray"), dict(colour="nope")):
        with pytest.raises(ValueError):
            Engine.to_tensor(object.__new__(Engine), [0], [0], window=(0, 0, 2, 2), **kw)


def test_decoder_tensor_option_colour_keys():
    for opts in (dict(colour="bt709", mode="gray"), dict(colour="stream", mode="gray"), dict(colour="nope"),
                 dict(colour="stream", unspecified="nope"), dict(colour="bt709", unspecified="size"),
                 dict(colour="bt709", color="bt709"), dict(unspecific="size")):
        with pytest.raises(ValueError):
            Decoder({"tensor": opts})


def test_stream_resolution_table():
    """h264mi_tensor_colour_resolve over (no VUI or no description = 2,
    matrix 1, 2, 5, 6, 7 and the rest) x range x fallback x sizes on either
    side of 1280 x 576; explicit ids pass through; bad modes give -1."""
    L = _mi()
    sizes = [(86, 52), (1278, 576), (1280, 2), (2, 578), (1920, 1080)]
    for matrix in [1, 2, 5, 6, 7, 0, 3, 4, 8, 9, 255]:
        for full in (0, 1):
            for u in K.UNSPEC.values():
                for cw, ch in sizes:
                    got = L.h264mi_tensor_colour_resolve(K.mode(K.STREAM, u), matrix, full, cw, ch)
                    assert got == K.resolve(matrix, full, u, cw, ch), (matrix, full, u, cw, ch)
    assert [L.h264mi_tensor_colour_resolve(K.mode(K.STREAM, 2), 2, 0, cw, ch) for cw, ch in sizes] == [0, 0, 2, 2, 2]
    assert L.h264mi_tensor_colour_resolve(K.mode(K.STREAM, 0), 7, 1, 1920, 1080) == 1
    assert L.h264mi_tensor_colour_resolve(K.mode(K.STREAM, 1), 2, 1, 2, 2) == 3
    for cid in range(4):
        assert L.h264mi_tensor_colour_resolve(K.mode(cid), 1, 1, 1920, 1080) == cid
    assert L.h264mi_tensor_colour_resolve(GRAY, 1, 1, 1920, 1080) == 0
    for bad in BAD_MODES_DEC:
        assert L.h264mi_tensor_colour_resolve(bad, 1, 0, 64, 64) == -1, hex(bad)


# modes every entry point refuses; the engine-level calls refuse STREAM too
BAD_MODES_DEC = ([K.mode(c, 0, GRAY) for c in (1, 2, 3, K.STREAM)] + [K.mode(0, 1, GRAY)] +
                 [K.mode(c) for c in range(4, 15)] + [K.mode(K.STREAM, 3)] +
                 [K.mode(2) | 1 << b for b in (14, 15, 16, 30)] + [RGB | 1 << 14, 2, -1, K.mode(2, 0, 2)])
BAD_MODES_ENGINE = BAD_MODES_DEC + [K.mode(K.STREAM, u) for u in range(3)]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/colour_host_check.c with the product host path, the generator and
    the CPU stand-in of the engine, under AddressSanitizer + UBSan (shift
    excluded, as in oracle/Makefile); its output lines."""
    td = tmp_path_factory.mktemp("colour_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c"),
                                               os.path.join(HERE, "colour_host_check.c")]
    cxxsrc = [os.path.join(ROOT, "oracle", "null_device.cpp"), os.path.join(P, "host", "hipback.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=undefined"]
    common = ["-O1", "-g", "-fno-omit-frame-pointer"] + san
    objs = []
    procs = []
    for f in csrc:
        o = str(td / (os.path.basename(f) + ".o"))
        objs.append(o)
        procs.append(subprocess.Popen([os.environ.get("CC", "gcc")] + common +
                                      ["-std=gnu11", "-Wno-unused-parameter", "-c", f, "-o", o]))
    assert all(p.wait() == 0 for p in procs)
    exe = str(td / "colour_host_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([os.environ.get("CXX", "g++")] + common + ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include"] +
                   cxxsrc + objs + ["-o", exe, "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
        "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
    assert not bad and p.returncode == 0, (p.returncode, bad[:3], p.stderr[-2000:])
    return p.stdout.splitlines()


@pytest.mark.timeout(600)
def test_host_side_on_the_cpu_stand_in(host_check):
    """No sanitizer report (the fixture), and: H264SwDecGetInfo reports the VUI
    the generator wrote; every picture is exported with the set of its own
    SPS -- in the two-SPS stream also those delivered when the second SPS is
    active already --; a bad mode is refused without consuming a picture."""
    lines = host_check
    info = {tuple(int(v) for v in ln.split()[1:3]): tuple(int(v) for v in ln.split()[4:6])
            for ln in lines if ln.startswith("info ")}
    assert info == {(m, f): ((f if m else 0), (m if m > 0 else 2)) for m in (0, -1, 1, 2, 5, 6, 7) for f in (0, 1)}
    for name, c in CASES.items():
        m, f = c["overrides"]["vui_matrix"], c["overrides"]["vui_full_range"]
        assert info[(m, f)] == (c["videoRange"], c["matrixCoefficients"]), name
    cases = {}
    for ln in lines:
        if ln.startswith("case "):
            head, _, items = ln.partition(":")
            cases[head.split()[1]] = (int(head.split()[3]), [tuple(int(v, 16) for v in it.split("/")) for it in items.split()])
    want = {"m1": 2, "m1_full": 3, "m6_full": 1, "m7_full": 3, "novui_size": 0, "sig_full_size": 1, "explicit_bt709": 2}
    for name, cid in want.items():
        n, items = cases[name]
        assert n == 5 and [(a, b) for a, b, _ in items] == [(cid, K.mode(cid))] * 5, name
    assert [(a, b) for a, b, _ in cases["gray"][1]] == [(0, GRAY)] * 5
    n, items = cases["two_sps"]
    assert n == 10 and [(a, b) for a, b, _ in items] == [(2, K.mode(2))] * 5 + [(1, K.mode(1))] * 5
    active = [c for _, _, c in items]
    assert active[0] == 1 and 6 in active[:5] and set(active[5:]) == {6}      # BT.709 pictures under the later SPS
    ref = [ln.split() for ln in lines if ln.startswith("refusals ")]
    assert len(ref) == 1 and ref[0][1] == ref[0][3] and int(ref[0][1]) > 0 and ref[0][5] == "5", ref
    res = [ln.split() for ln in lines if ln.startswith("resolve ")]
    assert len(res) == 1 and int(res[0][1]) > 6000 and res[0][3] == "0"


# ------------------------------------------------------------------ GPU ----
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128), "extremes": (256, 162, 128)}
WINDOWS = [None, (2, 2, 2, 2), (6, 2, 38, 26), (0, 0, 46, 32), (44, 30, 4, 2), (6, 2, 32, 26)]     # test_tensor.py's
SENTINEL = 0xA5
FRONT = 64


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 pictures in the (width, cpitch) layout (read-only): random
    ones as in test_tensor.py, and the extremes picture."""
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        if name == "extremes":
            out[name] = [K.extremes_picture()[0]]
            continue
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def run_export(pics, order, w, h, cp, win, mode, dtype, consts="unit", size=None, in_pad=0, out_pad=0, skew=0):
    """h264mi_tensor_device_pitch (size = (oh, ow): the resized call) over
    pictures `order` of `pics` with descriptor mode `mode`; returns rc, the
    whole output buffer (FRONT + skew sentinel bytes, pictures out_stride
    apart, 64 sentinel bytes), the first picture's offset, out_stride and a
    picture's bytes."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    es = T.ELEM[dtype]
    planes = 1 if (mode & 255) == GRAY else 3
    oh, ow = size if size is not None else (win[3], win[2])
    nbytes = planes * oh * ow * es
    in_stride = pics[0].size + in_pad
    out_stride = nbytes + out_pad
    host = np.zeros(in_stride * len(pics), dtype=np.uint8)
    for k, p in enumerate(pics):
        host[k * in_stride:k * in_stride + p.size] = p
    d_in = torch.from_numpy(host).to("cuda")
    n = len(order)
    offs = (C.c_size_t * n)(*[k * in_stride for k in order])
    first = FRONT + skew
    d_out = torch.full((first + out_stride * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    t = _lib.TensorDesc()
    t.x, t.y, t.cw, t.ch = win
    t.mode, t.dtype = mode, T.DTYPES.index(dtype)
    t.scale[:], t.bias[:] = T.CONSTS[consts]
    st = torch.cuda.current_stream().cuda_stream
    if size is None:
        rc = L.h264mi_tensor_device_pitch(d_in.data_ptr(), offs, n, w, h, cp, C.byref(t), d_out.data_ptr() + first,
                                          out_stride, st)
    else:
        r = _lib.TensorResizeDesc()
        r.t, r.ow, r.oh, r.filter = t, ow, oh, 0
        rc = L.h264mi_tensor_resize_device_pitch(d_in.data_ptr(), offs, n, w, h, cp, C.byref(r),
                                                 d_out.data_ptr() + first, out_stride, st)
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
    return ["unit"] if dtype == "uint8" else ["imagenet", "unit"]       # uint8 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("cid", [1, 2, 3])
def test_kernel_vs_oracle(pictures, cid, dtype):
    """Both store paths and the 2-column tail (WINDOWS) on the three pictures;
    nothing else is written."""
    for pic, (w, h, cp) in PICS.items():
        p = pictures[pic][0]
        for win in WINDOWS:
            win = win or (0, 0, w, h)
            for consts in consts_of(dtype):
                rc, out, first, _, nbytes = run_export([p], [0], w, h, cp, win, K.mode(cid), dtype, consts)
                assert rc == 0, (pic, win, consts)
                assert same(out[first:first + nbytes], K.expect(p, w, h, cp, win, cid, dtype, consts)), (pic, win, consts)
                assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (pic, win, consts)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,cid", [("float16", 3), ("uint8", 2)])
def test_kernel_batched_padded_strides_write_nothing_else(pictures, dtype, cid):
    """Picture list [2, 0, 2] of three pictures 37 bytes apart; out_stride
    padded by 5 elements (the general path) and by 48 bytes (16-byte rows keep
    the 16-byte stores)."""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    es = T.ELEM[dtype]
    order = [2, 0, 2]
    for win in [(6, 2, 38, 26), (6, 2, 32, 26)]:
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_export(pics, order, w, h, cp, win, K.mode(cid), dtype, "imagenet",
                                                        in_pad=37, out_pad=out_pad, skew=skew)
            assert rc == 0 and (out[:first] == SENTINEL).all(), (win, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                assert same(out[o:o + nbytes], K.expect(pics[i], w, h, cp, win, cid, dtype, "imagenet")), (win, out_pad, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (win, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (win, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_kernel_set_0_given_explicitly_is_the_default_export(pictures, dtype):
    """mode = RGB | 0 << 8 is mode = RGB: the reference's pixels (_tensor)."""
    assert K.mode(0) == RGB
    for pic in ("48x32_pitch128", "extremes"):
        w, h, cp = PICS[pic]
        p = pictures[pic][0]
        for win in ((6, 2, 38, 26), (0, 0, w, h)):
            rc, out, first, _, nbytes = run_export([p], [0], w, h, cp, win, K.mode(0), dtype, "imagenet")
            assert rc == 0 and same(out[first:first + nbytes], T.expect(p, w, h, cp, win, "rgb", dtype, "imagenet")), win
            assert same(out[first:first + nbytes], K.expect(p, w, h, cp, win, 0, dtype, "imagenet")), win


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("cid", [2, 3])
def test_resized_kernel_vs_oracle(pictures, cid, dtype):
    """convert(resize(samples_colour(window))); the identity size is the
    unresized colour tensor."""
    ex, rnd = pictures["extremes"][0], pictures["48x32_pitch128"][0]
    for pic, p, win, size in (("extremes", ex, (0, 0, 256, 162), (20, 24)), ("extremes", ex, (0, 0, 256, 162), (162, 256)),
                              ("48x32_pitch128", rnd, (0, 0, 46, 32), (7, 9))):
        w, h, cp = PICS[pic]
        rc, out, first, _, nbytes = run_export([p], [0], w, h, cp, win, K.mode(cid), dtype, "imagenet", size=size)
        assert rc == 0, (pic, size)
        assert same(out[first:first + nbytes], K.expect(p, w, h, cp, win, cid, dtype, "imagenet", size=size)), (pic, size)
        assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (pic, size)
        if size == (win[3], win[2]):
            assert same(out[first:first + nbytes], K.expect(p, w, h, cp, win, cid, dtype, "imagenet")), (pic, size)


@pytest.mark.gpu
def test_engine_level_calls_refuse_bad_modes_and_stream(pictures):
    """STREAM (an engine knows no stream), colour bits with GRAY, ids 4..14 and
    any bit from 14 up: -1 and nothing launched, at all four calls."""
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import Engine
    L = _mi()
    w, h, cp = PICS["48x32_pitch128"]
    p = pictures["48x32_pitch128"][:1]
    win = (2, 2, 4, 4)
    rc, out, first, _, nbytes = run_export(p, [0], w, h, cp, win, K.mode(2), "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # one step away from the modes below
    eng = Engine(3, 2, 1, 2)
    d_out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    one = (C.c_int * 1)(0)
    st = torch.cuda.current_stream().cuda_stream
    for mode in BAD_MODES_ENGINE:
        for size in (None, (3, 5)):
            rc, out, *_ = run_export(p, [0], w, h, cp, win, mode, "float16", size=size)
            assert rc == -1 and (out == SENTINEL).all(), (hex(mode), size)
        t = _lib.TensorDesc()
        t.x, t.y, t.cw, t.ch, t.mode, t.dtype = 2, 2, 4, 4, mode, 0
        r = _lib.TensorResizeDesc()
        r.t, r.ow, r.oh, r.filter = t, 5, 3, 0
        assert L.h264mi_engine_export_tensor(eng._h, 1, one, one, C.byref(t), d_out.data_ptr(), 0, st) == -1, hex(mode)
        assert L.h264mi_engine_export_tensor_resized(eng._h, 1, one, one, C.byref(r), d_out.data_ptr(), 0, st) == -1
    # (the same descriptors with a good mode pass: the refusals above are the mode's)
    t.mode = r.t.mode = K.mode(3)
    assert L.h264mi_engine_export_tensor(eng._h, 1, one, one, C.byref(t), d_out.data_ptr(), 0, st) == 0
    assert L.h264mi_engine_export_tensor_resized(eng._h, 1, one, one, C.byref(r), d_out.data_ptr() + 2048, 0, st) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[48:2048] == SENTINEL).all() and (got[2048 + 45:] == SENTINEL).all()


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


def swdec_tensors(stream, mode, dtype="uint8", size=None, bad_modes=()):
    """The reference testbench's loop (the whole buffer fed, NextPicture
    drained after every picture, flushed at the end) over the H264SwDec API,
    every picture taken as a tensor of the SPS crop window with `mode`.
    Returns per picture (tensor, H264SwDecLastTensorColour, the active SPS's
    matrixCoefficients at the call).  bad_modes: each is tried, on both
    calls, before every fetch and must give PARAM_ERR."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecLastTensorColour(inst) == -1
    buf = (C.c_uint8 * len(stream)).from_buffer_copy(stream)
    inp, outp, pic, info = _lib.H264SwDecInput(), _lib.H264SwDecOutput(), _lib.H264SwDecPicture(), _lib.H264SwDecInfo()
    inp.pStream, inp.dataLen = C.cast(buf, C.POINTER(C.c_uint8)), len(stream)
    st = torch.cuda.current_stream().cuda_stream
    got = []

    def desc(m):
        r = _lib.TensorResizeDesc()
        r.t.mode, r.t.dtype = m, T.DTYPES.index(dtype)
        r.t.scale[:], r.t.bias[:] = T.CONSTS["unit"]
        r.oh, r.ow = size if size is not None else (1, 1)
        return r

    def fetch(flush):
        while True:
            oh, ow = size if size is not None else (WIN[3], WIN[2])
            out = torch.full((3, oh, ow), 77, dtype=T.torch_dtype(dtype), device="cuda")
            for m in bad_modes:
                r = desc(m)
                assert L.H264SwDecNextPictureTensor(inst, C.byref(pic), 0, C.byref(r.t), out.data_ptr(), st) == _lib.H264SWDEC_PARAM_ERR
                assert L.H264SwDecNextPictureTensorResized(inst, C.byref(pic), 0, C.byref(r), out.data_ptr(), st) == _lib.H264SWDEC_PARAM_ERR
            r = desc(mode)
            ret = (L.H264SwDecNextPictureTensor(inst, C.byref(pic), flush, C.byref(r.t), out.data_ptr(), st) if size is None
                   else L.H264SwDecNextPictureTensorResized(inst, C.byref(pic), flush, C.byref(r), out.data_ptr(), st))
            if ret != _lib.H264SWDEC_PIC_RDY:
                assert ret == _lib.H264SWDEC_OK, ret
                return
            flush = 0
            assert L.H264SwDecGetInfo(inst, C.byref(info)) == _lib.H264SWDEC_OK
            got.append((out, L.H264SwDecLastTensorColour(inst), int(info.matrixCoefficients)))

    pic_id = 0
    try:
        while inp.dataLen > 0:
            inp.picId = pic_id
            ret = L.H264SwDecDecode(inst, C.byref(inp), C.byref(outp))
            used = C.cast(outp.pStrmCurrPos, C.c_void_p).value - C.cast(inp.pStream, C.c_void_p).value
            assert ret >= 0 and (used > 0 or ret in (_lib.H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY,
                                                     _lib.H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY)), ret
            inp.dataLen -= used
            inp.pStream = outp.pStrmCurrPos
            if ret in (_lib.H264SWDEC_PIC_RDY, _lib.H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY):
                pic_id += 1
                fetch(0)
        fetch(1)
        torch.cuda.synchronize()
    finally:
        L.H264SwDecRelease(inst)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("size", [None, (13, 22)])
def test_swdec_calls_refuse_bad_modes_without_consuming_a_picture(size):
    """PARAM_ERR for every bad mode, on both calls, before every fetch; the
    next valid call still delivers the next picture, the first included."""
    s = vui_stream("m1")
    frames, _, w, h, _ = O.decode(s)
    got = swdec_tensors(s, K.mode(K.STREAM, 0), "uint8", size, bad_modes=BAD_MODES_DEC)
    assert len(got) == len(frames) == 5
    for k, (t, cid, _) in enumerate(got):
        assert cid == 2 and same(tensor_bytes(t), K.frame_expect(frames[k], w, h, WIN, 2, "uint8", size=size)), k


@pytest.mark.gpu
def test_two_sps_in_one_stream_each_picture_uses_its_own():
    """(matrix 1, display reordering) then (matrix 6, full range), both SPS id
    0, of one geometry: the first stream's last pictures leave the DPB when
    the second SPS is active, and are BT.709 limited all the same."""
    a, b = vui_stream("m1_poc0"), vui_stream("m6_full_s62")
    frames, errs, w, h, _ = O.decode(a + b)
    assert errs == 0 and [O.md5(f) for f in frames] == CASES["m1_poc0"]["frames"] + CASES["m6_full_s62"]["frames"]
    got = swdec_tensors(a + b, K.mode(K.STREAM, 0), "float16")
    assert [cid for _, cid, _ in got] == [2] * 5 + [1] * 5
    active = [m for _, _, m in got]
    assert active[0] == 1 and 6 in active[:5] and set(active[5:]) == {6}
    for k, (t, cid, _) in enumerate(got):
        assert same(tensor_bytes(t), K.frame_expect(frames[k], w, h, WIN, cid, "float16")), k


@pytest.mark.gpu
def test_engine_to_tensor_colour_vs_reference_decoder():
    """Engine.to_tensor(colour=...) behind every launch on a side stream, as
    test_tensor.py's test_engine_to_tensor_vs_reference_decoder."""
    import torch
    from broadway_amd.engine import Capture, Engine
    s = plain_stream("m1")
    frames, errs, w, h, _ = O.decode(s)
    cap = Capture(s)
    assert errs == 0 and len(frames) == cap.npics
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    kinds = [("bt709", torch.float16, "imagenet", None), ("bt709", torch.uint8, "unit", None),
             ("bt709-full", torch.float32, "unit", None), ("bt601-full", torch.bfloat16, "imagenet", (26, 43)),
             ("reference", torch.uint8, "unit", None)]
    got = []
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        name, dtype, consts, size = kinds[k % len(kinds)]
        scale, bias = T.CONSTS[consts]
        got.append(eng.to_tensor([0], [pic.cur_slot], window=WIN, dtype=dtype, scale=scale, bias=bias, stream=side,
                                 size=size, colour=name))
    torch.cuda.synchronize()
    assert eng.errors() == 0
    for k, t in enumerate(got):
        name, dtype, consts, size = kinds[k % len(kinds)]
        assert tuple(t.shape) == (1, 3) + (size or (WIN[3], WIN[2])) and t.dtype == dtype
        want = K.frame_expect(frames[k], w, h, WIN, K.NAMES.index(name), str(dtype).split(".")[1], consts, size=size)
        assert same(tensor_bytes(t), want), k


def decode_js(nals, opts):
    got = []
    dec = Decoder(opts)
    assert dec.tensor_colour is None
    dec.onPictureDecoded = lambda buf, w, h, infos: got.append((buf, w, h, dec.tensor_colour))
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,unspecified,cid", [("m1", "bt709", 2), ("m1_full", "bt709", 3), ("m6_full", "bt709", 1),
                                                   ("m7_full", "bt709", 3), (None, "size", 0), ("m7_full", None, 1)])
def test_decoder_colour_stream(name, unspecified, cid):
    """The Decoder's tensor option with colour "stream": the bytes of the
    expected set, and tensor_colour names it; no VUI with "size" at this
    picture size is the default export."""
    import torch
    s = vui_stream(name) if name else plain_stream("m1")
    frames, _, w, h, _ = O.decode(s)
    opts = {"dtype": torch.float16, "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD, "colour": "stream"}
    if unspecified:
        opts["unspecified"] = unspecified
    got = decode_js(split_annexb(s), {"tensor": opts})
    assert len(got) == len(frames) == 5
    for k, (t, pw, ph, colour) in enumerate(got):
        assert (pw, ph) == (86, 52) and tuple(t.shape) == (3, 52, 86) and colour == K.NAMES[cid], k
        assert same(tensor_bytes(t), K.frame_expect(frames[k], w, h, WIN, cid, "float16", "imagenet")), k
    if name is None:
        del opts["colour"], opts["unspecified"]
        dflt = decode_js(split_annexb(s), {"tensor": opts})
        assert all(same(tensor_bytes(a[0]), tensor_bytes(b[0])) for a, b in zip(got, dflt)) and len(dflt) == 5
        assert {d[3] for d in dflt} == {"reference"}


@pytest.mark.gpu
def test_decoder_colour_stream_with_size_and_explicit_colour():
    import torch
    s = vui_stream("m1_full")
    frames, _, w, h, _ = O.decode(s)
    got = decode_js(split_annexb(s), {"tensor": {"dtype": torch.uint8, "colour": "stream", "size": (26, 43)}})
    exp = decode_js(split_annexb(s), {"tensor": {"dtype": torch.uint8, "colour": "bt601-full"}})
    assert len(got) == len(exp) == len(frames)
    for k in range(len(frames)):
        t, pw, ph, colour = got[k]
        assert (pw, ph) == (43, 26) and colour == "bt709-full"
        assert same(tensor_bytes(t), K.frame_expect(frames[k], w, h, WIN, 3, "uint8", size=(26, 43))), k
        assert exp[k][3] == "bt601-full" and same(tensor_bytes(exp[k][0]), K.frame_expect(frames[k], w, h, WIN, 1, "uint8")), k
