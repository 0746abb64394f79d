"""The decoded residual as device tensors (residual.hip): the record batches and
coefficient pools of decoded pictures as planar Y / UV / YUV tensors --
h264mi_residual_device, coefficient retention and h264mi_engine_export_residual
(Engine.keep_coefs / to_residual), and H264SwDecKeepResidual /
H264SwDecLastPictureResidual (Decoder's ``residual`` option).

The oracle (tests/_residual.py) restates the field definition of
include/h264mi.h in numpy over the raw record and coefficient bytes, and is
itself pinned to the reference's transform functions.  Every comparison is
exact equality of bytes."""
import ctypes as C
import hashlib
import os
from fractions import Fraction

import numpy as np
import pytest

import _crop
import _residual as R
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSD_SO = os.path.join(ROOT, "oracle", "_ref", "libh264bsdref.so")
CAP = 32                    # pictures per kernel launch (RESID_MAX_PICS)
CASE = _crop.cases()["crop_ltrb_6x4"]       # config 2, 6x4 MBs, 5 frames, gop 3, 2 slices, crop (6, 2) 86x52
CROP = (6, 2, 86, 52)


def case_stream():
    s = gen.generate(CASE["config"], CASE["seed"], **CASE["overrides"])
    assert hashlib.sha256(s).hexdigest() == CASE["stream_sha256"], "generator drift"
    return s


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_crop.py: the decoder instances here pool engines."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


def frozen(f):
    for p in f:
        p.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def captured():
    """(Capture, per picture the oracle's three planes) of the stream"""
    from broadway_amd.engine import Capture
    cap = Capture(case_stream())
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs) == (6, 4)
    fields = [frozen(R.field(cap.records_bytes(i), cap.coef_bytes(i), cap.w_mbs, cap.h_mbs)) for i in range(cap.npics)]
    return cap, fields


# ------------------------------------------------------------------ CPU ----
@pytest.fixture(scope="module")
def bsd():
    if not os.path.exists(BSD_SO):
        pytest.skip("oracle/_ref/libh264bsdref.so not built (needs the reference's sources at build time)")
    lib = C.CDLL(BSD_SO, mode=os.RTLD_LOCAL)
    i32p = C.POINTER(C.c_int32)
    lib.h264bsdProcessBlock.argtypes = [i32p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.h264bsdProcessBlock.restype = C.c_uint32
    lib.h264bsdProcessLumaDc.argtypes = [i32p, C.c_uint32]
    lib.h264bsdProcessLumaDc.restype = None
    lib.h264bsdProcessChromaDc.argtypes = [i32p, C.c_uint32]
    lib.h264bsdProcessChromaDc.restype = None
    return lib


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def ref_block(bsd, levels, qp, dc=None):
    """h264bsdProcessBlock on 16 levels in scan order (dc: position 0 comes
    from a DC transform): (4, 4) samples, or None on HANTRO_NOK"""
    data = _i32(levels)
    if dc is not None:
        data[0] = int(dc)
    cmap = sum(1 << s for s in range(16) if data[s])
    if bsd.h264bsdProcessBlock(data, qp, int(dc is not None), cmap) != 0:
        return None
    return np.array(list(data), dtype=np.int64).reshape(4, 4)


def draw_dc(rng, qp, npos):
    """16 DC levels, up to three of the first npos non-zero, small enough at
    this qp that most blocks stay inside [-512, 511]"""
    top = max(1, 32 >> max(qp // 6 - 3, 0))
    lv = np.zeros(16, dtype=np.int64)
    for s in rng.choice(npos, int(rng.integers(1, 4)), replace=False):
        lv[s] = int(rng.integers(-top, top + 1))
    return lv


def draw_levels(rng, qp, shape):
    """16 levels of the reference's shortcut `shape`, bounded likewise"""
    top = max(1, 160 >> (qp // 6))
    lv = np.zeros(16, dtype=np.int64)

    def nz():
        v = int(rng.integers(1, top + 1))
        return v if rng.random() < 0.5 else -v

    lv[0] = nz() if rng.random() < 0.8 else 0
    if shape == "row0":                                 # rows 1..3 zero: scan positions 1, 5, 6 only
        for s in rng.choice([1, 5, 6], int(rng.integers(1, 4)), replace=False):
            lv[s] = nz()
    elif shape == "full":
        for s in rng.choice(np.arange(1, 16), int(rng.integers(1, 5)), replace=False):
            lv[s] = nz()
        if not lv[[2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15]].any():
            lv[int(rng.choice([2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15]))] = nz()
    return lv


def test_oracle_blocks_match_the_reference(bsd):
    """Plain luma blocks, I16 luma blocks with and without a DC term and
    chroma blocks of both planes, at every qp, in each of the reference's three
    shortcuts (DC only; rows 1..3 zero; full), against h264bsdProcessLumaDc /
    h264bsdProcessChromaDc / h264bsdProcessBlock.  A block the reference
    rejects (HANTRO_NOK: it returns early and leaves the block half processed)
    is not compared; at least 90 % of the drawn blocks are."""
    rng = np.random.default_rng(7)
    drawn = compared = 0
    per = {}
    for qp in range(52):
        for shape in ("dc", "row0", "full"):
            for kind in ("luma", "i16", "i16_nodc", "cb", "cr"):
                for _ in range(2):
                    lv = draw_levels(rng, qp, shape)
                    dcl = draw_dc(rng, qp, 16 if kind == "i16" else 8)
                    if kind == "luma":
                        want, got = ref_block(bsd, lv, qp), R.inverse4x4(R.dequant(lv, qp, False))
                    else:
                        if kind == "i16":
                            data = _i32(dcl)
                            bsd.h264bsdProcessLumaDc(data, qp)
                            k = int(rng.integers(0, 16))
                            rdc, odc = data[k], R.luma_dc(dcl, qp)[k >> 2, k & 3]
                        elif kind == "i16_nodc":
                            rdc = odc = 0
                        else:
                            data = _i32(dcl[:8])
                            bsd.h264bsdProcessChromaDc(data, qp)
                            k = int(rng.integers(0, 4))
                            p = 0 if kind == "cb" else 1
                            rdc, odc = data[4 * p + k], R.chroma_dc(dcl[4 * p:4 * p + 4], qp)[k]
                        assert rdc == odc, (qp, shape, kind)
                        want = ref_block(bsd, lv, qp, dc=rdc)
                        d = R.dequant(lv, qp, True)
                        d[0] = odc
                        got = R.inverse4x4(d)
                    drawn += 1
                    if want is None:
                        continue
                    compared += 1
                    per[(shape, kind)] = per.get((shape, kind), 0) + 1
                    assert np.array_equal(got, want), (qp, shape, kind, lv.tolist())
    assert compared >= 0.9 * drawn, (compared, drawn)
    assert len(per) == 15 and min(per.values()) >= 52, per      # every shortcut of every kind, at most qps


def one_mb(mb_type, qp, qpc, cbits, blocks):
    r = np.zeros(1, dtype=R.MBREC)
    r["type"], r["qp"], r["qpc"], r["cbits"], r["coef"] = mb_type, qp, qpc, cbits, 0
    return r.tobytes(), np.asarray(blocks, dtype="<i2").reshape(-1, 16).tobytes()


def test_oracle_macroblocks_match_the_reference(bsd):
    """Whole MBs -- I16 with and without luma DC, inter and I4x4, each with
    both chroma planes -- composed from the reference's functions the way its
    ProcessResidual does (DC transforms first, then every block that has a level
    or a DC term) against the oracle's field of a one-MB picture."""
    rng = np.random.default_rng(11)
    drawn = compared = 0
    for qp in range(52):
        for mb_type in (R.MBT_I16, R.MBT_I16, R.MBT_INTER, R.MBT_I4x4):
            qpc = int(rng.integers(0, 52))
            cbits = int(rng.integers(0, 1 << 27))
            if mb_type != R.MBT_I16 or rng.random() < 0.3:
                cbits &= ~(1 << 24)
            blocks, b2i = [], {}
            for b in range(27):
                if (cbits >> b) & 1:
                    b2i[b] = len(blocks)
                    q = qp if b < 16 or b == 24 else qpc
                    lv = draw_levels(rng, q, ("dc", "row0", "full")[int(rng.integers(0, 3))]) if b < 24 else \
                        draw_dc(rng, q, 16 if b == 24 else 4)
                    blocks.append(lv)
            if not blocks:
                continue
            rec, pool = one_mb(mb_type, qp, qpc, cbits, blocks)
            got = R.field(rec, pool, 1, 1)
            drawn += 1
            i16 = mb_type == R.MBT_I16
            ldc = [0] * 16
            if i16 and 24 in b2i:
                data = _i32(blocks[b2i[24]])
                bsd.h264bsdProcessLumaDc(data, qp)
                ldc = list(data)
            cdc = [0] * 8
            for p in range(2):
                if 25 + p in b2i:
                    cdc[4 * p:4 * p + 4] = [int(v) for v in blocks[b2i[25 + p]][:4]]
            data = _i32(cdc)
            bsd.h264bsdProcessChromaDc(data, qpc)
            cdc = list(data)
            want = R.zero_field(1, 1)
            ok = True
            for b in range(24):
                lv = blocks[b2i[b]] if b in b2i else np.zeros(16, dtype=np.int64)
                if b < 16:
                    dc = ldc[R.BLK_Y[b] * 4 + R.BLK_X[b]] if i16 else None
                    plane, x, y, q = want[0], R.BLK_X[b], R.BLK_Y[b], qp
                else:
                    dc = cdc[b - 16]
                    plane, x, y, q = want[1 + ((b - 16) >> 2)], b & 1, (b >> 1) & 1, qpc
                if b not in b2i and not dc:
                    continue                            # (the reference does not process it: zeros)
                o = ref_block(bsd, lv, q, dc=dc)
                if o is None:
                    ok = False
                    break
                plane[4 * y:4 * y + 4, 4 * x:4 * x + 4] = o
            if not ok:
                continue
            compared += 1
            for g, w_ in zip(got, want):
                assert np.array_equal(g, w_), (qp, mb_type, hex(cbits))
    assert compared >= 0.9 * drawn, (compared, drawn)


def test_exactness_premise():
    """For every constant set of these tests and every int16 v, float64(v) *
    float64(scale) + float64(bias) is exact, so the oracle's one rounding to
    fp32 is the rounding of a fused multiply-add (as in tests/test_mbinfo.py)."""
    pairs = {(s, b) for scale, bias in R.CONSTS.values() for s, b in zip(scale, bias)}
    v = np.arange(-32768, 32768, dtype=np.int64)
    for s, b in sorted(pairs):
        assert float(np.float32(s)) == s and float(np.float32(b)) == b          # fp32-representable
        got = (v.astype(np.float64) * np.float64(s) + np.float64(b)).tolist()
        fs, fb = Fraction(s), Fraction(b)
        q = max(fs.denominator, fb.denominator)
        assert q & (q - 1) == 0 and (fs * q).denominator == (fb * q).denominator == 1
        ns, nb = int(fs * q), int(fb * q)
        for k, vk in enumerate(v.tolist()):
            assert got[k] * q == vk * ns + nb, (s, b, vk)


SIZES = {"1x1": (1, 1), "3x2": (3, 2), "5x3": (5, 3), "9x2": (9, 2)}    # MBs; 9x2: two workgroups a row and one MB more


def make_synthetic():
    rng = np.random.default_rng(31)
    out = {}
    for name, (w, h) in SIZES.items():
        batches = [R.synthetic_batch(rng, w, h) for _ in range(3)]
        out[name] = (batches, [frozen(R.field(r, c, w, h)) for r, c in batches])
    return out


@pytest.fixture(scope="module")
def synthetic():
    """size -> (3 (record batch, pool) pairs, their oracle fields) (read-only)"""
    R.peak[0] = 0
    out = make_synthetic()
    peak = R.peak[0]
    y = np.concatenate([f[0].reshape(-1) for fs in out.values() for f in fs[1]])
    c = np.concatenate([p.reshape(-1) for fs in out.values() for f in fs[1] for p in f[1:]])
    for v in (y, c):
        assert v.max() == 32767 and v.min() == -32768                       # the clamp, both ways
        assert ((np.abs(v) > 512) & (np.abs(v) < 32767)).any() and (v == 0).any() and ((v != 0) & (np.abs(v) < 512)).any()
    out["peak"] = peak
    return out


def test_no_intermediate_leaves_int32(synthetic):
    """Every level of the synthetic sets is within +-2047, and no int64
    intermediate of the oracle over them leaves int32: the kernel's 32-bit
    arithmetic computes the same integers."""
    for name in SIZES:
        for r, c in synthetic[name][0]:
            rec = np.frombuffer(r, dtype=R.MBREC)
            pool = np.frombuffer(c, dtype="<i2").reshape(-1, 16)
            for m in rec:
                if int(m["type"]) in (R.MBT_INTER, R.MBT_I4x4, R.MBT_I16):
                    k = bin(int(m["cbits"]) & 0x7FFFFFF).count("1")
                    assert np.abs(pool[int(m["coef"]):int(m["coef"]) + k].astype(np.int64)).max(initial=0) <= 2047
    assert 0 < synthetic["peak"] < 2 ** 31, synthetic["peak"]


def test_library_exports_the_residual_entry_points():
    from broadway_amd import _lib
    L = _lib.mi()           # (first: it imports torch ahead of the library, so the process holds one HIP runtime)
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    for name, nargs in (("h264mi_residual_device", 12), ("h264mi_engine_keep_coefs", 2),
                        ("h264mi_engine_export_residual", 8), ("H264SwDecKeepResidual", 2),
                        ("H264SwDecLastPictureResidual", 4)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int x, y, cw, ch, planes, dtype; float scale[3], bias[3]; }
    D = _lib.ResidualDesc
    assert C.sizeof(D) == 6 * 4 + 2 * 3 * 4 == C.sizeof(_lib.TensorDesc)
    assert [getattr(D, n).offset for n in ("x", "y", "cw", "ch", "planes", "dtype")] == [0, 4, 8, 12, 16, 20]
    assert (D.scale.offset, D.bias.offset) == (24, 36)
    assert _lib.RESID_PLANES == R.PLANES and _lib.TENSOR_I16 == 4


def test_residual_desc_arguments():
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import residual_desc
    d, n, dt = residual_desc("yuv", (1, 2, 3, 4), torch.float16, scale=0.25, bias=(0.0, 1.0, 2.0))
    assert (n, dt) == (3, torch.float16)
    assert (d.x, d.y, d.cw, d.ch, d.planes, d.dtype) == (1, 2, 3, 4, 2, _lib.TENSOR_F16)
    assert list(d.scale) == [0.25] * 3 and list(d.bias) == [0.0, 1.0, 2.0]
    d, n, dt = residual_desc()
    assert (n, dt, d.cw, d.ch, d.planes, d.dtype) == (1, torch.int16, 0, 0, 0, _lib.TENSOR_I16) and d.scale[0] == 1.0
    assert residual_desc("uv", (2, 4, 6, 8))[1] == 2
    for kw in (dict(planes="Y"), dict(planes="rgb"), dict(planes=0), dict(dtype=torch.uint8), dict(dtype=torch.int32),
               dict(planes="uv", scale=(1.0,)), dict(planes="y", bias=(1.0, 2.0)), dict(planes="yuv", scale=(1.0, 2.0)),
               dict(window=(0, 0, 4)), dict(window=(0, 0, 0, 4)), dict(window=(-1, 0, 4, 4)),
               dict(planes="uv", window=(1, 0, 4, 4)), dict(planes="uv", window=(0, 0, 4, 3))):
        with pytest.raises(ValueError):
            residual_desc(**kw)


def test_decoder_option_validation():
    with pytest.raises(ValueError):
        Decoder({"residual": {"window": (0, 0, 16, 16)}})       # the window is the crop window
    with pytest.raises(ValueError):
        Decoder({"residual": {"plane": "y"}})
    with pytest.raises(ValueError):
        Decoder({"residual": {"planes": "rgb"}})
    with pytest.raises(ValueError):
        Decoder({"residual": {"dtype": np.int16}})
    with pytest.raises(ValueError):
        Decoder({"residual": {"planes": "uv", "scale": (1.0, 2.0, 3.0)}})
    with pytest.raises(ValueError):                             # checked whatever the output mode
        Decoder({"residual": {"planes": "nope"}, "rgb": True, "crop": True})
    with pytest.raises(ValueError):
        Decoder({"residual": {"planes": "nope"}, "mbinfo": True, "tensor": True})


def test_the_stream_exercises_the_field(captured):
    """What the engine and decoder tests below compare is not trivially zero."""
    cap, fields = captured
    assert any((f[0] != 0).any() for f in fields)                           # luma residual
    assert any((f[1] != 0).any() for f in fields) and any((f[2] != 0).any() for f in fields)    # chroma, both planes
    i16_dc = skip = beside = False
    for i in range(cap.npics):
        r = np.frombuffer(cap.records_bytes(i), dtype=R.MBREC)
        i16_dc |= bool(((r["type"] == R.MBT_I16) & ((r["cbits"] >> 24) & 1 == 1)).any())
        skip |= bool((r["type"] == R.MBT_SKIP).any())
        y = fields[i][0].reshape(cap.h_mbs, 16, cap.w_mbs, 16)
        zero = ~(y != 0).any(axis=(1, 3))                                   # (h_mbs, w_mbs): the MB's luma is all zero
        for p in (1, 2):
            zero &= ~(fields[i][p].reshape(cap.h_mbs, 8, cap.w_mbs, 8) != 0).any(axis=(1, 3))
        beside |= bool((zero[:, 1:] & ~zero[:, :-1]).any() or (zero[:, :-1] & ~zero[:, 1:]).any())
    assert i16_dc and skip and beside
    slots = [p.cur_slot for p in cap.pictures]
    assert len(set(slots)) < cap.npics and len(set(slots)) < cap.nslots    # a slot is reused, one never decoded into


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


SENTINEL = 0xA5
FRONT = 64


def windows(w, h, planes):
    """The whole picture, one sample (one 2x2 for "uv"), the last column, the
    last row, one starting and ending off MB and 4x4 boundaries (of the plane),
    one whose row bytes are a multiple of 16 for every element type and one for
    none; wider than two workgroups: 16-byte rows from inside an MB over three
    workgroups."""
    W, H = 16 * w, 16 * h
    if planes == "uv":
        out = [(0, 0, W, H), (4, 2, 2, 2), (W - 2, 0, 2, H), (0, H - 2, W, 2), (6, 2, W - 12, H - 8),
               (0, 2, 16, H - 4), (2, 0, 14, H)]
        if W > 128:
            out += [(6, 2, 128 + 8, H - 4)]             # 68 chroma columns: 136 / 272 bytes
    else:
        out = [(0, 0, W, H), (5, 3, 1, 1), (W - 1, 0, 1, H), (0, H - 1, W, 1), (5, 3, W - 11, H - 6),
               (3, 1, 8, H - 2), (2, 0, 7, H)]
        if W > 128:
            out += [(3, 1, 136, H - 2)]
    return out


def make_desc(win, planes, dtype, consts="unit"):
    from broadway_amd import _lib
    d = _lib.ResidualDesc()
    d.x, d.y, d.cw, d.ch = win
    d.planes = R.PLANES.get(planes, planes)
    d.dtype = R.DTYPE_ID.get(dtype, dtype)
    scale, bias = R.CONSTS[consts]
    d.scale[:] = scale
    d.bias[:] = bias
    return d


def out_bytes(win, planes, dtype):
    es = R.ELEM.get(dtype, 2)
    if not (win[2] > 0 and win[3] > 0 and planes in R.PLANES):
        return 64
    hs = 1 if planes == "uv" else 0
    return R.NPLANES[planes] * (win[2] >> hs) * (win[3] >> hs) * es


def run_residual(batches, order, w, h, win, planes, dtype, consts="unit", in_pad=0, out_pad=0, skew=0, npics=None,
                 null=(), stride=None, offs=None, in_skew=0, coef_skew=0, dims=None, coef_blocks=None):
    """h264mi_residual_device over the pictures `order` of `batches`, whose
    records lie in_pad bytes apart and whose pools follow each other in one
    pool; returns rc, the whole output buffer (FRONT + skew sentinel bytes,
    then pictures out_stride apart, then 64 sentinel bytes), the first
    picture's offset, out_stride and a picture's bytes."""
    import torch
    L = _mi()
    nbytes = out_bytes(win, planes, dtype)
    in_stride = len(batches[0][0]) + in_pad
    out_stride = nbytes + out_pad if stride is None else stride
    host = np.zeros(in_stride * len(batches) + 64, dtype=np.uint8)
    bases, pool = [], b""
    for k, (r, c) in enumerate(batches):
        host[k * in_stride:k * in_stride + len(r)] = np.frombuffer(r, dtype=np.uint8)
        bases.append(len(pool) // 32)
        pool += c
    d_in = torch.from_numpy(host).to("cuda")
    d_coef = torch.from_numpy(np.frombuffer(pool + bytes(64), dtype=np.uint8).copy()).to("cuda")
    assert d_in.data_ptr() % 16 == 0 and d_coef.data_ptr() % 16 == 0
    n = len(order)
    offs = (C.c_size_t * n)(*([k * in_stride for k in order] if offs is None else offs))
    cb = (C.c_uint32 * n)(*[bases[k] for k in order])
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    desc = make_desc(win, planes, dtype, consts)
    wm, hm = dims or (w, h)
    rc = L.h264mi_residual_device(None if "in" in null else d_in.data_ptr() + in_skew, None if "offs" in null else offs,
                                  None if "coef" in null else d_coef.data_ptr() + coef_skew,
                                  None if "bases" in null else cb,
                                  len(pool) // 32 if coef_blocks is None else coef_blocks,
                                  n if npics is None else npics, wm, hm, None if "desc" in null else C.byref(desc),
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
    return ["unit"] if dtype == "int16" else sorted(R.CONSTS)       # int16 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_kernel_vs_oracle(synthetic, size, dtype):
    """Every `planes` over every window, with every constant set."""
    w, h = SIZES[size]
    batches, fields = synthetic[size]
    for planes in R.PLANES:
        for win in windows(w, h, planes):
            for consts in consts_of(dtype):
                rc, out, first, stride, nbytes = run_residual(batches[:1], [0], w, h, win, planes, dtype, consts)
                assert rc == 0, (planes, win, consts)
                assert same(out[first:first + nbytes], R.expect(fields[0], planes, win, dtype, consts)), (planes, win, consts)
                assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (planes, win, consts)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("size", ["3x2", "5x3", "9x2"])
def test_kernel_batched_padded_strides_write_nothing_else(synthetic, size, dtype):
    """Picture list [2, 0, 2, 1] of three batches 96 pad bytes apart;
    out_stride padded by 5 elements (never a multiple of 16 bytes: the element
    path), by 48 bytes (16-byte rows keep the 16-byte stores) and by 48 bytes
    with d_out one element past a 16-byte boundary: every picture is right and
    no pad byte changes, the first one past each picture included."""
    w, h = SIZES[size]
    batches, fields = synthetic[size]
    es = R.ELEM[dtype]
    order = [2, 0, 2, 1]
    for planes in R.PLANES:
        wins = windows(w, h, planes)
        for win in (wins[0], wins[5], wins[4]):
            for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
                rc, out, first, stride, nbytes = run_residual(batches, order, w, h, win, planes, dtype, "norm", in_pad=96,
                                                              out_pad=out_pad, skew=skew)
                what = (planes, win, out_pad, skew)
                assert rc == 0, what
                assert (out[:first] == SENTINEL).all(), what
                for k, i in enumerate(order):
                    o = first + k * stride
                    assert same(out[o:o + nbytes], R.expect(fields[i], planes, win, dtype, "norm")), what + (k,)
                    assert (out[o + nbytes:o + stride] == SENTINEL).all(), what + (k,)
                assert (out[first + len(order) * stride:] == SENTINEL).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_kernel_list_longer_than_one_launch(synthetic, dtype):
    w, h = SIZES["3x2"]
    batches, fields = synthetic["3x2"]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win = (5, 3, 37, 26)
    rc, out, first, stride, nbytes = run_residual(batches, order, w, h, win, "yuv", dtype, "mixed", in_pad=96)
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], R.expect(fields[i], "yuv", win, dtype, "mixed")), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["3x2", "9x2"])
def test_kernel_pool_declared_shorter_than_it_is(synthetic, size):
    """The buffer keeps its size and only coef_blocks shrinks: an MB whose
    blocks would end beyond it exports zeros, every other MB is unchanged."""
    w, h = SIZES[size]
    batches, fields = synthetic[size]
    rec, pool = batches[0]
    total = len(pool) // 32
    win = (0, 0, 16 * w, 16 * h)
    full = R.expect(fields[0], "yuv", win, "int16")
    seen_cut = seen_kept = False
    for nblk in (total - 1, total // 2, 3, 0):
        f = R.field(rec, pool, w, h, coef_blocks=nblk)
        want = R.expect(f, "yuv", win, "int16")
        seen_cut |= not np.array_equal(want, full)
        seen_kept |= bool(want.any())
        rc, out, first, stride, nbytes = run_residual(batches[:1], [0], w, h, win, "yuv", "int16", coef_blocks=nblk)
        assert rc == 0 and same(out[first:first + nbytes], want), nblk
    assert seen_cut and seen_kept
    # the bound counts from the picture's base: the second batch with the first one's blocks ahead of it
    base = total
    nblk = base + len(batches[1][1]) // 64
    f = R.field(batches[1][0], batches[1][1], w, h, coef_blocks=nblk - base)
    rc, out, first, stride, nbytes = run_residual(batches[:2], [1], w, h, win, "yuv", "int16", coef_blocks=nblk)
    assert rc == 0 and same(out[first:first + nbytes], R.expect(f, "yuv", win, "int16"))


@pytest.mark.gpu
def test_kernel_rejects_bad_arguments(synthetic):
    w, h = SIZES["3x2"]
    batches, _ = synthetic["3x2"]
    good = (2, 2, 8, 8)

    def refused(**kw):
        args = dict(win=good, planes="uv", dtype="float16")
        args.update(kw)
        win, planes, dtype = args.pop("win"), args.pop("planes"), args.pop("dtype")
        rc, out, *_ = run_residual(batches[:1], [0], w, h, win, planes, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    rc, out, first, _, nbytes = run_residual(batches[:1], [0], w, h, good, "uv", "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    for planes in (3, -1, 255):
        refused(planes=planes)
    for dtype in (0, 5, -1):                             # uint8 and unknown types
        refused(dtype=dtype)
    for win in ((0, 0, 50, 32), (0, 0, 48, 34), (48, 0, 2, 2), (0, 32, 2, 2), (40, 0, 10, 2), (0, 30, 2, 4), (-2, 0, 4, 4),
                (0, -2, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -4, 4)):
        refused(win=win)
        refused(win=win, planes="y")
    for win in ((1, 2, 8, 8), (2, 1, 8, 8), (2, 2, 7, 8), (2, 2, 8, 7)):    # odd "uv" windows
        refused(win=win)
    for null in ("in", "offs", "coef", "bases", "desc", "out"):
        refused(null=(null,))
    refused(npics=0)
    refused(npics=-1)
    refused(dims=(0, h))
    refused(dims=(w, 0))
    for dtype, skew in (("int16", 1), ("float16", 1), ("bfloat16", 1), ("float32", 2)):
        refused(dtype=dtype, skew=skew)                  # d_out not a multiple of the element size
    refused(dtype="float16", stride=2 * 4 * 4 * 2 + 1)   # nor out_stride
    refused(dtype="float32", stride=2 * 4 * 4 * 4 + 2)
    refused(offs=[48])                                   # not a multiple of sizeof(MbRec)
    refused(offs=[100])
    refused(in_skew=4)                                   # d_recs not 16-byte aligned
    refused(coef_skew=8)                                 # nor d_coef


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
def test_engine_keeps_coefficients_per_slot(captured):
    """After each picture its slot's residual is the oracle's over its records
    and coefficients; at the end every slot holds the last picture decoded into
    it, the others zeros; and retention changes no pixel."""
    import torch
    from broadway_amd.engine import Engine
    cap, fields = captured
    w, h = cap.w_mbs, cap.h_mbs
    plain = Engine(w, h, 1, cap.nslots)
    for pic in cap.pictures:
        plain.decode([0], [pic])
    want_pixels = [plain.read(0, s).tobytes() for s in range(cap.nslots)]
    with pytest.raises(RuntimeError):
        plain.to_residual([0], [0])                     # retention is off
    plain.keep_records()
    with pytest.raises(RuntimeError):
        plain.to_residual([0], [0])                     # the records alone are not enough
    plain.close()

    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_coefs()
    side = torch.cuda.Stream()
    kinds = [("y", "int16", "unit"), ("yuv", "float16", "norm"), ("uv", "float32", "mixed"), ("yuv", "bfloat16", "mixed"),
             ("yuv", "int16", "unit")]
    got, last = [], {}
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        planes, dtype, consts = kinds[k % len(kinds)]
        scale, bias = R.CONSTS[consts]
        n = R.NPLANES[planes]
        got.append(eng.to_residual([0], [pic.cur_slot], planes=planes, dtype=getattr(torch, dtype), scale=scale[:n],
                                   bias=bias[:n], stream=side))
        last[pic.cur_slot] = k
    torch.cuda.synchronize()
    assert eng.errors() == 0
    whole = (0, 0, 16 * w, 16 * h)
    for k, t in enumerate(got):
        planes, dtype, consts = kinds[k % len(kinds)]
        hs = 1 if planes == "uv" else 0
        assert tuple(t.shape) == (1, R.NPLANES[planes], 16 * h >> hs, 16 * w >> hs), k
        assert t.dtype == getattr(torch, dtype) and t.is_cuda
        assert same(tensor_bytes(t), R.expect(fields[k], planes, whole, dtype, consts)), k
    # every slot at once, with the defaults over the crop window
    t = eng.to_residual([0] * cap.nslots, list(range(cap.nslots)), window=CROP)
    torch.cuda.synchronize()
    assert tuple(t.shape) == (cap.nslots, 1, CROP[3], CROP[2]) and t.dtype == torch.int16
    zero = R.zero_field(w, h)
    for s in range(cap.nslots):
        f = fields[last[s]] if s in last else zero
        assert same(tensor_bytes(t[s]), R.expect(f, "y", CROP, "int16")), s
    assert [eng.read(0, s).tobytes() for s in range(cap.nslots)] == want_pixels
    # the records travel with the coefficients: to_mbinfo works while keep_coefs is on
    assert tuple(eng.to_mbinfo([0], [0]).shape) == (1, 2, 4 * h, 4 * w)
    # forgetting a slot; a bad slot or window; switching off and on again starts empty
    s = cap.pictures[-1].cur_slot
    assert R.expect(fields[last[s]], "yuv", whole, "int16").any()
    eng.forget_records(0, s)
    t = eng.to_residual([0], [s], planes="yuv")
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), R.expect(zero, "yuv", whole, "int16"))
    for kw in (dict(streams=[1], slots=[0]), dict(streams=[0], slots=[cap.nslots]),
               dict(streams=[0], slots=[0], window=(0, 0, 16 * w + 1, 1))):
        with pytest.raises(RuntimeError):
            eng.to_residual(**kw)
    s0 = cap.pictures[0].cur_slot
    eng.keep_coefs(False)
    with pytest.raises(RuntimeError):
        eng.to_residual([0], [s0])
    with pytest.raises(RuntimeError):
        eng.to_mbinfo([0], [s0])                        # the records' own switch was never on
    eng.keep_coefs(True)
    t = eng.to_residual([0], [s0], planes="yuv")
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), R.expect(zero, "yuv", whole, "int16"))
    # with the records' own switch on, the records outlive the coefficients -- and then do not serve a residual
    eng.keep_records()
    eng.decode([0], [cap.pictures[0]])
    eng.keep_coefs(False)
    assert tuple(eng.to_mbinfo([0], [s0]).shape) == (1, 2, 4 * h, 4 * w)
    eng.keep_coefs(True)
    t = eng.to_residual([0], [s0], planes="yuv")
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), R.expect(zero, "yuv", whole, "int16"))
    eng.close()


@pytest.mark.gpu
def test_engine_export_is_ordered_against_the_next_decode_into_the_slot(captured):
    """Export into ``out``, then decode the next picture into the same slot
    with no synchronisation in between: ``out`` holds the earlier picture."""
    import torch
    from broadway_amd.engine import Engine
    cap, fields = captured
    slots = [p.cur_slot for p in cap.pictures]
    k1 = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])      # the first decode into a used slot
    k0 = slots.index(slots[k1])
    w, h = cap.w_mbs, cap.h_mbs
    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_coefs()
    out = torch.empty((1, 3, 16 * h, 16 * w), dtype=torch.int16, device="cuda")
    for k in range(k1):
        eng.decode([0], [cap.pictures[k]])
    assert eng.to_residual([0], [slots[k0]], planes="yuv", out=out) is out
    eng.decode([0], [cap.pictures[k1]])
    after = eng.to_residual([0], [slots[k1]], planes="yuv")
    torch.cuda.synchronize()
    whole = (0, 0, 16 * w, 16 * h)
    assert same(tensor_bytes(out), R.expect(fields[k0], "yuv", whole, "int16"))
    assert same(tensor_bytes(after), R.expect(fields[k1], "yuv", whole, "int16"))
    assert not np.array_equal(tensor_bytes(out), tensor_bytes(after))
    for bad in (torch.empty((1, 3, 16 * h, 16 * w + 1), dtype=torch.int16, device="cuda"),
                torch.empty((1, 3, 16 * h, 16 * w), dtype=torch.float16, device="cuda"),
                torch.empty((1, 3, 16 * h, 16 * w), dtype=torch.int16, device="cpu"),
                torch.empty((1, 3, 16 * w, 16 * h), dtype=torch.int16, device="cuda").transpose(2, 3)):
        with pytest.raises(ValueError):
            eng.to_residual([0], [slots[k0]], planes="yuv", out=bad)
    eng.close()


def decode_js(nals, opts):
    """(pictures, their residual and mbinfo tensors, (w, h) per picture) of a Decoder run"""
    got, resid, infos, dims = [], [], [], []
    dec = Decoder(opts)

    def on_picture(buf, w, h, _):
        # (a host picture is a view of the decoder's buffer: copied here; a tensor is the caller's)
        got.append(bytes(buf) if isinstance(buf, np.ndarray) else buf)
        resid.append(dec.residual)
        infos.append(dec.mbinfo)
        dims.append((w, h))

    dec.onPictureDecoded = on_picture
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, resid, infos, dims


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "tensor", "crop_rgb", "mbinfo"])
def test_decoder_residual_option(captured, mode):
    """decoder.residual, set before each onPictureDecoded call, is the
    oracle's residual of that picture over the crop window (this stream's
    output order is its decode order), whatever the output mode and together
    with ``mbinfo``; and the pixels are those of the same run without it."""
    import torch
    cap, fields = captured
    nals = split_annexb(case_stream())
    base = {"plain": {}, "tensor": {"tensor": True}, "crop_rgb": {"crop": True, "rgb": True},
            "mbinfo": {"mbinfo": True}}[mode]
    want, none, winfos, wdims = decode_js(nals, base)
    assert none == [None] * len(want)
    got, resid, infos, dims = decode_js(nals, dict(base, residual=True))
    all3, resid3, infos3, _ = decode_js(nals, dict(base, residual={"planes": "yuv", "dtype": torch.float32,
                                                                   "scale": R.CONSTS["mixed"][0],
                                                                   "bias": R.CONSTS["mixed"][1]}))
    uv, resid2, _, _ = decode_js(nals, dict(base, residual={"planes": "uv", "dtype": torch.float16}))
    assert len(got) == len(want) == len(all3) == len(uv) == cap.npics and dims == wdims
    x, y, cw, ch = CROP
    for k in range(cap.npics):
        if mode == "tensor":
            assert torch.equal(got[k], want[k]) and torch.equal(all3[k], want[k]) and torch.equal(uv[k], want[k]), k
        else:
            assert got[k] == want[k] and all3[k] == want[k] and uv[k] == want[k], k
        if mode == "mbinfo":
            assert torch.equal(infos[k], winfos[k]) and torch.equal(infos3[k], winfos[k]), k
        else:
            assert infos[k] is None
        t = resid[k]
        assert tuple(t.shape) == (1, ch, cw) and t.dtype == torch.int16 and t.is_cuda, k
        assert same(tensor_bytes(t), R.expect(fields[k], "y", CROP, "int16")), k
        t = resid3[k]
        assert tuple(t.shape) == (3, ch, cw) and t.dtype == torch.float32, k
        assert same(tensor_bytes(t), R.expect(fields[k], "yuv", CROP, "float32", "mixed")), k
        t = resid2[k]
        assert tuple(t.shape) == (2, ch // 2, cw // 2) and t.dtype == torch.float16, k
        assert same(tensor_bytes(t), R.expect(fields[k], "uv", CROP, "float16")), k


@pytest.mark.gpu
def test_swdec_last_picture_residual_return_codes(captured):
    """H264SWDEC_OK before any picture; H264SWDEC_PARAM_ERR with retention
    never switched on and for what the export refuses; H264SWDEC_PIC_RDY and
    the residual after a picture; a desc with its own window."""
    import torch
    from broadway_amd import _lib
    cap, fields = captured
    L = _mi()
    stream = case_stream()
    dst = torch.full((3 * 96 * 64 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    cur = torch.cuda.current_stream().cuda_stream

    def first_picture(inst):
        """feed NALs until a picture is delivered"""
        pic = _lib.H264SwDecPicture()
        for nal in split_annexb(stream):
            buf = (C.c_uint8 * len(nal)).from_buffer_copy(nal)
            inp, out = _lib.H264SwDecInput(), _lib.H264SwDecOutput()
            inp.pStream, inp.dataLen = C.cast(buf, C.POINTER(C.c_uint8)), len(nal)
            while inp.dataLen:
                ret = L.H264SwDecDecode(inst, C.byref(inp), C.byref(out))
                used = C.cast(out.pStrmCurrPos, C.c_void_p).value - C.cast(inp.pStream, C.c_void_p).value
                if ret == _lib.H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY:
                    inp.dataLen -= used
                    inp.pStream = out.pStrmCurrPos
                else:
                    inp.dataLen = 0
                if ret in (_lib.H264SWDEC_PIC_RDY, _lib.H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY):
                    if L.H264SwDecNextPicture(inst, C.byref(pic), 0) == _lib.H264SWDEC_PIC_RDY:
                        return True
        return False

    whole = make_desc((0, 0, 0, 0), "yuv", "int16")
    # retention never switched on (the records' alone is not enough)
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecKeepMbInfo(inst, 1) == _lib.H264SWDEC_OK
    assert first_picture(inst)
    assert L.H264SwDecLastPictureResidual(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    L.H264SwDecRelease(inst)
    # retention on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecKeepResidual(inst, 1) == _lib.H264SWDEC_OK
    assert L.H264SwDecLastPictureResidual(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_OK
    assert first_picture(inst)
    for bad in (make_desc((0, 0, 0, 0), 3, "int16"), make_desc((0, 0, 0, 0), -1, "int16"),
                make_desc((0, 0, 0, 0), "yuv", 0), make_desc((0, 0, 0, 0), "yuv", 5),
                make_desc((0, 0, 97, 1), "y", "int16"), make_desc((0, 64, 1, 1), "y", "int16"),
                make_desc((0, 0, 4, 0), "y", "int16"), make_desc((0, 0, 0, 4), "y", "int16"),
                make_desc((1, 0, 4, 4), "uv", "int16"), make_desc((0, 0, 4, 3), "uv", "int16")):
        assert L.H264SwDecLastPictureResidual(inst, C.byref(bad), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureResidual(inst, None, dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureResidual(inst, C.byref(whole), None, cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureResidual(inst, C.byref(whole), dst.data_ptr() + 1, cur) == _lib.H264SWDEC_PARAM_ERR
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()                       # nothing was queued
    assert L.H264SwDecLastPictureResidual(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    win = (6, 2, 42, 30)
    own = make_desc(win, "uv", "float16", "mixed")
    n2 = 2 * 21 * 15 * 2
    dst2 = torch.full((n2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert L.H264SwDecLastPictureResidual(inst, C.byref(own), dst2.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    torch.cuda.synchronize()
    n = 3 * CROP[2] * CROP[3] * 2
    got = dst.cpu().numpy()
    assert same(got[:n], R.expect(fields[0], "yuv", CROP, "int16")) and (got[n:] == SENTINEL).all()
    got = dst2.cpu().numpy()
    assert same(got[:n2], R.expect(fields[0], "uv", win, "float16", "mixed")) and (got[n2:] == SENTINEL).all()
    L.H264SwDecRelease(inst)
