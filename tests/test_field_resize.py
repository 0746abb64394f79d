"""Resized accumulated-motion and accumulated-residual exports
(field_resize.hip): ``size=(oh, ow)`` on the two fields -- the
stateless h264mi_accmv_resize_device / h264mi_accres_resize_device, the engine's
h264mi_engine_export_accmv_resized / _accres_resized (Engine.to_accmv /
to_accres), and H264SwDecLastPictureAccMotionResized (Decoder's ``accmv``
option).

The oracle (tests/_field_resize.py) restates the definition of include/h264mi.h
in numpy int64 on top of the unresized fields' oracles (tests/_accmv.py,
tests/_accres.py).  Every comparison is exact equality of bytes."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _accmv as A
import _accres as R
import _field_resize as F
import _mbinfo as M
from _resize import taps
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 32                    # pictures per export launch
NOKEY = (1 << 64) - 1       # (size_t)-1
STREAM_SHA256 = "9cebfabe58154b0e80fb1277b2af7ad4c637be22564f4ab33997a6c3d75dcc48"
SENTINEL = 0xA5
FRONT = 64
ALL = list(range(5))
DIMS = (6, 4)               # MBs: 96 x 64 samples
WHOLE = (0, 0, 96, 64)


def case_stream():
    """the pinned stream of tests/test_accmv.py and tests/test_accres.py"""
    s = gen.generate(2, 7, w_mbs=6, h_mbs=4, nframes=10, gop=5, num_ref_frames=4, offpic_pct=25, pm_intra=10, slices=2)
    assert hashlib.sha256(s).hexdigest() == STREAM_SHA256, "generator drift"
    return s


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_crop.py: the decoder instances here pool engines."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


@pytest.fixture(scope="module")
def captured():
    from broadway_amd.engine import Capture
    cap = Capture(case_stream())
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs, cap.npics) == (6, 4, 10)
    return cap


def same(got, want):
    """Exact equality; what differs is printed before the assertion fails."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape == want.shape and np.array_equal(got, want):
        return True
    if got.shape != want.shape:
        print(f"shapes differ: {got.shape} {want.shape}")
    else:
        bad = np.flatnonzero(got != want)
        print(f"{bad.size} of {want.size} differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()} "
              f"want {want[bad[:8]].tolist()}")
    return False


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


# ------------------------------------------------------------------ CPU ----
def test_oracle_identity_constants_and_ramp():
    """The three consequences of the definition the header states, and the bounds
    of the two accumulators at the extremes."""
    rng = np.random.default_rng(5)
    s = rng.integers(-32767, 32768, (2, 13, 21))
    # identity: one tap of 16384 per output, r = 16 s
    assert all(q.tolist() == [16384] and f == j for j, (f, q) in enumerate(taps(21, 21)))
    assert np.array_equal(F.resize_field(s, 13, 21), 16 * s)
    # constants: r = 16 c at every size, also at 1 x 1 and at the extremes
    for c in (-32767, -255, -1, 0, 1, 255, 32767):
        for (gh, gw), (oh, ow) in (((64, 96), (1, 3)), ((64, 96), (23, 37)), ((32, 64), (1, 2)), ((6, 10), (17, 31)),
                                   ((16, 64), (3, 5)), ((1, 1), (2, 3))):
            acc, inner = F.resize_acc(np.full((gh, gw), c), oh, ow)
            assert (acc == c * 16384 * 16384).all() and inner == abs(c) * 16384
            assert inner < 1 << 29 and abs(c) * 16384 * 16384 < 1 << 43
            assert (F.resize_field(np.full((gh, gw), c), oh, ow) == 16 * c).all()
    # alternating extremes stay inside both bounds too
    chk = np.where((np.add.outer(np.arange(64), np.arange(96)) & 1) == 0, 32767, -32767)
    acc, inner = F.resize_acc(chk, 2, 3)
    assert inner < 1 << 29 and np.abs(acc).max() < 1 << 43
    # the ramp JX = x over 96 columns -> 37: away from the two outputs at each
    # end, r / 16 is within 1 / 16 of the output's centre
    ramp = np.broadcast_to(np.arange(96), (8, 96))
    r = F.resize_field(ramp, 8, 37)
    centre = (np.arange(37) + 0.5) * 96 / 37 - 0.5
    err = np.abs(r[:, 2:-2] / 16.0 - centre[2:-2])
    print("ramp: largest distance from the centre", err.max())
    assert err.max() <= 1 / 16
    assert (r == r[:1]).all()


def test_exactness_premise():
    """_mbinfo.convert's premise for the values here: float64(r / 16) *
    float64(scale) + float64(bias) is exact for both constant sets, so one
    rounding to fp32 equals the hardware fma of (float)r * 0.0625f."""
    rs = [0, 1, -1, 7, 8, 9, -8, 255 * 16, -255 * 16 + 3, 32767 * 16, -32767 * 16, 524287, -524287, 123457, -98765]
    for consts in ("unit", "mixed"):
        scale, bias = M.CONSTS[consts]
        for s, b in zip(scale[:8], bias[:8]):
            s32, b32 = float(np.float32(s)), float(np.float32(b))
            for r in rs:
                assert float(np.float32(r) * np.float32(0.0625)) == r / 16.0          # exact in fp32
                exact = Fraction(r, 16) * Fraction(s32) + Fraction(b32)
                assert Fraction((r / 16.0) * s32 + b32) == exact, (consts, s, b, r)


ACCMV_GRID = {
    "identity": "accept", "down": "accept", "up": "accept", "ow_0": "refuse", "ow_1": "accept", "ow_16384": "accept",
    "ow_16385": "refuse", "oh_0": "refuse", "oh_1": "accept", "oh_16384": "accept", "oh_16385": "refuse",
    "ow_negative": "refuse", "cw_32_ow": "accept", "cw_32_ow_plus_2": "refuse", "ch_32_oh": "accept",
    "ch_32_oh_plus_1": "refuse", "filter_1": "refuse", "filter_minus_1": "refuse", "dtype_u8": "refuse",
    "nch_0": "refuse", "nch_9": "refuse", "window_past_the_picture": "refuse", "cw_0": "refuse",
    "grid_16384": "accept", "grid_16386": "refuse", "far_right": "accept",
}
ACCMV_FIXED_REFUSED = {"ow_0", "ow_16385", "oh_0", "oh_16385", "ow_negative", "filter_1", "filter_minus_1", "dtype_u8",
                       "nch_0", "nch_9"}
ACCRES_GRID = {
    "identity": "accept", "rgb_down": "accept", "uv_identity": "accept", "ow_0": "refuse", "ow_1": "accept",
    "ow_16384": "accept", "ow_16385": "refuse", "oh_16385": "refuse", "cw_32_ow": "accept", "cw_32_ow_plus_2": "refuse",
    "uv_cw_64_ow": "accept", "uv_cw_64_ow_plus_2": "refuse", "uv_ch_64_oh": "accept", "y_cw_64_ow": "refuse",
    "uv_odd_window": "refuse", "filter_1": "refuse", "dtype_u8": "refuse", "planes_4": "refuse", "colour_4": "refuse",
    "unanchored_2": "refuse", "window_past_the_picture": "refuse", "uv_grid_16384": "accept", "y_grid_16386": "refuse",
}
ACCRES_FIXED_REFUSED = {"ow_0", "ow_16385", "oh_16385", "filter_1", "dtype_u8", "planes_4", "colour_4", "unanchored_2"}


def test_descriptor_rules(tmp_path):
    """common/export_desc.h's rules of the two resize descriptors walked by
    tests/field_resize_desc_check.c under AddressSanitizer + UBSan, as
    tests/test_accmv.py walks the unresized ones; the expected column is written
    out from include/h264mi.h: the inner descriptor's rules; the triangle
    filter; 1 <= ow, oh <= 16384; the source grid (UV: half the window) at most
    16384 a side and at most 32 ow by 32 oh.  The fixed part refuses what does
    not depend on the picture."""
    exe = str(tmp_path / "field_resize_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "field_resize_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    got = {"accmv": {}, "accres": {}}
    fixed = {"accmv": {}, "accres": {}}
    for ln in p.stdout.splitlines():
        f = ln.split()
        into, f = (fixed, f[1:]) if f[0] == "fixed" else (got, f)
        assert f[1] not in into[f[0]], ln
        into[f[0]][f[1]] = f[2]
    for kind, grid, refused in (("accmv", ACCMV_GRID, ACCMV_FIXED_REFUSED), ("accres", ACCRES_GRID, ACCRES_FIXED_REFUSED)):
        assert sorted(got[kind]) == sorted(grid)
        assert {k: v for k, v in got[kind].items() if v != grid[k]} == {}
        assert {k for k, v in fixed[kind].items() if v == "refuse"} == refused, kind


def test_library_exports_the_resized_entry_points():
    from broadway_amd import _lib
    L = _lib.mi()           # (first: it loads torch's HIP runtime before the library binds to one)
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    for name, nargs in (("h264mi_accmv_resize_device", 9), ("h264mi_accres_resize_device", 13),
                        ("h264mi_engine_export_accmv_resized", 8), ("h264mi_engine_export_accres_resized", 8),
                        ("H264SwDecLastPictureAccMotionResized", 4)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { h264mi_accmv_desc f; int ow, oh, filter; } / { h264mi_accres_desc f; int ow, oh, filter; }
    for D, inner in ((_lib.AccMvResizeDesc, _lib.AccMvDesc), (_lib.AccResResizeDesc, _lib.AccResDesc)):
        n = C.sizeof(inner)
        assert C.sizeof(D) == n + 12 and D.f.offset == 0
        assert (D.ow.offset, D.oh.offset, D.filter.offset) == (n, n + 4, n + 8)
    assert C.sizeof(_lib.AccMvDesc) == 120 and C.sizeof(_lib.AccResDesc) == 56
    assert L.h264mi_engine_abi() == 6


def test_size_argument_validation():
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import accmv_desc, accres_desc
    d, n, dt = accmv_desc(("jx", "ady"), (1, 2, 30, 50), torch.float16, scale=0.25, size=(7, 9))
    assert isinstance(d, _lib.AccMvResizeDesc) and (n, dt) == (2, torch.float16)
    assert (d.oh, d.ow, d.filter) == (7, 9, _lib.RESIZE_TRIANGLE)
    assert (d.f.x, d.f.y, d.f.cw, d.f.ch, d.f.nch, d.f.dtype) == (1, 2, 30, 50, 2, _lib.TENSOR_F16)
    assert list(d.f.id)[:2] == [2, 1] and list(d.f.scale)[:2] == [0.25, 0.25]
    d, n, dt = accres_desc("rgb", (0, 0, 32, 16), torch.float32, colour="bt709-full", unanchored="zero", size=(1, 16384))
    assert isinstance(d, _lib.AccResResizeDesc) and (n, dt) == (3, torch.float32)
    assert (d.oh, d.ow, d.filter, d.f.planes, d.f.colour, d.f.unanchored) == (1, 16384, _lib.RESIZE_TRIANGLE, 3, 3, 1)
    assert type(accmv_desc(size=None)[0]) is _lib.AccMvDesc and type(accres_desc(size=None)[0]) is _lib.AccResDesc
    assert type(accmv_desc()[0]) is _lib.AccMvDesc and type(accres_desc()[0]) is _lib.AccResDesc
    for size in (7, (7,), (7, 9, 11), "ab", (0, 9), (7, 0), (16385, 9), (7, 16385), (-1, 9), ("x", 9)):
        with pytest.raises(ValueError):
            accmv_desc(size=size)
        with pytest.raises(ValueError):
            accres_desc(size=size)
        with pytest.raises(ValueError):
            Decoder({"accmv": {"size": size}})
    with pytest.raises(ValueError):
        accmv_desc(dtype=torch.uint8, size=(7, 9))
    with pytest.raises(ValueError):
        accres_desc(dtype=torch.uint8, size=(7, 9))
    with pytest.raises(ValueError):
        Decoder({"accmv": {"size": (7, 9), "dtype": torch.uint8}})
    for name in ("mbinfo", "residual"):                  # the other fields have no size
        with pytest.raises(ValueError):
            Decoder({name: {"size": (7, 9)}})


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


# window -> size pairs of the motion tests: identity; 2 : 1; off every grid;
# partial tiles on both axes; upscaling from odd offsets; 32 : 1 on both axes
# (64 taps); three outputs of 95 x 63; one source sample
MV_CASES = [(WHOLE, (64, 96)), (WHOLE, (32, 48)), (WHOLE, (23, 37)), (WHOLE, (17, 33)), ((5, 3, 10, 6), (17, 31)),
            ((0, 0, 64, 32), (1, 2)), ((1, 1, 95, 63), (3, 3)), ((7, 9, 1, 1), (2, 3))]
MV_LISTS = [[0, 1], [4, 3, 2, 1, 0, 0, 4, 2]]
# The constant sets under which the identity size is compared with the unresized
# kernels' own bytes.  Both sides compute fma(v, scale, bias) of the same v; the
# resized export rounds it to fp32 and then to the element type, as the header
# defines it and the oracle does.  The unresized kernels' fp16 path rounds the
# exact sum once (the compiler folds fma and conversion into v_fma_mixlo_f16),
# which differs from the definition in about one element in 8192 when scale *
# v is not exact in fp32 -- "mixed"'s 1 / 51.  That is the unresized kernels'
# business (their own tests never meet such an element); with "qpel" the
# product is exact and the two roundings agree.
IDENTITY_CONSTS = {"int16": ["unit"], "float16": ["unit", "qpel"], "bfloat16": ["unit", "mixed"], "float32": ["unit", "mixed"]}


@pytest.fixture(scope="module")
def mv_maps():
    """96 x 64: a map of random words with JX, JY over all of 0..32767 (0x7FFF
    planted) and random ANCHORED, and one of 0x7FFF7FFF; read-only, with their
    five channels"""
    rng = np.random.default_rng(77)
    W, H = 16 * DIMS[0], 16 * DIMS[1]
    m = (rng.integers(0, 32768, (H, W)).astype(np.uint32) | rng.integers(0, 32768, (H, W)).astype(np.uint32) << np.uint32(16) |
         rng.integers(0, 2, (H, W)).astype(np.uint32) << np.uint32(31))
    m[0, 0] = 0x7FFF7FFF
    m[H - 1, W - 1] = 0xFFFF7FFF
    m[5, 7] = 0x7FFF0000
    top = np.full((H, W), 0x7FFF7FFF, dtype=np.uint32)
    maps = [m, top]
    chans = [A.channels(x) for x in maps]
    for a in maps + chans:
        a.setflags(write=False)
    assert chans[0][2].max() == 32767 and chans[0][3].max() == 32767 and chans[1][0].max() == 32767
    return maps, chans


@functools.lru_cache(maxsize=None)
def _mv_resized(key, win, size):
    r = F.resize_field(A.select(_MV_FIELDS[key], ALL, win), *size)
    r.setflags(write=False)
    return r


_MV_FIELDS = {}


def mv_expect(chans, win, size, ids, dtype, consts="unit"):
    """the resized export's bytes; the five channels are resized once per (field, window, size)"""
    _MV_FIELDS[id(chans)] = chans
    scale, bias = M.CONSTS[consts]
    return F.convert(_mv_resized(id(chans), tuple(win), tuple(size))[list(ids)], dtype, scale, bias)


def mv_desc(win, size, ids, dtype, consts="unit", nch=None, filt=0):
    from broadway_amd import _lib
    d = _lib.AccMvResizeDesc()
    d.f.x, d.f.y, d.f.cw, d.f.ch = win
    d.f.nch = len(ids) if nch is None else nch
    d.f.dtype = M.DTYPE_ID.get(dtype, dtype)
    d.f.id[:len(ids)] = ids
    scale, bias = M.CONSTS[consts]
    d.f.scale[:] = scale[:8]
    d.f.bias[:] = bias[:8]
    d.oh, d.ow = size
    d.filter = filt
    return d


def out_buffer(n, nbytes, out_pad, skew, stride):
    import torch
    out_stride = nbytes + out_pad if stride is None else stride
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    return d_out, first, out_stride


def run_mv(maps, order, win, size, ids, dtype, consts="unit", dims=DIMS, out_pad=0, skew=0, stride=None, nch=None,
           filt=0, null=(), npics=None, offs=None, in_skew=0, call_dims=None):
    """h264mi_accmv_resize_device over the maps `order` of `maps` (64 sentinel
    bytes apart); returns rc, the whole output buffer (FRONT + skew sentinel
    bytes, then pictures out_stride apart, then 64 sentinel bytes), the first
    picture's offset, out_stride and a picture's bytes."""
    import torch
    L = _mi()
    es = M.ELEM.get(dtype, 2)
    nbytes = max(len(ids), 1) * max(size[0], 1) * max(size[1], 1) * es
    in_stride = maps[0].nbytes + 64
    host = np.full(in_stride * len(maps) + 64, SENTINEL, dtype=np.uint8)
    for k, m in enumerate(maps):
        host[k * in_stride:k * in_stride + m.nbytes] = m.reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host).to("cuda")
    n = len(order)
    offs = (C.c_size_t * n)(*([k * in_stride for k in order] if offs is None else offs))
    d_out, first, out_stride = out_buffer(n, nbytes, out_pad, skew, stride)
    desc = mv_desc(win, size, ids, dtype, consts, nch, filt)
    wm, hm = call_dims or dims
    rc = L.h264mi_accmv_resize_device(None if "in" in null else d_in.data_ptr() + in_skew, None if "offs" in null else offs,
                                      n if npics is None else npics, wm, hm, None if "desc" in null else C.byref(desc),
                                      None if "out" in null else d_out.data_ptr() + first, out_stride,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


def consts_of(dtype):
    return ["unit"] if dtype == "int16" else ["unit", "mixed"]          # int16 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_motion_kernel_vs_oracle(mv_maps, dtype):
    """Every window -> size pair with both channel lists and constant sets on
    the random map; the identity size also against h264mi_accmv_device's own
    bytes; the map of 0x7FFF7FFF (adx up to +32767) at 1 x 2 and 3 x 3."""
    import torch
    from broadway_amd import _lib
    maps, chans = mv_maps
    for win, size in MV_CASES:
        for ids in MV_LISTS:
            for consts in consts_of(dtype):
                rc, out, first, _, nbytes = run_mv(maps[:1], [0], win, size, ids, dtype, consts)
                assert rc == 0, (win, size, ids, consts)
                assert same(out[first:first + nbytes], mv_expect(chans[0], win, size, ids, dtype, consts)), (win, size, ids, consts)
                assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (win, size, ids)
    for win, size in (((0, 0, 64, 32), (1, 2)), ((1, 1, 95, 63), (3, 3))):
        rc, out, first, _, nbytes = run_mv(maps, [1], win, size, ALL, dtype, "unit")
        assert rc == 0 and same(out[first:first + nbytes], mv_expect(chans[1], win, size, ALL, dtype, "unit")), (win, size)
    # the identity size is the unresized export, byte for byte
    L = _mi()
    ids = MV_LISTS[1]
    d_in = torch.from_numpy(maps[0].reshape(-1).view(np.uint8).copy()).to("cuda")
    n = len(ids) * 64 * 96 * M.ELEM[dtype]
    off = (C.c_size_t * 1)(0)
    st = torch.cuda.current_stream().cuda_stream
    for consts in IDENTITY_CONSTS[dtype]:
        d = mv_desc(WHOLE, (64, 96), ids, dtype, consts)
        assert isinstance(d, _lib.AccMvResizeDesc)
        a = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        b = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert L.h264mi_accmv_device(d_in.data_ptr(), off, 1, *DIMS, C.byref(d.f), a.data_ptr(), n, st) == 0
        assert L.h264mi_accmv_resize_device(d_in.data_ptr(), off, 1, *DIMS, C.byref(d), b.data_ptr(), n, st) == 0
        torch.cuda.synchronize()
        assert same(b.cpu().numpy(), a.cpu().numpy()), consts


@pytest.mark.gpu
def test_motion_kernel_at_the_far_right_of_the_widest_picture():
    """2048 x 1 MBs (32768 x 16, a 2 MB map) of zero words, window (32704, 0,
    64, 16) -> (3, 5): adx about -32700, the negative end of the 43-bit range."""
    w, h = 2048, 1
    m = np.zeros((16, 32768), dtype=np.uint32)
    f = A.channels(m)
    win, size = (32704, 0, 64, 16), (3, 5)
    assert A.select(f, [0], win).min() == -32767 and A.select(f, [0], win).max() == -32704
    for dtype in ("int16", "float32"):
        rc, out, first, _, nbytes = run_mv([m], [0], win, size, ALL, dtype, "unit", dims=(w, h))
        assert rc == 0
        assert same(out[first:first + nbytes], F.expect(A.select(f, ALL, win), size, dtype)), dtype
        assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all()


# --- the residual
RES_DIMS = DIMS


@pytest.fixture(scope="module")
def res_case():
    """96 x 64: two current and two key frames of random bytes, tests/_accres.py's
    planted map, and the extreme frames (all 255, all 0); read-only"""
    rng = np.random.default_rng(4242)
    w, h = RES_DIMS
    frames = [rng.integers(0, 256, R.slot_bytes(w, h), dtype=np.uint8) for _ in range(4)]
    frames += [np.full(R.slot_bytes(w, h), 255, dtype=np.uint8), np.zeros(R.slot_bytes(w, h), dtype=np.uint8)]
    m = R.planted_map(rng, w, h)
    ident = A.identity(w, h, 1)
    for a in frames + [m, ident]:
        a.setflags(write=False)
    return dict(frames=frames, maps=[m, ident])


_RES_FIELDS = {}


@functools.lru_cache(maxsize=None)
def _res_field(key, cur, keyf, mi, planes, policy, colour):
    c = _RES_FIELDS[key]
    v = R.field(c["frames"][cur], None if keyf is None else c["frames"][keyf], c["maps"][mi], *RES_DIMS, planes, policy, colour)
    v.setflags(write=False)
    return v


def res_expect(case, pic, win, size, planes, dtype, policy="key", colour=0, consts="unit"):
    _RES_FIELDS[id(case)] = case
    cur, keyf, mi = pic
    v = R.select(_res_field(id(case), cur, keyf, mi, planes, policy, colour), win, planes)
    return F.expect(v, size, dtype, consts)


def res_desc(win, size, planes, dtype, policy="key", colour=0, consts="unit", filt=0):
    from broadway_amd import _lib
    d = _lib.AccResResizeDesc()
    d.f.x, d.f.y, d.f.cw, d.f.ch = win
    d.f.planes = R.PLANES.get(planes, planes)
    d.f.dtype = M.DTYPE_ID.get(dtype, dtype)
    d.f.colour = colour
    d.f.unanchored = R.POLICY.get(policy, policy)
    scale, bias = M.CONSTS[consts]
    d.f.scale[:] = scale[:3]
    d.f.bias[:] = bias[:3]
    d.oh, d.ow = size
    d.filter = filt
    return d


def run_res(case, order, win, size, planes, dtype, policy="key", colour=0, consts="unit", dims=RES_DIMS, out_pad=0, skew=0,
            stride=None, filt=0, null=(), npics=None, call_dims=None, map_offs=None, key_offs=None, cur_skew=0,
            frames=None, maps=None):
    """h264mi_accres_resize_device over pictures order[k] = (current, key or
    None, map) indices into the case's frames and maps, which lie in one device
    buffer 64 sentinel bytes apart; returns as run_mv."""
    import torch
    L = _mi()
    w, h = dims
    frames = case["frames"] if frames is None else frames
    maps = case["maps"] if maps is None else maps
    fb, mb, pad = R.slot_bytes(w, h), 4 * 256 * w * h, 64
    host = np.full((fb + pad) * len(frames) + (mb + pad) * len(maps) + pad, SENTINEL, dtype=np.uint8)
    map0 = (fb + pad) * len(frames)
    for i, f in enumerate(frames):
        host[i * (fb + pad):i * (fb + pad) + fb] = f
    for i, m in enumerate(maps):
        host[map0 + i * (mb + pad):map0 + i * (mb + pad) + mb] = m.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).to("cuda")
    n = len(order)
    co = (C.c_size_t * n)(*[c * (fb + pad) for c, _, _ in order])
    ko = (C.c_size_t * n)(*([NOKEY if k is None else k * (fb + pad) for _, k, _ in order] if key_offs is None else key_offs))
    mo = (C.c_size_t * n)(*([m * (mb + pad) for _, _, m in order] if map_offs is None else map_offs))
    es = M.ELEM.get(dtype, 2)
    nbytes = R.NPLANES.get(planes, 1) * max(size[0], 1) * max(size[1], 1) * es
    d_out, first, out_stride = out_buffer(n, nbytes, out_pad, skew, stride)
    d = res_desc(win, size, planes, dtype, policy, colour, consts, filt)
    wm, hm = call_dims or dims
    base = dev.data_ptr()
    assert base % 16 == 0
    rc = L.h264mi_accres_resize_device(None if "cur" in null else base + cur_skew, None if "co" in null else co,
                                       None if "key" in null else base, None if "ko" in null else ko,
                                       None if "maps" in null else base + map0, None if "mo" in null else mo,
                                       n if npics is None else npics, wm, hm, None if "desc" in null else C.byref(d),
                                       None if "out" in null else d_out.data_ptr() + first, out_stride,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)                          # the inputs are only read
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


# window -> size pairs per kind of planes; UV resizes the half-resolution grid
# (48 x 32 for the whole picture; 47 x 31 and 1 x 1 in the last two)
RES_CASES = [(WHOLE, (64, 96)), (WHOLE, (23, 37)), ((5, 3, 10, 6), (17, 31)), ((0, 0, 64, 32), (1, 2)),
             ((1, 1, 95, 63), (3, 3)), ((7, 9, 1, 1), (2, 3))]
UV_CASES = [(WHOLE, (32, 48)), (WHOLE, (17, 33)), ((4, 2, 10, 6), (17, 31)), ((0, 0, 64, 32), (1, 2)),
            ((2, 2, 94, 62), (3, 3)), ((6, 8, 2, 2), (2, 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("planes", ["y", "uv", "yuv", "rgb"])
def test_residual_kernel_vs_oracle(res_case, planes):
    """A batch of three pictures over the planted map (runs from every byte
    offset, runs ending on the last byte of each plane, out-of-range words), the
    second without a key (all bias): every window -> size pair, both policies,
    int16 and float16, colour ids 0 and 3 for rgb; the other two element types
    once."""
    order = [(0, 2, 0), (1, None, 0), (1, 3, 0)]
    colours = (0, 3) if planes == "rgb" else (0,)
    cases = [(win, size, policy, dtype, colour, "unit" if dtype == "int16" else "mixed")
             for win, size in (UV_CASES if planes == "uv" else RES_CASES) for policy in ("key", "zero")
             for dtype in ("int16", "float16") for colour in colours]
    win, size = (UV_CASES if planes == "uv" else RES_CASES)[1]
    cases += [(win, size, "zero", "bfloat16", colours[-1], "mixed"), (win, size, "key", "float32", colours[-1], "mixed")]
    for win, size, policy, dtype, colour, consts in cases:
        tag = (win, size, policy, dtype, colour)
        rc, out, first, stride, nbytes = run_res(res_case, order, win, size, planes, dtype, policy, colour, consts)
        assert rc == 0, tag
        for k, pic in enumerate(order):
            o = first + k * stride
            assert same(out[o:o + nbytes], res_expect(res_case, pic, win, size, planes, dtype, policy, colour, consts)), tag + (k,)
        assert (out[:first] == SENTINEL).all() and (out[first + 3 * stride:] == SENTINEL).all(), tag
    # the picture without a key is all bias
    scale, bias = M.CONSTS["mixed"]
    npl = R.NPLANES[planes]
    want = M.convert(np.zeros((npl, size[0], size[1]), dtype=np.int64), "float32", scale, bias)
    assert same(out[first + stride:first + stride + nbytes], want)


@pytest.mark.gpu
def test_residual_kernel_extremes_and_identity(res_case):
    """Current all 255 against key all 0 and the reverse (v = +-255 on Y) at 1 x
    1 and at the identity size; the identity size of random frames equals
    h264mi_accres_device's own bytes."""
    import torch
    for cur, key in ((4, 5), (5, 4)):
        for win, size in (((0, 0, 32, 32), (1, 1)), (WHOLE, (64, 96))):
            for planes, dtype in (("y", "int16"), ("yuv", "float16"), ("rgb", "int16")):
                rc, out, first, _, nbytes = run_res(res_case, [(cur, key, 1)], win, size, planes, dtype)
                assert rc == 0
                want = res_expect(res_case, (cur, key, 1), win, size, planes, dtype)
                assert same(out[first:first + nbytes], want), (cur, win, planes)
                if planes == "y":
                    assert set(np.frombuffer(want.tobytes(), dtype=np.int16).tolist()) == {255 if cur == 4 else -255}
    L = _mi()
    w, h = RES_DIMS
    fb = R.slot_bytes(w, h)
    host = np.concatenate([res_case["frames"][0], res_case["frames"][2], res_case["maps"][0].reshape(-1).view(np.uint8)])
    dev = torch.from_numpy(host).to("cuda")
    st = torch.cuda.current_stream().cuda_stream
    for planes, size, dtype in (("rgb", (64, 96), "float16"), ("uv", (32, 48), "bfloat16"), ("yuv", (64, 96), "float32")):
        d = res_desc(WHOLE, size, planes, dtype, "zero", 3 if planes == "rgb" else 0, "mixed")
        n = R.NPLANES[planes] * size[0] * size[1] * M.ELEM[dtype]
        a = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        b = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        z, ko, mo = (C.c_size_t * 1)(0), (C.c_size_t * 1)(fb), (C.c_size_t * 1)(2 * fb)
        base = dev.data_ptr()
        assert L.h264mi_accres_device(base, z, base, ko, base, mo, 1, w, h, C.byref(d.f), a.data_ptr(), n, st) == 0
        assert L.h264mi_accres_resize_device(base, z, base, ko, base, mo, 1, w, h, C.byref(d), b.data_ptr(), n, st) == 0
        torch.cuda.synchronize()
        assert same(b.cpu().numpy(), a.cpu().numpy()), planes


# --- batches and memory discipline
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_batches_longer_than_one_launch_write_nothing_else(dtype):
    """33 pictures of 1 x 1 MB -> (5, 7): two launches; out_stride 48 bytes
    larger than a picture and d_out one element past a 16-byte boundary: every
    picture is right and no byte before, between or behind them changes."""
    rng = np.random.default_rng(99)
    w, h = 1, 1
    es = M.ELEM[dtype]
    size = (5, 7)
    win = (0, 0, 16, 16)
    maps = [(rng.integers(0, 32768, (16, 16)).astype(np.uint32) | rng.integers(0, 32768, (16, 16)).astype(np.uint32) << np.uint32(16) |
             rng.integers(0, 2, (16, 16)).astype(np.uint32) << np.uint32(31)) for _ in range(3)]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    ids = [1, 0, 4]
    rc, out, first, stride, nbytes = run_mv(maps, order, win, size, ids, dtype, "mixed", dims=(w, h), out_pad=48, skew=es)
    assert rc == 0 and stride == nbytes + 48 and (first % 16) == es
    chans = [A.channels(m) for m in maps]
    assert (out[:first] == SENTINEL).all()
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], F.expect(A.select(chans[i], ids, win), size, dtype, "mixed")), k
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), k
    assert (out[first + len(order) * stride:] == SENTINEL).all()
    # the residual: frames 0..3, a picture in three without a key
    frames = [rng.integers(0, 256, R.slot_bytes(w, h), dtype=np.uint8) for _ in range(4)]
    rmaps = [R.planted_map(rng, w, h), A.step(np.zeros(1, dtype=M.MBREC).tobytes(), w, h, [A.identity(w, h, 1)])]
    rorder = [(k % 2, None if k % 3 == 1 else 2 + (k // 2) % 2, k % 2) for k in range(CAP + 1)]
    rc, out, first, stride, nbytes = run_res(None, rorder, win, size, "rgb", dtype, "zero", 3, "mixed", dims=(w, h), out_pad=48,
                                             skew=es, frames=frames, maps=rmaps)
    assert rc == 0 and stride == nbytes + 48
    scale, bias = M.CONSTS["mixed"]
    assert (out[:first] == SENTINEL).all()
    for k, (c, kf, mi) in enumerate(rorder):
        o = first + k * stride
        v = R.select(R.field(frames[c], None if kf is None else frames[kf], rmaps[mi], w, h, "rgb", "zero", 3), win, "rgb")
        assert same(out[o:o + nbytes], F.expect(v, size, dtype, "mixed")), k
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), k
    assert (out[first + len(rorder) * stride:] == SENTINEL).all()


@pytest.mark.gpu
def test_kernels_reject_bad_arguments(mv_maps, res_case):
    """Every bad argument of the rules returns -1 and nothing is launched."""
    maps, _ = mv_maps
    good = dict(win=(1, 1, 20, 12), size=(5, 7))

    def refused(**kw):
        args = dict(good, ids=[0, 1], dtype="float16")
        args.update(kw)
        win, size, ids, dtype = args.pop("win"), args.pop("size"), args.pop("ids"), args.pop("dtype")
        rc, out, *_ = run_mv(maps[:1], [0], win, size, ids, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    rc, out, first, _, nbytes = run_mv(maps[:1], [0], good["win"], good["size"], [0, 1], "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    for size in ((0, 7), (5, 0), (16385, 7), (5, 16385), (-1, 7)):
        refused(size=size)
    refused(filt=1)
    refused(filt=-1)
    refused(win=(0, 0, 66, 12), size=(5, 2))             # cw > 32 ow
    refused(win=(0, 0, 20, 33), size=(1, 7))             # ch > 32 oh
    for nch in (0, 9, -1):
        refused(nch=nch)
    refused(ids=[0, 5])
    for dtype in (0, 5, -1):                             # uint8 and unknown types
        refused(dtype=dtype)
    for win in ((0, 0, 97, 8), (0, 0, 48, 65), (96, 0, 1, 1), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        refused(win=win)
    for null in ("in", "offs", "desc", "out"):
        refused(null=(null,))
    refused(npics=0)
    refused(npics=-1)
    refused(call_dims=(0, 4))
    refused(call_dims=(2049, 4))
    for dtype, skew in (("int16", 1), ("float16", 1), ("bfloat16", 1), ("float32", 2)):
        refused(dtype=dtype, skew=skew)                  # d_out not a multiple of the element size
    refused(dtype="float16", stride=2 * 5 * 7 * 2 + 1)   # nor out_stride
    refused(dtype="float32", stride=2 * 5 * 7 * 4 + 2)
    refused(offs=[2])                                    # not a multiple of 4
    refused(in_skew=2)
    refused(win=(0, 0, 16386, 16), size=(1, 16384), call_dims=(2048, 1))        # a grid beyond 16384

    def res_refused(**kw):
        args = dict(good, planes="yuv", dtype="float16")
        args.update(kw)
        win, size, planes, dtype = args.pop("win"), args.pop("size"), args.pop("planes"), args.pop("dtype")
        rc, out, *_ = run_res(res_case, [(0, 2, 0)], win, size, planes, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw

    rc, out, first, _, nbytes = run_res(res_case, [(0, 2, 0)], good["win"], good["size"], "yuv", "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()
    for size in ((0, 7), (5, 0), (16385, 7), (5, 16385)):
        res_refused(size=size)
    res_refused(filt=1)
    res_refused(win=(0, 0, 66, 12), size=(5, 2))
    res_refused(win=(0, 0, 66, 12), size=(5, 1), planes="uv")       # a grid of 33 > 32 ow
    res_refused(win=(1, 1, 20, 12), planes="uv")                     # odd
    res_refused(planes=4)
    res_refused(planes=-1)
    res_refused(colour=4)
    res_refused(policy=2)
    for dtype in (0, 5):
        res_refused(dtype=dtype)
    for null in ("cur", "co", "key", "ko", "maps", "mo", "desc", "out"):
        res_refused(null=(null,))
    res_refused(npics=0)
    res_refused(call_dims=(0, 4))
    res_refused(dtype="float16", skew=1)
    res_refused(dtype="float32", stride=3 * 5 * 7 * 4 + 2)
    res_refused(map_offs=[2])
    res_refused(key_offs=[2])
    res_refused(cur_skew=2)
    rc, out, first, _, nbytes = run_res(res_case, [(0, 2, 0)], (0, 0, 66, 12), (5, 2), "uv", "float16")     # a grid of 33 <= 32 ow
    assert rc == 0 and same(out[first:first + nbytes], res_expect(res_case, (0, 2, 0), (0, 0, 66, 12), (5, 2), "uv", "float16"))


# --- the engine
SIZE = (56, 80)


@pytest.mark.gpu
def test_engine_resized_exports_equal_the_oracle_on_its_own_fields(captured):
    """keep_accmv and keep_accres(2) on, the whole stream decoded: for three
    slots at different GOP positions to_accmv(size=) and to_accres(planes="rgb",
    size=) equal the oracle applied to the engine's own full-resolution int16
    field of the same slot; a slot whose key is not held exports all bias."""
    import torch
    from broadway_amd.engine import Engine
    cap = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    eng = Engine(w, h, 1, ns)
    eng.keep_accmv()
    eng.keep_accres(2)
    for pic in cap.pictures:
        eng.decode([0], [pic])
    picked = {cap.pictures[k].cur_slot: k for k in (5, 7, 9)}         # the second GOP's key picture, its 3rd and 5th
    assert len(picked) == 3
    slots = sorted(picked)
    full = eng.to_accmv([0] * 3, slots)
    rfull = eng.to_accres([0] * 3, slots, planes="rgb")
    torch.cuda.synchronize()
    full, rfull = full.cpu().numpy().astype(np.int64), rfull.cpu().numpy().astype(np.int64)
    assert full.shape == (3, 2, 64, 96) and rfull.shape == (3, 3, 64, 96)
    assert (full[1:] != 0).any() and (rfull[1:] != 0).any()
    scale, bias = M.CONSTS["mixed"]
    for dtype, consts in (("int16", "unit"), ("float16", "mixed"), ("float32", "mixed")):
        sc, bi = M.CONSTS[consts]
        t = eng.to_accmv([0] * 3, slots, dtype=getattr(torch, dtype), scale=sc[:2], bias=bi[:2], size=SIZE)
        r = eng.to_accres([0] * 3, slots, planes="rgb", dtype=getattr(torch, dtype), scale=sc[:3], bias=bi[:3], size=SIZE)
        torch.cuda.synchronize()
        assert tuple(t.shape) == (3, 2) + SIZE and tuple(r.shape) == (3, 3) + SIZE and t.is_cuda
        for k in range(3):
            assert same(tensor_bytes(t[k]), F.expect(full[k], SIZE, dtype, consts)), (dtype, k)
            assert same(tensor_bytes(r[k]), F.expect(rfull[k], SIZE, dtype, consts)), (dtype, k)
    # a window and channels of its own
    win = (7, 3, 57, 41)
    t = eng.to_accmv([0], slots[2:], channels=("jy", "anchored", "adx"), window=win, size=(9, 11))
    f = eng.to_accmv([0], slots[2:], channels=("jy", "anchored", "adx"), window=win)
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), F.expect(f.cpu().numpy().astype(np.int64)[0], (9, 11), "int16"))
    out = torch.empty((1, 2) + SIZE, dtype=torch.int16, device="cuda")
    assert eng.to_accmv([0], slots[:1], size=SIZE, out=out) is out
    # a slot whose key is not held: all bias
    s = slots[1]
    assert eng.accres_held(0, s)
    eng.forget_records(0, s)
    assert not eng.accres_held(0, s)
    r = eng.to_accres([0], [s], planes="rgb", dtype=torch.float32, scale=scale[:3], bias=bias[:3], size=SIZE)
    torch.cuda.synchronize()
    assert same(tensor_bytes(r), M.convert(np.zeros((3,) + SIZE, dtype=np.int64), "float32", scale, bias))
    for kw in (dict(size=(1, 80)), dict(size=(56, 2)), dict(window=(0, 0, 97, 1), size=SIZE)):
        with pytest.raises(RuntimeError):
            eng.to_accmv([0], [0], **kw)
        with pytest.raises(RuntimeError):
            eng.to_accres([0], [0], **kw)
    assert eng.errors() == 0
    eng.close()
    plain = Engine(w, h, 1, ns)
    with pytest.raises(RuntimeError):
        plain.to_accmv([0], [0], size=SIZE)                 # retention is off
    with pytest.raises(RuntimeError):
        plain.to_accres([0], [0], size=SIZE)
    plain.close()


@pytest.mark.gpu
def test_engine_resized_export_is_ordered_against_the_next_decode_into_the_slot(captured):
    """tests/test_accmv.py's ordering test with ``size`` set: export into
    ``out``, then decode the next picture into the same slot with no
    synchronisation in between: ``out`` holds the earlier picture's field."""
    import torch
    from broadway_amd.engine import Engine
    cap = captured
    slots = [p.cur_slot for p in cap.pictures]
    k1 = next(k for k in range(2, cap.npics) if slots[k] in slots[1:k])     # the first decode over a P picture's slot
    k0 = slots.index(slots[k1], 1)
    w, h = cap.w_mbs, cap.h_mbs
    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_accmv()
    eng.keep_accres(2)
    out = torch.empty((1, 5) + SIZE, dtype=torch.int16, device="cuda")
    rout = torch.empty((1, 3) + SIZE, dtype=torch.int16, device="cuda")
    for k in range(k1):
        eng.decode([0], [cap.pictures[k]])
    before = eng.to_accmv([0], [slots[k0]], channels=A.CHANNELS)
    rbefore = eng.to_accres([0], [slots[k0]], planes="yuv")
    assert eng.to_accmv([0], [slots[k0]], channels=A.CHANNELS, out=out, size=SIZE) is out
    assert eng.to_accres([0], [slots[k0]], planes="yuv", out=rout, size=SIZE) is rout
    eng.decode([0], [cap.pictures[k1]])
    after = eng.to_accmv([0], [slots[k1]], channels=A.CHANNELS, size=SIZE)
    rafter = eng.to_accres([0], [slots[k1]], planes="yuv", size=SIZE)
    torch.cuda.synchronize()
    assert same(tensor_bytes(out), F.expect(before.cpu().numpy().astype(np.int64)[0], SIZE, "int16"))
    assert same(tensor_bytes(rout), F.expect(rbefore.cpu().numpy().astype(np.int64)[0], SIZE, "int16"))
    assert not np.array_equal(tensor_bytes(out), tensor_bytes(after))
    assert not np.array_equal(tensor_bytes(rout), tensor_bytes(rafter))
    eng.close()


# --- the decoder
def decode_js(nals, opts):
    """(pictures, their accmv tensors) of a Decoder run"""
    got, infos = [], []
    dec = Decoder(opts)

    def on_picture(buf, w, h, _):
        got.append(bytes(buf) if isinstance(buf, np.ndarray) else buf)
        infos.append(dec.accmv)

    dec.onPictureDecoded = on_picture
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, infos


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "tensor"])
def test_decoder_accmv_size_option(captured, mode):
    """decoder.accmv with ``size`` is the oracle applied to what a second
    decoder without ``size`` delivers for the same picture over the crop window,
    whatever the output mode; the pixels are the same."""
    import torch
    cap = captured
    nals = split_annexb(case_stream())
    base = {"plain": {}, "tensor": {"tensor": True}}[mode]
    size = (23, 37)
    want, full = decode_js(nals, dict(base, accmv=True))
    got, small = decode_js(nals, dict(base, accmv={"size": size}))
    sc, bi = M.CONSTS["mixed"]
    opts = {"channels": A.CHANNELS, "dtype": torch.float32, "scale": sc[:5], "bias": bi[:5]}
    _, full5 = decode_js(nals, dict(base, accmv=dict(opts, dtype=torch.int16, scale=None, bias=None)))
    all5, small5 = decode_js(nals, dict(base, accmv=dict(opts, size=size)))
    assert len(got) == len(want) == len(all5) == cap.npics
    for k in range(cap.npics):
        if mode == "tensor":
            assert torch.equal(got[k], want[k]) and torch.equal(all5[k], want[k]), k
        else:
            assert got[k] == want[k] and all5[k] == want[k], k
        t = small[k]
        assert tuple(t.shape) == (2,) + size and t.dtype == torch.int16 and t.is_cuda, k
        assert tuple(full[k].shape)[1:] != (64, 96)                          # the stream is cropped
        assert same(tensor_bytes(t), F.expect(full[k].cpu().numpy().astype(np.int64), size, "int16")), k
        t = small5[k]
        assert tuple(t.shape) == (5,) + size and t.dtype == torch.float32, k
        assert same(tensor_bytes(t), F.expect(full5[k].cpu().numpy().astype(np.int64), size, "float32", "mixed")), k
    assert any(bool(t.any()) for t in small[1:])


@pytest.mark.gpu
def test_swdec_last_picture_accmotion_resized_return_codes():
    """H264SWDEC_OK before any picture; H264SWDEC_PARAM_ERR with retention never
    switched on, on a bad descriptor and on a d_dst off the device;
    H264SWDEC_PIC_RDY and the field after a picture."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    stream = case_stream()
    size = (9, 13)
    n = 5 * size[0] * size[1] * 2
    dst = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    full = torch.full((5 * 64 * 96 * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    cur = torch.cuda.current_stream().cuda_stream
    RESIZED = L.H264SwDecLastPictureAccMotionResized

    def pictures(inst, n):
        """feed NALs until n pictures were delivered"""
        pic = _lib.H264SwDecPicture()
        seen = 0
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
                    while L.H264SwDecNextPicture(inst, C.byref(pic), 0) == _lib.H264SWDEC_PIC_RDY:
                        seen += 1
                        if seen == n:
                            return True
        return False

    crop = mv_desc((0, 0, 0, 0), size, ALL, "int16")
    # retention never switched on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert pictures(inst, 1)
    assert RESIZED(inst, C.byref(crop), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    L.H264SwDecRelease(inst)
    # retention on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecKeepAccMotion(inst, 1) == _lib.H264SWDEC_OK
    assert RESIZED(inst, C.byref(crop), dst.data_ptr(), cur) == _lib.H264SWDEC_OK
    assert pictures(inst, 2)                            # the second picture: a P picture
    for bad in (mv_desc((0, 0, 0, 0), size, ALL, "int16", nch=0), mv_desc((0, 0, 0, 0), size, [0, 5], "int16"),
                mv_desc((0, 0, 0, 0), size, ALL, 0), mv_desc((0, 0, 0, 0), (0, 13), ALL, "int16"),
                mv_desc((0, 0, 0, 0), (9, 16385), ALL, "int16"), mv_desc((0, 0, 0, 0), size, ALL, "int16", filt=1),
                mv_desc((0, 0, 0, 0), (1, 1), ALL, "int16"),              # the crop window is more than 32 a side
                mv_desc((0, 0, 97, 1), size, ALL, "int16"), mv_desc((0, 0, 4, 0), size, ALL, "int16")):
        assert RESIZED(inst, C.byref(bad), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert RESIZED(inst, None, dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert RESIZED(inst, C.byref(crop), None, cur) == _lib.H264SWDEC_PARAM_ERR
    assert RESIZED(inst, C.byref(crop), dst.data_ptr() + 1, cur) == _lib.H264SWDEC_PARAM_ERR
    host = np.zeros(n, dtype=np.uint8)
    assert RESIZED(inst, C.byref(crop), host.ctypes.data, cur) == _lib.H264SWDEC_PARAM_ERR      # d_dst off the device
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all() and not host.any()   # nothing was queued
    assert RESIZED(inst, C.byref(crop), dst.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(crop.f), full.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    torch.cuda.synchronize()
    info = _lib.H264SwDecInfo()
    assert L.H264SwDecGetInfo(inst, C.byref(info)) == _lib.H264SWDEC_OK and info.croppingFlag
    cw, ch = info.cropParams.cropOutWidth, info.cropParams.cropOutHeight
    f = np.frombuffer(full.cpu().numpy()[:5 * cw * ch * 2].tobytes(), dtype=np.int16).reshape(5, ch, cw).astype(np.int64)
    assert (f[0] != 0).any()
    got = dst.cpu().numpy()
    assert same(got[:n], F.expect(f, size, "int16")) and (got[n:] == SENTINEL).all()
    L.H264SwDecRelease(inst)
