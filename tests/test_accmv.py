"""Accumulated motion as device tensors (accmv.hip): origin maps -- every luma
sample traced back to its position in the key picture of its GOP -- stepped per
picture (h264mi_accmv_step_device), exported as planar channels
(h264mi_accmv_device), kept per frame slot by the engine
(h264mi_engine_keep_accmv / _export_accmv, Engine.keep_accmv / to_accmv) and
delivered with each picture (H264SwDecKeepAccMotion /
H264SwDecLastPictureAccMotion, Decoder's ``accmv`` option).

The oracle (tests/_accmv.py) restates the field definition of include/h264mi.h
in numpy over the raw record bytes.  Every comparison is exact equality of
bytes."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _accmv as A
import _mbinfo as M
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 32                    # pictures per export launch (ACCMV_MAX_PICS)
TILE_MBS = 16               # MBs of a row per step workgroup (ACCMV_TILE_MBS)
MAX_SLOTS = 32              # H264MI_ACCMV_MAX_SLOTS
STREAM_SHA256 = "9cebfabe58154b0e80fb1277b2af7ad4c637be22564f4ab33997a6c3d75dcc48"
SENTINEL = 0xA5
PAGE = 4096
ALL = list(range(5))


def case_stream():
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
    """(Capture, the oracle chain after the whole stream, per picture its map) of the stream"""
    from broadway_amd.engine import Capture
    cap = Capture(case_stream())
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs, cap.npics) == (6, 4, 10)
    chain = A.Chain(cap.w_mbs, cap.h_mbs, cap.nslots)
    maps = [chain.decode(cap.records_bytes(i), cap.pictures[i].cur_slot) for i in range(cap.npics)]
    for m in maps:
        m.setflags(write=False)
    return cap, chain, maps


def small_motion_records(rng, w, h, nslots_hint=8):
    """_mbinfo.synthetic_records (types {0..4, 255}, arbitrary ref bytes, the
    extreme vectors in the first two records) with, for three records in four,
    vectors that stay near the picture and ref bytes below `nslots_hint`: the
    raw ones nearly always clamp to a corner and name no slot.  From three MBs
    on, the third is an inter record of slot 0 whose first and fifth blocks
    read row pieces with the picture's left and right edge inside them."""
    r = np.frombuffer(M.synthetic_records(rng, w, h), dtype=M.MBREC).copy()
    n = w * h
    near = rng.random(n) < 0.75
    near[:2] = False
    reach = (4 * 6 * w, 4 * 6 * h)                  # quarter-pels: up to 3 / 8 of the picture away on each axis
    mv = np.stack([rng.integers(-a, a + 1, (n, 16)) for a in reach], axis=-1).astype(np.int16)
    ref = rng.integers(0, nslots_hint, (n, 4)).astype(np.uint8)
    r["mv"][near] = mv[near]
    r["ref"][near] = ref[near]
    if n > 2:
        W, mbx = 16 * w, 16 * (2 % w)
        r["type"][2] = M.MBT_INTER
        r["ref"][2] = 0
        r["mv"][2, 0, 0] = 4 * (-2 - mbx)                   # block 0, column 0 of the MB: source columns -2 .. 1
        r["mv"][2, 4, 0] = 4 * (W - 2 - (mbx + 8)) + 1      # block 4, column 8: W - 2 .. W + 1 (+ 1 quarter-pel rounds away)
    return r.tobytes()


def random_map(rng, w, h):
    """random in-range coordinates and random ANCHORED bits (bit 15 zero)"""
    W, H = 16 * w, 16 * h
    return (rng.integers(0, W, (H, W)).astype(np.uint32) | rng.integers(0, H, (H, W)).astype(np.uint32) << np.uint32(16) |
            rng.integers(0, 2, (H, W)).astype(np.uint32) << np.uint32(31))


# ------------------------------------------------------------------ CPU ----
def test_oracle_key_step_is_the_identity_and_anchored():
    m = A.step(b"", 3, 2, [], key=True)
    f = A.channels(m)
    Y, X = np.mgrid[0:32, 0:48]
    assert m.dtype == np.uint32 and m.shape == (32, 48)
    assert (f[0] == 0).all() and (f[1] == 0).all() and (f[2] == X).all() and (f[3] == Y).all() and (f[4] == 1).all()
    assert (m & 0x8000).max() == 0                                      # bit 15 stays clear
    assert A.is_key(np.zeros(6, dtype=M.MBREC).tobytes()) is False      # type 0 is MBT_INTER
    r = np.zeros(6, dtype=M.MBREC)
    r["type"] = [2, 3, 4, 255, 2, 3]
    assert A.is_key(r.tobytes())


def test_oracle_one_hop_from_a_key_map_is_the_rounded_vector():
    """ADX == (MVX + 2) >> 2 and ADY likewise, exactly, where the clamp does not
    bite; anchored there; intra samples (0, 0, unanchored)."""
    rng = np.random.default_rng(5)
    w, h = 5, 3
    rec = small_motion_records(rng, w, h)
    W, H = 16 * w, 16 * h
    key = A.identity(w, h, 1)
    refs = [key] * 256                                                  # whatever the ref byte says
    f = A.channels(A.step(rec, w, h, refs))
    mvx, mvy, mbt = (np.repeat(np.repeat(M.field(rec, w, h)[c], 4, axis=0), 4, axis=1) for c in (0, 1, 4))
    Y, X = np.mgrid[0:H, 0:W]
    dx, dy = (mvx + 2) >> 2, (mvy + 2) >> 2
    inter = (mbt == M.MBT_INTER) | (mbt == M.MBT_SKIP)
    free = inter & (X + dx >= 0) & (X + dx < W) & (Y + dy >= 0) & (Y + dy < H)
    assert 0.05 < free.mean() < 0.9 and 0.05 < (inter & ~free).mean()  # both kinds are there
    assert (f[0][free] == dx[free]).all() and (f[1][free] == dy[free]).all()
    assert (f[4][inter] == 1).all()
    assert (f[2][inter & ~free] == np.clip(X + dx, 0, W - 1)[inter & ~free]).all()
    assert (f[0][~inter] == 0).all() and (f[1][~inter] == 0).all() and (f[4][~inter] == 0).all()
    assert (np.array([-3, -2, -1, 0, 1, 2, 3, 5, 6, -6, -7]) + 2 >> 2).tolist() == [-1, 0, 0, 0, 0, 1, 1, 1, 2, -1, -2]


def test_oracle_two_steps_equal_a_per_sample_trace():
    """key -> P1 -> P2 over three slots, one of them without a map: the
    vectorised step twice against a trace followed sample by sample."""
    rng = np.random.default_rng(11)
    w, h, nslots = 3, 2, 3
    recs = [small_motion_records(rng, w, h, nslots_hint=4) for _ in range(2)]
    m0 = A.step(b"", w, h, [], key=True)                                # slot 0
    m1 = A.step(recs[0], w, h, [m0, None, None])                        # slot 1, reads slot 0
    m2 = A.step(recs[1], w, h, [m0, m1, None])                          # slot 2, reads slots 0 and 1
    pics = [(None, True, {}), (np.frombuffer(recs[0], dtype=M.MBREC), False, {0: 0}),
            (np.frombuffer(recs[1], dtype=M.MBREC), False, {0: 0, 1: 1})]
    f = A.channels(m2)
    for y in range(16 * h):
        for x in range(16 * w):
            jx, jy, an = A.trace(x, y, 2, pics, w, h)
            assert (f[2][y, x], f[3][y, x], f[4][y, x]) == (jx, jy, an), (x, y)
    r2 = np.frombuffer(recs[1], dtype=M.MBREC)
    two_hops = ((r2["type"] <= 1)[:, None] & (r2["ref"] == 1)).sum()
    assert two_hops > 0 and 0 < f[4].mean() < 1


ACCMV_GRID = {
    "whole": "accept", "flush_right_bottom": "accept", "right_plus_1": "refuse", "right_plus_1_by_origin": "refuse",
    "bottom_plus_1": "refuse", "bottom_plus_1_by_origin": "refuse", "origin_0": "accept", "odd_window": "accept",
    "last_sample": "accept", "x_negative": "refuse", "y_negative": "refuse", "cw_0": "refuse", "ch_0": "refuse",
    "cw_negative": "refuse", "ch_negative": "refuse",
    "dtype_u8": "refuse", "dtype_f16": "accept", "dtype_bf16": "accept", "dtype_f32": "accept", "dtype_5": "refuse",
    "dtype_minus_1": "refuse",
    "nch_0": "refuse", "nch_1": "accept", "nch_8": "accept", "nch_9": "refuse", "nch_negative": "refuse",
    "channel_minus_1": "refuse", "channel_4": "accept", "channel_5": "refuse", "channel_5_at_8": "refuse",
    "wide_2048_mbs": "accept", "wide_2049_mbs": "refuse", "tall_2048_mbs": "accept", "tall_2049_mbs": "refuse",
}


def test_descriptor_rules(tmp_path):
    """common/export_desc.h's accmv rules walked by tests/accmv_desc_check.c
    under AddressSanitizer + UBSan, as tests/test_export_desc.py walks the
    others; the expected column is written out from include/h264mi.h: x, y >= 0,
    cw, ch >= 1, inside 96 x 64 (odd allowed); 1 <= nch <= 8, channel ids 0 ..
    4; F16, BF16, F32 or I16; at most 2048 MBs each way."""
    exe = str(tmp_path / "accmv_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "accmv_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    got = {}
    for ln in p.stdout.splitlines():
        f = ln.split()
        if f[0] == "accmv":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(ACCMV_GRID)
    assert {k: v for k, v in got.items() if v != ACCMV_GRID[k]} == {}
    assert "size 1 0 0 0 0" in p.stdout.splitlines()


def test_library_exports_the_accmv_entry_points():
    from broadway_amd import _lib
    L = _lib.mi()           # (first: it loads torch's HIP runtime before the library binds to one)
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    for name, nargs in (("h264mi_accmv_step_device", 8), ("h264mi_accmv_device", 9), ("h264mi_engine_keep_accmv", 2),
                        ("h264mi_engine_export_accmv", 8), ("H264SwDecKeepAccMotion", 2),
                        ("H264SwDecLastPictureAccMotion", 4)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int x, y, cw, ch, nch, dtype; int id[8]; float scale[8], bias[8]; }
    D = _lib.AccMvDesc
    assert C.sizeof(D) == 6 * 4 + 3 * 8 * 4
    assert [getattr(D, n).offset for n in ("x", "y", "cw", "ch", "nch", "dtype")] == [0, 4, 8, 12, 16, 20]
    assert (D.id.offset, D.scale.offset, D.bias.offset) == (24, 56, 88)
    assert _lib.ACCMV_MAX_CH == 8 and [_lib.ACCMV_CHANNELS[n] for n in A.CHANNELS] == list(range(5))


def test_decoder_option_validation():
    with pytest.raises(ValueError):
        Decoder({"accmv": {"window": (0, 0, 4, 4)}})            # the window is the crop window
    with pytest.raises(ValueError):
        Decoder({"accmv": {"channel": ("adx",)}})
    with pytest.raises(ValueError):
        Decoder({"accmv": {"channels": ("adx", "adz")}})
    with pytest.raises(ValueError):
        Decoder({"accmv": {"channels": ()}})
    with pytest.raises(ValueError):
        Decoder({"accmv": {"dtype": np.int16}})
    with pytest.raises(ValueError):
        Decoder({"accmv": {"channels": ("adx", "ady"), "scale": (1.0, 2.0, 3.0)}})
    with pytest.raises(ValueError):                             # checked whatever the output mode
        Decoder({"accmv": {"channels": ("nope",)}, "rgb": True, "crop": True})


def test_accmv_desc_arguments():
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import accmv_desc
    d, n, dt = accmv_desc(("jy", "adx", "jy"), (1, 2, 3, 5), torch.float16, scale=0.25, bias=(0.0, 1.0, 2.0))
    assert (n, dt) == (3, torch.float16) and (d.x, d.y, d.cw, d.ch, d.nch, d.dtype) == (1, 2, 3, 5, 3, _lib.TENSOR_F16)
    assert list(d.id)[:3] == [3, 0, 3] and list(d.scale)[:3] == [0.25] * 3 and list(d.bias)[:3] == [0.0, 1.0, 2.0]
    d, n, dt = accmv_desc()
    assert (n, dt, d.cw, d.ch, d.dtype) == (2, torch.int16, 0, 0, _lib.TENSOR_I16) and list(d.id)[:2] == [0, 1]
    assert d.scale[0] == 1.0 and d.bias[1] == 0.0
    assert accmv_desc("anchored")[0].id[0] == 4 and accmv_desc(A.CHANNELS)[1] == 5
    for kw in (dict(channels=()), dict(channels=("adx",) * 9), dict(channels=("ADX",)), dict(channels=(0,)),
               dict(channels=("adx",), dtype=torch.uint8), dict(channels=("adx",), dtype=torch.int32),
               dict(channels=("adx", "ady"), scale=(1.0,)), dict(channels=("adx",), bias=(1.0, 2.0)),
               dict(channels=("adx",), window=(0, 0, 4)), dict(channels=("adx",), window=(0, 0, 0, 4)),
               dict(channels=("adx",), window=(-1, 0, 4, 4))):
        with pytest.raises(ValueError):
            accmv_desc(**kw)


def test_the_stream_exercises_the_field(captured):
    """What the engine and decoder tests below rely on, from the captured
    records: they cannot pass on an empty field."""
    cap, chain, maps = captured
    st = chain.stats
    assert sum(s["key"] for s in st) >= 2                               # at least 2 key pictures
    assert max(len(s["slots"]) for s in st) >= 3                        # some picture reading at least 3 slots
    assert max(s["clamped"] for s in st) >= 0.10                        # at least 10 % clamped samples
    assert any(0.02 <= s["unanchored"] <= 0.50 for s in st)             # an unanchored share between 2 % and 50 %
    assert max(s["max_hops"] for s in st) >= 4                          # some chain of at least 4 hops
    slots = [p.cur_slot for p in cap.pictures]
    keys = [k for k, s in enumerate(st) if s["key"]]
    assert slots[keys[0]] == slots[keys[1]]                             # the second key overwrites the first one's slot
    assert len(set(slots)) == cap.nslots                                # and every slot goes stale at the second key


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


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


STEP_SIZES = {"1x1": (1, 1), "3x2": (3, 2), "5x3": (5, 3), "9x2": (9, 2), "17x2": (TILE_MBS + 1, 2)}
NSLOTS = 6                  # slots 1 and 4 have no map; small_motion_records names slots 0..7 and arbitrary bytes


def run_step(rec, w, h, refs, key=0, nslots=None, null=(), dims=None, alias=False, rec_skew=0, out_skew=0, ref_skew=0):
    """h264mi_accmv_step_device over one record batch and the maps `refs` (None:
    no map).  Every buffer lies in one device allocation between sentinel
    pages.  Returns rc, the output map, whether every sentinel byte and every
    reference map is unchanged, and whether the output still is all sentinel."""
    import torch
    L = _mi()
    nw = 256 * w * h
    recs = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(96 * w * h, dtype=np.uint8)
    rec_room = (recs.size + PAGE - 1) // PAGE * PAGE
    map_room = (4 * nw + PAGE - 1) // PAGE * PAGE + PAGE               # a map, the rest of its page, a sentinel page
    host = np.full(PAGE + rec_room + PAGE + map_room * (len(refs) + 1), SENTINEL, dtype=np.uint8)
    host[PAGE:PAGE + recs.size] = recs
    base = PAGE + rec_room + PAGE
    offs = [base + k * map_room for k in range(len(refs) + 1)]          # the references, then the output
    for k, m in enumerate(refs):
        if m is not None:
            host[offs[k]:offs[k] + 4 * nw] = m.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).to("cuda")
    assert dev.data_ptr() % 16 == 0
    ptrs = (C.c_void_p * max(len(refs), 1))(*[None if m is None else dev.data_ptr() + offs[k] + ref_skew
                                               for k, m in enumerate(refs)])
    out_ptr = dev.data_ptr() + offs[-1] + out_skew
    if alias:
        ptrs[0] = out_ptr
    wm, hm = dims or (w, h)
    rc = L.h264mi_accmv_step_device(None if "rec" in null else dev.data_ptr() + PAGE + rec_skew, wm, hm,
                                    None if "refs" in null else ptrs, len(refs) if nslots is None else nslots, key,
                                    None if "out" in null else out_ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    out = got[offs[-1]:offs[-1] + 4 * nw].copy()
    untouched = not out.view(np.uint8).tobytes().strip(bytes([SENTINEL]))
    got[offs[-1]:offs[-1] + 4 * nw] = host[offs[-1]:offs[-1] + 4 * nw]
    return rc, out.view(np.uint32).reshape(16 * h, 16 * w), np.array_equal(got, host), untouched


@pytest.fixture(scope="module")
def step_cases():
    """size -> (record batch, NSLOTS reference maps with two of them None) (read-only)"""
    rng = np.random.default_rng(41)
    out = {}
    for name, (w, h) in STEP_SIZES.items():
        rec = small_motion_records(rng, w, h)
        refs = [None if s in (1, 4) else random_map(rng, w, h) for s in range(NSLOTS)]
        for m in refs:
            if m is not None:
                m.setflags(write=False)
        out[name] = (rec, refs)
    return out


def test_step_cases_cover_the_rules(step_cases):
    """Every size but the one-MB one has samples through a map, samples whose
    slot has none or lies beyond nslots, intra samples, row pieces the clamp
    cuts on the left and on the right, and the extreme vectors."""
    for name, (w, h) in STEP_SIZES.items():
        rec, refs = step_cases[name]
        r = np.frombuffer(rec, dtype=M.MBREC)
        assert r["mv"].min() == -32768 and r["mv"].max() == 32767, name
        if name == "1x1":
            continue
        inter = r["type"] <= 1
        ref = r["ref"][inter]
        assert inter.any() and (~inter).any(), name
        assert np.isin(ref, [0, 2, 3, 5]).any() and np.isin(ref, [1, 4]).any() and (ref >= NSLOTS).any(), name
        st = {}
        A.step(rec, w, h, refs, stats=st)
        assert 0.05 < st["clamped"] < 0.95, name
        # a row piece's first source column: its MB's and its z-scan block's column plus the rounded vector
        W = 16 * w
        d = (r["mv"][:, :, 0].astype(np.int64) + 2) >> 2
        x0 = (np.arange(w * h) % w * 16)[:, None] + np.array([0, 4, 0, 4, 8, 12, 8, 12] * 2)[None, :] + d
        mapped = (inter[:, None] & np.isin(r["ref"], [0, 2, 3, 5]))[:, np.arange(16) >> 2]
        assert (mapped & (x0 < 0) & (x0 + 3 >= 0)).any(), name         # the left edge inside a piece read through a map
        assert (mapped & (x0 <= W - 1) & (x0 + 3 > W - 1)).any(), name  # and the right edge


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(STEP_SIZES))
def test_step_kernel_vs_oracle(step_cases, size):
    """The step over synthetic batches: byte for byte the oracle's map, nothing
    written outside it, the references unchanged; with nslots cut down the
    slots beyond it count as none; with the key flag the identity."""
    w, h = STEP_SIZES[size]
    rec, refs = step_cases[size]
    for nslots in (NSLOTS, 3, 0):
        rc, out, clean, _ = run_step(rec, w, h, refs[:nslots])
        assert rc == 0, nslots
        assert same(out, A.step(rec, w, h, refs[:nslots])), nslots
        assert clean, nslots
    none = [None] * MAX_SLOTS                                           # the most slots, none with a map
    rc, out, clean, _ = run_step(rec, w, h, none)
    assert rc == 0 and same(out, A.step(rec, w, h, none)) and clean
    for r, nslots in ((refs, NSLOTS), ([], 0)):
        rc, out, clean, _ = run_step(rec, w, h, r, key=1, null=() if r else ("refs",))
        assert rc == 0 and same(out, A.identity(w, h, 1)) and clean, nslots


@pytest.mark.gpu
def test_step_kernel_rejects_bad_arguments(step_cases):
    w, h = STEP_SIZES["3x2"]
    rec, refs = step_cases["3x2"]

    def refused(**kw):
        r = kw.pop("refs", refs)
        rc, _, clean, untouched = run_step(rec, w, h, r, **kw)
        assert rc == -1 and clean and untouched, kw                     # nothing was launched

    rc, _, clean, untouched = run_step(rec, w, h, refs)
    assert rc == 0 and clean and not untouched                          # the arguments below are one step away
    for null in ("rec", "out", "refs"):
        refused(null=(null,))
    refused(dims=(0, h))
    refused(dims=(w, 0))
    refused(dims=(2049, h))                                             # beyond 32768 samples
    refused(dims=(w, 2049))
    refused(nslots=-1)
    refused(refs=[None] * (MAX_SLOTS + 1))
    refused(alias=True)                                                 # a reference map that is the output
    refused(rec_skew=4)
    refused(out_skew=4)
    refused(ref_skew=2)


DTYPES = M.DTYPES
EXPORT_DIMS = (3, 2)        # MBs: 48 x 32 samples
CHANNEL_LISTS = [[c] for c in ALL] + [ALL[::-1], [0, 1, 0, 4, 4, 2], [3] * 8]


def export_windows(W, H):
    """The whole picture, one sample, the last one, odd offsets and sizes off
    the MB and 4x4 grids, one whose row bytes are a multiple of 16 for every
    element type (8 columns) and one for none (7 columns)."""
    return [(0, 0, W, H), (5, 3, 1, 1), (W - 1, H - 1, 1, 1), (3, 1, W - 5, H - 3), (1, 1, 8, H - 2), (17, 5, 7, 13),
            (2, 0, 16, 3)]


@pytest.fixture(scope="module")
def export_maps():
    """3 random maps and their channels (read-only)"""
    rng = np.random.default_rng(43)
    maps = [random_map(rng, *EXPORT_DIMS) for _ in range(3)]
    chans = [A.channels(m) for m in maps]
    for a in maps + chans:
        a.setflags(write=False)
    f = np.stack(chans)
    assert f[:, 0].min() < -20 and f[:, 0].max() > 20 and set(np.unique(f[:, 4]).tolist()) == {0, 1}
    return maps, chans


def make_desc(win, ids, dtype, consts="unit", nch=None):
    from broadway_amd import _lib
    d = _lib.AccMvDesc()
    d.x, d.y, d.cw, d.ch = win
    d.nch = len(ids) if nch is None else nch
    d.dtype = M.DTYPE_ID.get(dtype, dtype)
    d.id[:len(ids)] = ids
    scale, bias = M.CONSTS[consts]
    d.scale[:] = scale[:8]
    d.bias[:] = bias[:8]
    return d


def expect(f, ids, win, dtype, consts="unit"):
    scale, bias = M.CONSTS[consts]
    return M.convert(A.select(f, ids, win), dtype, scale, bias)


FRONT = 64


def run_export(maps, order, win, ids, dtype, consts="unit", in_pad=0, out_pad=0, skew=0, nch=None, npics=None, null=(),
               stride=None, offs=None, in_skew=0, dims=None):
    """h264mi_accmv_device over the maps `order` of `maps`; returns rc, the
    whole output buffer (FRONT + skew sentinel bytes, then pictures out_stride
    apart, then 64 sentinel bytes), the first picture's offset, out_stride and
    a picture's bytes."""
    import torch
    L = _mi()
    w, h = EXPORT_DIMS
    es = M.ELEM.get(dtype, 2)
    nbytes = max(len(ids), 1) * win[2] * win[3] * es if win[2] > 0 and win[3] > 0 else 16
    in_stride = maps[0].nbytes + in_pad
    out_stride = nbytes + out_pad if stride is None else stride
    host = np.full(in_stride * len(maps) + 64, SENTINEL, dtype=np.uint8)
    for k, m in enumerate(maps):
        host[k * in_stride:k * in_stride + m.nbytes] = m.reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host).to("cuda")
    n = len(order)
    offs = (C.c_size_t * n)(*([k * in_stride for k in order] if offs is None else offs))
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    desc = make_desc(win, ids, dtype, consts, nch)
    wm, hm = dims or (w, h)
    rc = L.h264mi_accmv_device(None if "in" in null else d_in.data_ptr() + in_skew, None if "offs" in null else offs,
                               n if npics is None else npics, wm, hm, None if "desc" in null else C.byref(desc),
                               None if "out" in null else d_out.data_ptr() + first, out_stride,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


def consts_of(dtype):
    return ["unit"] if dtype == "int16" else ["unit", "mixed"]          # int16 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_export_kernel_vs_oracle(export_maps, dtype):
    """All five channels over every window with both constant sets, then the
    channel lists (each id alone, reversed, repeats, one of 8 entries: the
    constants go with the channel position, not the id)."""
    maps, chans = export_maps
    W, H = 16 * EXPORT_DIMS[0], 16 * EXPORT_DIMS[1]
    cases = [(win, ALL, c) for win in export_windows(W, H) for c in consts_of(dtype)]
    cases += [(win, ids, "mixed") for ids in CHANNEL_LISTS for win in ((0, 0, W, H), (3, 1, W - 5, H - 3))]
    for win, ids, consts in cases:
        rc, out, first, stride, nbytes = run_export(maps[:1], [0], win, ids, dtype, consts)
        assert rc == 0, (win, ids, consts)
        assert same(out[first:first + nbytes], expect(chans[0], ids, win, dtype, consts)), (win, ids, consts)
        assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (win, ids, consts)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_export_kernel_batched_padded_strides_write_nothing_else(export_maps, dtype):
    """Picture list [2, 0, 2, 1] of three maps 64 pad bytes apart; out_stride
    padded by 5 elements (never a multiple of 16 bytes: the element path), by
    48 bytes (16-byte rows keep the 16-byte stores) and by 48 bytes with d_out
    one element past a 16-byte boundary (the element path again): every
    picture is right and no pad byte changes."""
    maps, chans = export_maps
    W, H = 16 * EXPORT_DIMS[0], 16 * EXPORT_DIMS[1]
    es = M.ELEM[dtype]
    order = [2, 0, 2, 1]
    ids = [0, 1, 4]
    for win in [(0, 0, W, H), (1, 1, 8, H - 2), (3, 1, W - 5, H - 3)]:
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_export(maps, order, win, ids, dtype, "mixed", in_pad=64, out_pad=out_pad,
                                                        skew=skew)
            assert rc == 0, (win, out_pad, skew)
            assert (out[:first] == SENTINEL).all(), (win, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                assert same(out[o:o + nbytes], expect(chans[i], ids, win, dtype, "mixed")), (win, out_pad, skew, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (win, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (win, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_export_kernel_list_longer_than_one_launch(export_maps, dtype):
    maps, chans = export_maps
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win = (3, 2, 16, 5)
    rc, out, first, stride, nbytes = run_export(maps, order, win, [1, 2], dtype, "mixed", in_pad=64)
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], expect(chans[i], [1, 2], win, dtype, "mixed")), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
def test_export_kernel_rejects_bad_arguments(export_maps):
    maps, _ = export_maps
    good = (1, 1, 4, 4)

    def refused(**kw):
        args = dict(win=good, ids=[0, 1], dtype="float16")
        args.update(kw)
        win, ids, dtype = args.pop("win"), args.pop("ids"), args.pop("dtype")
        rc, out, *_ = run_export(maps[:1], [0], win, ids, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    rc, out, first, _, nbytes = run_export(maps[:1], [0], good, [0, 1], "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    for nch in (0, 9, -1):
        refused(nch=nch)
    for bad in (5, -1, 255):
        refused(ids=[0, bad])
    for dtype in (0, 5, -1):                             # uint8 and unknown types
        refused(dtype=dtype)
    for win in ((0, 0, 49, 8), (0, 0, 48, 33), (48, 0, 1, 1), (0, 32, 1, 1), (45, 0, 4, 1), (0, 30, 1, 3), (-1, 0, 4, 4),
                (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -4, 4)):
        refused(win=win)
    for null in ("in", "offs", "desc", "out"):
        refused(null=(null,))
    refused(npics=0)
    refused(npics=-1)
    refused(dims=(0, 2))
    refused(dims=(3, 0))
    refused(dims=(2049, 2))
    for dtype, skew in (("int16", 1), ("float16", 1), ("bfloat16", 1), ("float32", 2)):
        refused(dtype=dtype, skew=skew)                  # d_out not a multiple of the element size
    refused(dtype="float16", stride=2 * 4 * 4 * 2 + 1)   # nor out_stride
    refused(dtype="float32", stride=2 * 4 * 4 * 4 + 2)
    refused(offs=[2])                                    # not a multiple of 4
    refused(in_skew=2)


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


def engine_maps(eng, stream, nslots, W, H):
    """the maps of every slot of `stream`, from the jx, jy and anchored channels"""
    import torch
    t = eng.to_accmv([stream] * nslots, list(range(nslots)), channels=("jx", "jy", "anchored"))
    torch.cuda.synchronize()
    assert tuple(t.shape) == (nslots, 3, H, W) and t.dtype == torch.int16
    v = t.cpu().numpy().astype(np.int64)
    return [A.pack(v[s, 0], v[s, 1], 0) | (v[s, 2].astype(np.uint32) << np.uint32(31)) for s in range(nslots)]


@pytest.mark.gpu
def test_engine_keeps_origin_maps_per_slot(captured):
    """Picture by picture with retention on: after each one every slot matches
    the oracle chain under the serial rule (a slot last written before the
    current key stays exportable, and later pictures that name it start
    unanchored there); retention changes no pixel; forgetting, bad arguments,
    off and on again."""
    import torch
    from broadway_amd.engine import Engine
    cap, chain_all, maps = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    W, H = 16 * w, 16 * h
    plain = Engine(w, h, 1, ns)
    for pic in cap.pictures:
        plain.decode([0], [pic])
    want_pixels = [plain.read(0, s).tobytes() for s in range(ns)]
    with pytest.raises(RuntimeError):
        plain.to_accmv([0], [0])                        # retention is off
    plain.close()

    eng = Engine(w, h, 1, ns)
    eng.keep_accmv()
    chain = A.Chain(w, h, ns)
    stale_seen = False
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        chain.decode(cap.records_bytes(k), pic.cur_slot)
        got = engine_maps(eng, 0, ns, W, H)
        for s in range(ns):
            assert same(got[s], chain.maps[s]), (k, s)
        stale_seen |= any(0 < chain.ser[s] < chain.key for s in range(ns))
        assert same(chain.maps[pic.cur_slot], maps[k]), k
    assert stale_seen and eng.errors() == 0
    assert [eng.read(0, s).tobytes() for s in range(ns)] == want_pixels
    # the export proper: dtypes, constants, a window off every grid, repeats
    last = cap.pictures[-1].cur_slot
    f = A.channels(chain.maps[last])
    win = (7, 3, 57, 41)
    for dtype, consts, ids in (("int16", "unit", [0, 1]), ("float16", "mixed", [4, 0, 0, 3]), ("float32", "mixed", ALL),
                               ("bfloat16", "unit", [2])):
        scale, bias = M.CONSTS[consts]
        t = eng.to_accmv([0], [last], channels=[A.CHANNELS[i] for i in ids], window=win, dtype=getattr(torch, dtype),
                         scale=scale[:len(ids)], bias=bias[:len(ids)])
        torch.cuda.synchronize()
        assert tuple(t.shape) == (1, len(ids), win[3], win[2])
        assert same(tensor_bytes(t), expect(f, ids, win, dtype, consts)), dtype
    # forgetting a slot the rest of a GOP reads: (x, y, 0) there, unanchored starts in a later picture
    eng.keep_accmv(False)
    with pytest.raises(RuntimeError):
        eng.to_accmv([0], [0])
    with pytest.raises(RuntimeError):
        eng.forget_records(0, 0)                        # nothing is kept
    eng.keep_accmv(True)
    chain = A.Chain(w, h, ns)                           # off then on starts from nothing
    for s, m in enumerate(engine_maps(eng, 0, ns, W, H)):
        assert same(m, A.identity(w, h, 0)), s
    keyslot = cap.pictures[0].cur_slot
    for k, pic in enumerate(cap.pictures[:5]):
        if k == 2:
            eng.forget_records(0, keyslot)
            chain.forget(keyslot)
        eng.decode([0], [pic])
        chain.decode(cap.records_bytes(k), pic.cur_slot)
    got = engine_maps(eng, 0, ns, W, H)
    for s in range(ns):
        assert same(got[s], chain.maps[s]), s
    assert same(got[keyslot], A.identity(w, h, 0))
    assert chain.stats[4]["unanchored"] > chain_all.stats[4]["unanchored"]
    for kw in (dict(streams=[1], slots=[0]), dict(streams=[0], slots=[ns]),
               dict(streams=[0], slots=[0], window=(0, 0, W + 1, 1))):
        with pytest.raises(RuntimeError):
            eng.to_accmv(**kw)
    with pytest.raises(RuntimeError):
        eng.forget_records(0, ns)
    eng.close()


@pytest.mark.gpu
def test_engine_two_streams_at_different_phases_do_not_mix(captured):
    """Stream 1 runs three pictures behind stream 0 in one engine, so batches
    hold a key picture of one and a P picture of the other."""
    import torch
    from broadway_amd.engine import Engine
    cap, _, maps = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    eng = Engine(w, h, 2, ns)
    eng.keep_accmv()
    chains = [A.Chain(w, h, ns), A.Chain(w, h, ns)]
    lag = 3
    for k in range(cap.npics + lag):
        streams = [s for s, i in ((0, k), (1, k - lag)) if 0 <= i < cap.npics]
        idx = [i for i in (k, k - lag) if 0 <= i < cap.npics]
        eng.decode(streams, [cap.pictures[i] for i in idx])
        for s, i in zip(streams, idx):
            chains[s].decode(cap.records_bytes(i), cap.pictures[i].cur_slot)
        if k in (4, 6, cap.npics + lag - 1):
            for s in (0, 1):
                got = engine_maps(eng, s, ns, 16 * w, 16 * h)
                for slot in range(ns):
                    assert same(got[slot], chains[s].maps[slot]), (k, s, slot)
    torch.cuda.synchronize()
    assert eng.errors() == 0
    eng.close()


@pytest.mark.gpu
def test_engine_export_is_ordered_against_the_next_decode_into_the_slot(captured):
    """Export into ``out``, then decode the next picture into the same slot
    with no synchronisation in between: ``out`` holds the earlier map."""
    import torch
    from broadway_amd.engine import Engine
    cap, _, maps = captured
    slots = [p.cur_slot for p in cap.pictures]
    k1 = next(k for k in range(2, cap.npics) if slots[k] in slots[1:k])     # the first decode over a P picture's slot
    k0 = slots.index(slots[k1], 1)
    w, h = cap.w_mbs, cap.h_mbs
    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_accmv()
    out = torch.empty((1, 5, 16 * h, 16 * w), dtype=torch.int16, device="cuda")
    for k in range(k1):
        eng.decode([0], [cap.pictures[k]])
    assert eng.to_accmv([0], [slots[k0]], channels=A.CHANNELS, out=out) is out
    eng.decode([0], [cap.pictures[k1]])
    after = eng.to_accmv([0], [slots[k1]], channels=A.CHANNELS)
    torch.cuda.synchronize()
    whole = (0, 0, 16 * w, 16 * h)
    assert same(tensor_bytes(out), expect(A.channels(maps[k0]), ALL, whole, "int16"))
    assert same(tensor_bytes(after), expect(A.channels(maps[k1]), ALL, whole, "int16"))
    assert not np.array_equal(tensor_bytes(out), tensor_bytes(after))
    eng.close()


def decode_js(nals, opts):
    """(pictures, their accmv tensors, crop window per picture) of a Decoder run"""
    got, infos, wins = [], [], []
    dec = Decoder(opts)

    def on_picture(buf, w, h, _):
        got.append(bytes(buf) if isinstance(buf, np.ndarray) else buf)
        infos.append(dec.accmv)
        wins.append(tuple(dec._crop_window()))

    dec.onPictureDecoded = on_picture
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, infos, wins


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "tensor", "crop_rgb"])
def test_decoder_accmv_option(captured, mode):
    """decoder.accmv, set before each onPictureDecoded call, is the oracle's
    accumulated motion of that picture over the crop window (this stream's
    output order is its decode order), whatever the output mode; and the pixels
    are those of the same run without ``accmv``."""
    import torch
    cap, _, maps = captured
    nals = split_annexb(case_stream())
    base = {"plain": {}, "tensor": {"tensor": True}, "crop_rgb": {"crop": True, "rgb": True}}[mode]
    want, none, _ = decode_js(nals, base)
    assert none == [None] * len(want)
    got, infos, wins = decode_js(nals, dict(base, accmv=True))
    all5, infos5, _ = decode_js(nals, dict(base, accmv={"channels": A.CHANNELS, "dtype": torch.float32,
                                                        "scale": M.CONSTS["mixed"][0][:5],
                                                        "bias": M.CONSTS["mixed"][1][:5]}))
    assert len(got) == len(want) == len(all5) == cap.npics
    for k in range(cap.npics):
        if mode == "tensor":
            assert torch.equal(got[k], want[k]) and torch.equal(all5[k], want[k]), k
        else:
            assert got[k] == want[k] and all5[k] == want[k], k
        x, y, cw, ch = win = wins[k]
        assert (cw, ch) != (16 * cap.w_mbs, 16 * cap.h_mbs)            # the stream is cropped
        f = A.channels(maps[k])
        t = infos[k]
        assert tuple(t.shape) == (2, ch, cw) and t.dtype == torch.int16 and t.is_cuda, k
        assert same(tensor_bytes(t), expect(f, [0, 1], win, "int16")), k
        t = infos5[k]
        assert tuple(t.shape) == (5, ch, cw) and t.dtype == torch.float32, k
        assert same(tensor_bytes(t), expect(f, ALL, win, "float32", "mixed")), k


@pytest.mark.gpu
def test_swdec_last_picture_accmotion_return_codes(captured):
    """H264SWDEC_OK before any picture; H264SWDEC_PARAM_ERR with retention
    never switched on and for what the export refuses; H264SWDEC_PIC_RDY and
    the field after a picture; a desc with its own window."""
    import torch
    from broadway_amd import _lib
    cap, _, maps = captured
    L = _mi()
    stream = case_stream()
    dst = torch.full((5 * 64 * 96 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    cur = torch.cuda.current_stream().cuda_stream

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

    whole = make_desc((0, 0, 0, 0), ALL, "int16")
    # retention never switched on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert pictures(inst, 1)
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    L.H264SwDecRelease(inst)
    # retention on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecKeepAccMotion(inst, 1) == _lib.H264SWDEC_OK
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_OK
    assert pictures(inst, 2)                            # the second picture: a P picture
    for bad in (make_desc((0, 0, 0, 0), ALL, "int16", nch=0), make_desc((0, 0, 0, 0), ALL, "int16", nch=9),
                make_desc((0, 0, 0, 0), [0, 5], "int16"), make_desc((0, 0, 0, 0), ALL, 0),
                make_desc((0, 0, 97, 1), ALL, "int16"), make_desc((0, 64, 1, 1), ALL, "int16"),
                make_desc((0, 0, 4, 0), ALL, "int16")):
        assert L.H264SwDecLastPictureAccMotion(inst, C.byref(bad), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureAccMotion(inst, None, dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(whole), None, cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(whole), dst.data_ptr() + 1, cur) == _lib.H264SWDEC_PARAM_ERR
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()                       # nothing was queued
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    win = (3, 2, 7, 5)
    own = make_desc(win, [1, 4], "float16", "mixed")
    dst2 = torch.full((2 * 7 * 5 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert L.H264SwDecLastPictureAccMotion(inst, C.byref(own), dst2.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    torch.cuda.synchronize()
    info = _lib.H264SwDecInfo()
    assert L.H264SwDecGetInfo(inst, C.byref(info)) == _lib.H264SWDEC_OK and info.croppingFlag
    cp = info.cropParams
    crop = (cp.cropLeftOffset, cp.cropTopOffset, cp.cropOutWidth, cp.cropOutHeight)
    f = A.channels(maps[1])
    assert (f[0] != 0).any() and 0 < f[4].mean() < 1
    n = 5 * crop[2] * crop[3] * 2
    got = dst.cpu().numpy()
    assert same(got[:n], expect(f, ALL, crop, "int16")) and (got[n:] == SENTINEL).all()
    got = dst2.cpu().numpy()
    assert same(got[:140], expect(f, [1, 4], win, "float16", "mixed")) and (got[140:] == SENTINEL).all()
    L.H264SwDecRelease(inst)
