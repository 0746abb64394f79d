"""The accumulated residual as device tensors (accres.hip): every sample of a
picture minus its origin in the key picture of its GOP, exported by the
stateless h264mi_accres_device, kept exportable by the engine's key store
(h264mi_engine_keep_accres / _accres_held / _export_accres, Engine.keep_accres /
accres_held / to_accres).

The oracle (tests/_accres.py) restates the field definition of include/h264mi.h
in numpy over frame bytes and map words.  Every comparison is exact equality of
bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _accmv as A
import _accres as R
import _colour as COL
import _mbinfo as M
from test_accmv import SENTINEL, case_stream, engine_maps, random_map, same, tensor_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 32                    # pictures per export launch (ACCRES_MAX_PICS)
NOKEY = (1 << 64) - 1       # (size_t)-1
SIZES = {"1x1": (1, 1), "3x2": (3, 2), "5x3": (5, 3), "17x1": (17, 1)}
ALL_PLANES = ["y", "uv", "yuv", "rgb"]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


@pytest.fixture(scope="module")
def captured():
    from broadway_amd.engine import Capture
    cap = Capture(case_stream())
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs, cap.npics) == (6, 4, 10)
    chain = A.Chain(cap.w_mbs, cap.h_mbs, cap.nslots)
    maps = [chain.decode(cap.records_bytes(i), cap.pictures[i].cur_slot) for i in range(cap.npics)]
    return cap, chain, maps


def random_frame(rng, w, h):
    """random samples, and random bytes in the chroma rows' padding"""
    f = rng.integers(0, 256, R.slot_bytes(w, h), dtype=np.uint8)
    f.setflags(write=False)
    return f


def near_motion_records(rng, w, h):
    """inter records of slot 0 whose blocks move by up to 3 samples each way
    (quarter-pel vectors), and from two MBs on one intra record"""
    r = np.zeros(w * h, dtype=M.MBREC)
    r["type"] = M.MBT_INTER
    r["mv"] = rng.integers(-12, 13, (w * h, 16, 2))
    if w * h > 1:
        r["type"][1] = M.MBT_I4x4
    return r.tobytes()


@pytest.fixture(scope="module")
def cases():
    """Per size: two current frames, two key frames, and the maps random (no
    runs), stepped (one oracle step from an identity map over records with
    small motion: mostly runs; the GPU test makes the same map with
    h264mi_accmv_step_device) and planted."""
    out = {}
    for name, (w, h) in SIZES.items():
        rng = np.random.default_rng(1000 + 17 * w + h)
        rec = near_motion_records(rng, w, h)
        stepped = A.step(rec, w, h, [A.identity(w, h, 1)])
        out[name] = dict(w=w, h=h, cur=[random_frame(rng, w, h) for _ in range(2)],
                         key=[random_frame(rng, w, h) for _ in range(2)], rec=rec,
                         maps=dict(random=random_map(rng, w, h), stepped=stepped, planted=R.planted_map(rng, w, h)))
    return out


# ------------------------------------------------------------------ CPU ----
def test_library_exports_the_accres_entry_points():
    from broadway_amd import _lib
    L = _lib.mi()
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    for name, nargs in (("h264mi_accres_device", 13), ("h264mi_engine_keep_accres", 2), ("h264mi_engine_accres_held", 3),
                        ("h264mi_engine_export_accres", 8)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int x, y, cw, ch, planes, dtype, colour, unanchored; float scale[3], bias[3]; }
    D = _lib.AccResDesc
    assert C.sizeof(D) == 8 * 4 + 2 * 3 * 4
    assert [getattr(D, n).offset for n in ("x", "y", "cw", "ch", "planes", "dtype", "colour", "unanchored")] == \
        [0, 4, 8, 12, 16, 20, 24, 28]
    assert (D.scale.offset, D.bias.offset) == (32, 44)
    assert _lib.ACCRES_PLANES == R.PLANES and _lib.ACCRES_UNANCHORED == R.POLICY and _lib.ACCRES_MAX_KEYS == 8


def test_accres_desc_arguments():
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import accres_desc
    d, n, dt = accres_desc("rgb", (1, 2, 3, 5), torch.float16, scale=0.25, bias=(0.0, 1.0, 2.0), colour="bt709",
                           unanchored="zero")
    assert (n, dt) == (3, torch.float16)
    assert (d.x, d.y, d.cw, d.ch, d.planes, d.dtype, d.colour, d.unanchored) == (1, 2, 3, 5, 3, _lib.TENSOR_F16, 2, 1)
    assert list(d.scale) == [0.25] * 3 and list(d.bias) == [0.0, 1.0, 2.0]
    d, n, dt = accres_desc()
    assert (n, dt, d.cw, d.ch, d.planes, d.dtype, d.colour, d.unanchored) == (1, torch.int16, 0, 0, 0, _lib.TENSOR_I16, 0, 0)
    assert accres_desc("uv", (2, 4, 6, 8))[1] == 2 and accres_desc("yuv")[1] == 3
    for kw in (dict(planes="Y"), dict(planes=0), dict(planes="uv", window=(1, 0, 4, 4)), dict(planes="uv", window=(0, 0, 4, 3)),
               dict(dtype=torch.uint8), dict(dtype=torch.int32), dict(planes="yuv", scale=(1.0,)),
               dict(planes="y", bias=(1.0, 2.0)), dict(window=(0, 0, 4)), dict(window=(0, 0, 0, 4)),
               dict(window=(-1, 0, 4, 4)), dict(planes="rgb", colour="stream"), dict(planes="rgb", colour="bt2020"),
               dict(planes="y", colour="bt709"), dict(unanchored="one"), dict(unanchored=1)):
        with pytest.raises(ValueError):
            accres_desc(**kw)


ACCRES_GRID = {
    "whole": "accept", "flush_right_bottom": "accept", "right_plus_1": "refuse", "right_plus_1_by_origin": "refuse",
    "bottom_plus_1": "refuse", "bottom_plus_1_by_origin": "refuse", "origin_0": "accept", "odd_window_yuv": "accept",
    "odd_window_rgb": "accept", "last_sample": "accept", "x_negative": "refuse", "y_negative": "refuse", "cw_0": "refuse",
    "ch_0": "refuse", "cw_negative": "refuse", "ch_negative": "refuse", "uv_even": "accept", "uv_whole": "accept",
    "uv_odd_x": "refuse", "uv_odd_y": "refuse", "uv_odd_cw": "refuse", "uv_odd_ch": "refuse", "dtype_u8": "refuse",
    "dtype_f16": "accept", "dtype_bf16": "accept", "dtype_f32": "accept", "dtype_5": "refuse", "dtype_minus_1": "refuse",
    "planes_rgb": "accept", "planes_4": "refuse", "planes_minus_1": "refuse", "colour_3": "accept", "colour_4": "refuse",
    "colour_stream": "refuse", "colour_stream_y": "refuse", "colour_minus_1": "refuse", "policy_zero": "accept",
    "policy_2": "refuse", "policy_minus_1": "refuse", "wide_2048_mbs": "accept", "wide_2049_mbs": "refuse",
    "tall_2048_mbs": "accept", "tall_2049_mbs": "refuse",
}


def test_descriptor_rules(tmp_path):
    """common/export_desc.h's accres rules walked by tests/accres_desc_check.c
    under AddressSanitizer + UBSan, a program of its own; the expected column
    is written out from include/h264mi.h."""
    exe = str(tmp_path / "accres_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "accres_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    got = {}
    for ln in p.stdout.splitlines():
        f = ln.split()
        assert f[0] == "accres" and f[1] not in got, ln
        got[f[1]] = f[2]
    assert sorted(got) == sorted(ACCRES_GRID)
    assert {k: v for k, v in got.items() if v != ACCRES_GRID[k]} == {}


def test_oracle_identities():
    rng = np.random.default_rng(5)
    w, h = 3, 2
    W, H = 16 * w, 16 * h
    c, k = random_frame(rng, w, h), random_frame(rng, w, h)
    ident = A.identity(w, h, 1)
    for planes in ALL_PLANES:
        assert not R.field(c, c, ident, w, h, planes).any(), planes          # identity map, K = C: zeros
        assert not R.field(c, None, ident, w, h, planes).any(), planes       # no key: zeros
        assert R.field(c, k, ident, w, h, planes).any(), planes
    # UV is the even-sited subsampling of YUV's chroma planes where the words of a 2x2 block agree on (JX >> 1, JY >> 1)
    m = random_map(rng, w, h)
    m[0::2, 1::2] = m[0::2, 0::2]
    m[1::2, :] = m[0::2, :]
    yuv, uv = R.field(c, k, m, w, h, "yuv"), R.field(c, k, m, w, h, "uv")
    assert np.array_equal(uv, yuv[1:, ::2, ::2])
    assert np.array_equal(yuv[1:, 1::2, 1::2], yuv[1:, ::2, ::2])
    # a planted counter-example: the odd-sited word of one block points elsewhere; UV does not see it
    m2 = m.copy()
    jx, jy, _ = R.origins(m2[4:5, 6:7], W, H)
    m2[5, 7] = A.pack((jx[0, 0] + 8) % W, (jy[0, 0] + 8) % H, 0)
    kk = np.arange(R.slot_bytes(w, h), dtype=np.int64)                       # a key frame whose samples all differ nearby
    kk = ((kk * 37) % 251).astype(np.uint8)
    yuv2, uv2 = R.field(c, kk, m2, w, h, "yuv"), R.field(c, kk, m2, w, h, "uv")
    assert np.array_equal(uv2, R.field(c, kk, m, w, h, "uv"))
    assert not np.array_equal(yuv2[1:, 5, 7], yuv2[1:, 4, 6])
    # ZERO differs from KEY only where A = 0
    for planes in ALL_PLANES:
        a, z = R.field(c, k, m, w, h, planes, "key"), R.field(c, k, m, w, h, planes, "zero")
        anch = (m >> 31).astype(bool)
        anch = anch[::2, ::2] if planes == "uv" else anch
        assert np.array_equal(a[:, anch], z[:, anch]) and not z[:, ~anch].any() and a[:, ~anch].any(), planes


def test_the_planted_data_takes_both_gather_paths(cases):
    """From the oracle's own classification: in every size the whole-picture
    exports of the planted map take both paths, runs start at every byte offset
    and end on the last sample of the plane; the random map has (nearly) no
    run and the stepped map mostly runs."""
    for name, c in cases.items():
        w, h = c["w"], c["h"]
        whole = (0, 0, 16 * w, 16 * h)
        for planes in ("y", "uv"):
            p = R.gather_paths(c["maps"]["planted"], w, h, whole, planes)
            assert p["runs"] > 0 and p["singles"] > 0 and p["offsets"] == {0, 1, 2, 3} and p["at_end"] >= 1, (name, planes, p)
            assert p["crossing"] >= 3, (name, planes, p)
        r = R.gather_paths(c["maps"]["random"], w, h, whole, "y")
        assert r["singles"] > 20 * max(r["runs"], 1), (name, r)
        s = R.gather_paths(c["maps"]["stepped"], w, h, whole, "y")
        assert s["runs"] > s["singles"] > 0 and len(s["offsets"]) == 4, (name, s)
        jx = c["maps"]["planted"] & 0x7FFF
        jy = (c["maps"]["planted"] >> 16) & 0x7FFF
        assert (jx >= 16 * w).any() and (jy >= 16 * h).any()                 # out-of-range words are there


def test_the_stream_exercises_the_feature(captured):
    """What the engine tests rely on, from the captured records: where the
    keys go, that a GOP-1 picture outlives key 2's decode, and -- a property of
    the maps alone, so checked on frames of random samples, not on the
    stream's pictures -- that in every P picture the two policies differ and
    some sample has v != 0."""
    cap, chain, maps = captured
    st = chain.stats
    slots = [p.cur_slot for p in cap.pictures]
    keys = [k for k, s in enumerate(st) if s["key"]]
    assert len(keys) == 2 and slots[keys[0]] == slots[keys[1]] == 4         # both keys go to slot 4
    assert any(slots[k] not in slots[k + 1:keys[1] + 1] for k in range(1, keys[1]))      # a GOP-1 picture outlives key 2's decode
    W, H = 16 * cap.w_mbs, 16 * cap.h_mbs
    rng = np.random.default_rng(3)
    c, k = random_frame(rng, cap.w_mbs, cap.h_mbs), random_frame(rng, cap.w_mbs, cap.h_mbs)
    for i, s in enumerate(st):
        if s["key"]:
            continue
        a, z = R.field(c, k, maps[i], cap.w_mbs, cap.h_mbs, "y", "key"), R.field(c, k, maps[i], cap.w_mbs, cap.h_mbs, "y", "zero")
        assert (a != z).any() and z.any(), i                                 # the policies differ, and v != 0 somewhere


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


def make_desc(win, planes, dtype, policy="key", colour=0, consts="unit"):
    from broadway_amd import _lib
    d = _lib.AccResDesc()
    d.x, d.y, d.cw, d.ch = win
    d.planes = R.PLANES.get(planes, planes)
    d.dtype = M.DTYPE_ID.get(dtype, dtype)
    d.colour = colour
    d.unanchored = R.POLICY.get(policy, policy)
    scale, bias = M.CONSTS[consts]
    d.scale[:] = scale[:3]
    d.bias[:] = bias[:3]
    return d


FRONT = 64


def run_accres(w, h, curs, keys, maps, order, win, planes, dtype, policy="key", colour=0, consts="unit", out_pad=0,
               skew=0, stride=None, null=(), npics=None, dims=None, map_offs=None, cur_skew=0, key_skew=0, map_skew=0,
               desc=None):
    """h264mi_accres_device over pictures order[k] = (current, key or None, map)
    indices; the inputs lie in one device buffer, 64 sentinel bytes apart.
    Returns rc, the whole output buffer (FRONT + skew sentinel bytes, then
    pictures out_stride apart, then 64 sentinel bytes), the first picture's
    offset, out_stride and a picture's bytes."""
    import torch
    L = _mi()
    fb = R.slot_bytes(w, h)
    mb = 4 * 256 * w * h
    pad = 64
    host = np.full((fb + pad) * (len(curs) + len(keys)) + (mb + pad) * len(maps) + pad, SENTINEL, dtype=np.uint8)
    cur0, key0 = 0, (fb + pad) * len(curs)
    map0 = key0 + (fb + pad) * len(keys)
    for i, f in enumerate(curs):
        host[cur0 + i * (fb + pad):cur0 + i * (fb + pad) + fb] = f
    for i, f in enumerate(keys):
        host[key0 + i * (fb + pad):key0 + i * (fb + pad) + fb] = f
    for i, m in enumerate(maps):
        host[map0 + i * (mb + pad):map0 + i * (mb + pad) + mb] = m.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).to("cuda")
    n = len(order)
    co = (C.c_size_t * n)(*[c * (fb + pad) for c, _, _ in order])
    ko = (C.c_size_t * n)(*[NOKEY if k is None else k * (fb + pad) for _, k, _ in order])
    mo = (C.c_size_t * n)(*([m * (mb + pad) for _, _, m in order] if map_offs is None else map_offs))
    es = M.ELEM.get(dtype, 2)
    hs = 1 if planes == "uv" else 0
    npl = R.NPLANES.get(planes, 1)
    nbytes = npl * (win[2] >> hs) * (win[3] >> hs) * es if win[2] > 0 and win[3] > 0 else 16
    nbytes = max(nbytes, es)
    out_stride = nbytes + out_pad if stride is None else stride
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d = make_desc(win, planes, dtype, policy, colour, consts) if desc is None else desc
    wm, hm = dims or (w, h)
    base = dev.data_ptr()
    rc = L.h264mi_accres_device(None if "cur" in null else base + cur0 + cur_skew, None if "co" in null else co,
                                None if "key" in null else base + key0 + key_skew, None if "ko" in null else ko,
                                None if "maps" in null else base + map0 + map_skew, None if "mo" in null else mo,
                                n if npics is None else npics, wm, hm, None if "desc" in null else C.byref(d),
                                None if "out" in null else d_out.data_ptr() + first, out_stride,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)                          # the inputs are only read
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


def windows(W, H):
    """whole; one sample; the last one; odd and off every grid (the element
    path); 8 columns from an odd one (16-byte rows for every element type)"""
    return [(0, 0, W, H), (5, 3, 1, 1), (W - 1, H - 1, 1, 1), (3, 1, W - 5, H - 3), (1, 1, 8, H - 2)]


def uv_windows(W, H):
    return [(0, 0, W, H), (4, 2, 2, 2), (W - 2, H - 2, 2, 2), (2, 2, W - 6, H - 4), (2, 0, 8, H - 2), (0, 2, 16, 4)]


def consts_of(dtype):
    return ["unit"] if dtype == "int16" else ["unit", "mixed"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(SIZES))
def test_kernel_vs_oracle(cases, size):
    """Every map kind, plane set, window, element type, policy and constant
    set of one size; the stepped map is made on the device and equals the
    oracle's."""
    import torch
    c = cases[size]
    w, h = c["w"], c["h"]
    W, H = 16 * w, 16 * h
    L = _mi()
    # the stepped map, from h264mi_accmv_step_device
    rec = torch.from_numpy(np.frombuffer(c["rec"], dtype=np.uint8).copy()).to("cuda")
    ident = torch.from_numpy(A.identity(w, h, 1).view(np.int32).reshape(-1)).to("cuda")
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ptrs = (C.c_void_p * 1)(ident.data_ptr())
    assert L.h264mi_accmv_step_device(rec.data_ptr(), w, h, ptrs, 1, 0, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    stepped = out.cpu().numpy().view(np.uint32).reshape(H, W)
    assert same(stepped, c["maps"]["stepped"])
    names = ["random", "stepped", "planted"]
    maps = [c["maps"]["random"], stepped, c["maps"]["planted"]]
    for mi, mname in enumerate(maps):
        for planes in ALL_PLANES:
            wins = uv_windows(W, H) if planes == "uv" else windows(W, H)
            for wi, win in enumerate(wins):
                # every dtype on the whole picture and the off-grid window; the others rotate through them
                dts = M.DTYPES if wi in (0, 3) else [M.DTYPES[(wi + mi) % 4]]
                for dtype in dts:
                    for policy in ("key", "zero"):
                        consts = consts_of(dtype)[-1] if policy == "key" else "unit"
                        rc, o, first, stride, nbytes = run_accres(w, h, c["cur"][:1], c["key"][:1], [maps[mi]], [(0, 0, 0)],
                                                                  win, planes, dtype, policy, 1, consts)
                        tag = (names[mi], planes, win, dtype, policy)
                        assert rc == 0, tag
                        want = R.expect(c["cur"][0], c["key"][0], maps[mi], w, h, win, planes, dtype, policy, 1, consts)
                        assert same(o[first:first + nbytes], want), tag
                        assert (o[:first] == SENTINEL).all() and (o[first + nbytes:] == SENTINEL).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_kernel_colour_sets_on_the_extremes_picture(colour):
    """RGB under every colour id: tests/_colour.py's extremes picture (every
    clamp, both signs of every term) as the current frame and, turned upside
    down, as the key frame, through a random map."""
    pic, pw, ph, pcp = COL.extremes_picture()
    w, h = pw // 16, (ph + 15) // 16
    W, H = 16 * w, 16 * h
    packed = np.zeros(W * H * 3 // 2, dtype=np.uint8)
    packed[:pw * ph] = pic[:pw * ph]
    c4 = (pw // 2) * (ph // 2)
    packed[W * H:W * H + c4] = pic[pw * ph:pw * ph + c4]
    packed[W * H + W * H // 4:W * H + W * H // 4 + c4] = pic[pw * ph + c4:]
    cur = R.from_packed(packed, w, h)
    key = np.ascontiguousarray(cur[::-1])
    m = random_map(np.random.default_rng(77), w, h)
    whole = (0, 0, W, H)
    for dtype, win in (("int16", whole), ("float32", (3, 1, W - 5, H - 3))):
        rc, o, first, stride, nbytes = run_accres(w, h, [cur], [key], [m], [(0, 0, 0)], win, "rgb", dtype, "key", colour, "mixed")
        assert rc == 0
        want = R.expect(cur, key, m, w, h, win, "rgb", dtype, "key", colour, "mixed")
        assert same(o[first:first + nbytes], want), (dtype, win)
    f = R.field(cur, key, m, w, h, "rgb", "key", colour)
    assert f.min() < -200 and f.max() > 200


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_kernel_batched_padded_strides_write_nothing_else(cases, dtype):
    """A list that mixes pictures with and without a key over two current
    frames, two keys and three maps; out_stride padded by 5 elements (the
    element path), by 48 bytes (16-byte stores) and by 48 bytes with d_out one
    element past a 16-byte boundary (the element path again)."""
    c = cases["3x2"]
    w, h = c["w"], c["h"]
    W, H = 16 * w, 16 * h
    es = M.ELEM[dtype]
    maps = [c["maps"]["random"], c["maps"]["stepped"], c["maps"]["planted"]]
    order = [(1, 0, 2), (0, None, 1), (0, 1, 0), (1, None, 2), (0, 0, 1)]
    for planes, win in (("yuv", (0, 0, W, H)), ("y", (1, 1, 8, H - 2)), ("uv", (2, 2, 16, H - 4)), ("rgb", (3, 1, W - 5, H - 3))):
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, o, first, stride, nbytes = run_accres(w, h, c["cur"], c["key"], maps, order, win, planes, dtype, "key", 2,
                                                      "mixed", out_pad=out_pad, skew=skew)
            tag = (planes, win, out_pad, skew)
            assert rc == 0, tag
            assert (o[:first] == SENTINEL).all(), tag
            for k, (ci, ki, mi) in enumerate(order):
                at = first + k * stride
                want = R.expect(c["cur"][ci], None if ki is None else c["key"][ki], maps[mi], w, h, win, planes, dtype,
                                "key", 2, "mixed")
                assert same(o[at:at + nbytes], want), tag + (k,)
                assert (o[at + nbytes:at + stride] == SENTINEL).all(), tag + (k,)
            assert (o[first + len(order) * stride:] == SENTINEL).all(), tag


@pytest.mark.gpu
def test_kernel_list_longer_than_one_launch_and_no_key_at_all(cases):
    c = cases["1x1"]
    w, h = c["w"], c["h"]
    maps = [c["maps"]["random"], c["maps"]["planted"]]
    order = [(k % 2, None if k % 3 == 0 else (k // 3) % 2, (k // 2) % 2) for k in range(CAP + 1)]
    win = (3, 2, 8, 5)
    rc, o, first, stride, nbytes = run_accres(w, h, c["cur"], c["key"], maps, order, win, "yuv", "float32", "zero", 0, "mixed")
    assert rc == 0
    for k, (ci, ki, mi) in enumerate(order):
        at = first + k * stride
        want = R.expect(c["cur"][ci], None if ki is None else c["key"][ki], maps[mi], w, h, win, "yuv", "float32", "zero",
                        0, "mixed")
        assert same(o[at:at + nbytes], want), k
    assert (o[:first] == SENTINEL).all() and (o[first + len(order) * stride:] == SENTINEL).all()
    # no picture has a key: d_key may be NULL
    rc, o, first, stride, nbytes = run_accres(w, h, c["cur"], c["key"], maps, [(0, None, 0), (1, None, 1)], win, "y",
                                              "float16", "key", 0, "mixed", null=("key",))
    assert rc == 0
    want = M.convert(np.zeros((1, 5, 8), dtype=np.int64), "float16", *M.CONSTS["mixed"])
    assert same(o[first:first + nbytes], want) and same(o[first + stride:first + stride + nbytes], want)


@pytest.mark.gpu
def test_kernel_rejects_bad_arguments(cases):
    c = cases["3x2"]
    w, h = c["w"], c["h"]
    maps = [c["maps"]["random"]]
    good = (1, 1, 4, 4)

    def refused(**kw):
        args = dict(win=good, planes="y", dtype="float16")
        args.update(kw)
        win, planes, dtype = args.pop("win"), args.pop("planes"), args.pop("dtype")
        order = args.pop("order", [(0, 0, 0)])
        rc, o, *_ = run_accres(w, h, c["cur"][:1], c["key"][:1], maps, order, win, planes, dtype, **args)
        assert rc == -1, kw
        assert (o == SENTINEL).all(), kw                 # nothing was launched

    rc, o, first, _, nbytes = run_accres(w, h, c["cur"][:1], c["key"][:1], maps, [(0, 0, 0)], good, "y", "float16")
    assert rc == 0 and not (o[first:first + nbytes] == SENTINEL).all()      # the arguments below are one step away
    for planes in (4, -1):
        refused(planes=planes)
    for dtype in (0, 5, -1):
        refused(dtype=dtype)
    for colour in (4, 15, -1):
        refused(colour=colour, planes="rgb")
    refused(colour=15)
    for policy in (2, -1):
        refused(policy=policy)
    for win in ((0, 0, 49, 8), (0, 0, 48, 33), (48, 0, 1, 1), (0, 32, 1, 1), (45, 0, 4, 1), (0, 30, 1, 3), (-1, 0, 4, 4),
                (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -4, 4)):
        refused(win=win)
    for win in ((1, 0, 4, 4), (0, 1, 4, 4), (0, 0, 3, 4), (0, 0, 4, 3)):
        refused(win=win, planes="uv")
    for null in ("cur", "co", "ko", "maps", "mo", "desc", "out"):
        refused(null=(null,))
    refused(null=("key",))                               # a picture has a key and d_key is NULL
    refused(npics=0)
    refused(npics=-1)
    refused(dims=(0, 2))
    refused(dims=(3, 0))
    refused(dims=(2049, 2))
    for dtype, skew in (("int16", 1), ("float16", 1), ("bfloat16", 1), ("float32", 2)):
        refused(dtype=dtype, skew=skew)                  # d_out not a multiple of the element size
    refused(dtype="float16", stride=4 * 4 * 2 + 1)       # nor out_stride
    refused(dtype="float32", stride=4 * 4 * 4 + 2)
    refused(map_offs=[2])                                # not a multiple of 4
    refused(map_skew=2)
    refused(cur_skew=2)
    refused(key_skew=2)


def want_engine(eng, cap, stream, slot, m, key, win, planes, dtype, policy="key", colour=0, consts="unit"):
    cur = R.from_packed(eng.read(stream, slot), cap.w_mbs, cap.h_mbs)
    return R.expect(cur, key, m, cap.w_mbs, cap.h_mbs, win, planes, dtype, policy, colour, consts)


class Tracker:
    """What the test itself knows of one stream: the oracle chain's serials and,
    per key serial, the key picture's frame as read back right after its decode."""

    def __init__(self, cap, nkeys, first_serial=1):
        self.cap, self.nkeys = cap, nkeys
        self.chain = A.Chain(cap.w_mbs, cap.h_mbs, cap.nslots)
        self.keys = {}
        self.first = first_serial

    def decoded(self, eng, stream, i):
        pic = self.cap.pictures[i]
        self.chain.decode(self.cap.records_bytes(i), pic.cur_slot)
        if self.chain.stats[-1]["key"]:
            self.keys[self.chain.key] = R.from_packed(eng.read(stream, pic.cur_slot), self.cap.w_mbs, self.cap.h_mbs)

    def key_of(self, slot):
        t = self.chain.ser[slot]
        held = t >= self.first and t > self.chain.key - self.nkeys and t in self.keys
        return self.keys[t] if held else None


def check_all_slots(eng, cap, stream, tr, tag, planes="y", policy="key"):
    import torch
    ns = cap.nslots
    W, H = 16 * cap.w_mbs, 16 * cap.h_mbs
    whole = (0, 0, W, H)
    got_maps = engine_maps(eng, stream, ns, W, H)
    t = eng.to_accres([stream] * ns, list(range(ns)), planes=planes, unanchored=policy)
    torch.cuda.synchronize()
    hs = 1 if planes == "uv" else 0
    assert tuple(t.shape) == (ns, R.NPLANES[planes], H >> hs, W >> hs) and t.dtype == torch.int16
    for s in range(ns):
        assert same(got_maps[s], tr.chain.maps[s]), tag + (s,)
        key = tr.key_of(s)
        assert eng.accres_held(stream, s) == (key is not None), tag + (s,)
        assert same(tensor_bytes(t[s]), want_engine(eng, cap, stream, s, got_maps[s], key, whole, planes, "int16", policy)), \
            tag + (s,)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [2, 1])
def test_engine_exports_against_the_held_keys(captured, nkeys):
    """Picture by picture: after each one every slot's export equals the oracle
    on the frames read back, the maps from to_accmv and the key the test
    tracked; with two keys the slots of GOP 1 still export against key 1 after
    key 2 overwrote its slot, with one they export zeros; retention changes no
    pixel."""
    import torch
    from broadway_amd.engine import Engine
    cap, chain_all, _ = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    plain = Engine(w, h, 1, ns)
    for pic in cap.pictures:
        plain.decode([0], [pic])
    want_pixels = [plain.read(0, s).tobytes() for s in range(ns)]
    with pytest.raises(RuntimeError):
        plain.keep_accres()                             # needs keep_accmv
    with pytest.raises(RuntimeError):
        plain.to_accres([0], [0])
    with pytest.raises(RuntimeError):
        plain.accres_held(0, 0)
    plain.close()

    eng = Engine(w, h, 1, ns)
    eng.keep_accmv()
    eng.keep_accres(nkeys)
    tr = Tracker(cap, nkeys)
    key2 = [k for k, s in enumerate(chain_all.stats) if s["key"]][1]
    stale_nonzero = stale_zero = 0
    for k in range(cap.npics):
        eng.decode([0], [cap.pictures[k]])
        tr.decoded(eng, 0, k)
        t = check_all_slots(eng, cap, 0, tr, (k,), planes=ALL_PLANES[k % 4], policy=("key", "zero")[(k // 4) % 2])
        if k >= key2:
            for s in range(ns):
                if 0 < tr.chain.ser[s] < tr.chain.key:                      # a GOP-1 picture after key 2's decode
                    stale_nonzero += bool(t[s].any())
                    stale_zero += not bool(t[s].any())
    if nkeys == 2:
        assert stale_nonzero > 0 and stale_zero == 0
    else:
        assert stale_zero > 0 and stale_nonzero == 0
    assert eng.errors() == 0
    assert [eng.read(0, s).tobytes() for s in range(ns)] == want_pixels
    # the export proper: dtypes, constants, a window off every grid, colour
    last = cap.pictures[-1].cur_slot
    m = tr.chain.maps[last]
    for planes, dtype, consts, win, colour in (("y", "float16", "mixed", (7, 3, 57, 41), None),
                                               ("uv", "float32", "mixed", (6, 2, 58, 40), None),
                                               ("yuv", "bfloat16", "unit", (0, 0, 96, 64), None),
                                               ("rgb", "float32", "mixed", (7, 3, 57, 41), "bt709-full")):
        scale, bias = M.CONSTS[consts]
        npl = R.NPLANES[planes]
        t = eng.to_accres([0], [last], planes=planes, window=win, dtype=getattr(torch, dtype), scale=scale[:npl],
                          bias=bias[:npl], colour=colour)
        torch.cuda.synchronize()
        cid = 0 if colour is None else COL.NAMES.index(colour)
        assert same(tensor_bytes(t), want_engine(eng, cap, 0, last, m, tr.key_of(last), win, planes, dtype, "key", cid, consts)), planes
    for kw in (dict(streams=[1], slots=[0]), dict(streams=[0], slots=[ns]), dict(streams=[0], slots=[0], window=(0, 0, 97, 1))):
        with pytest.raises(RuntimeError):
            eng.to_accres(**kw)
    with pytest.raises(RuntimeError):
        eng.accres_held(0, ns)
    with pytest.raises(RuntimeError):
        eng.keep_accres(9)
    eng.close()


@pytest.mark.gpu
def test_engine_key_copy_is_ordered_against_an_earlier_export_of_its_entry(captured):
    """One key per stream: a GOP-1 slot is exported into ``out`` against key 1,
    then key 2 is decoded with no synchronisation in between and is copied over
    the entry the export reads: ``out`` holds the residual against key 1."""
    import torch
    from broadway_amd.engine import Engine
    cap, chain_all, maps = captured
    w, h = cap.w_mbs, cap.h_mbs
    whole = (0, 0, 16 * w, 16 * h)
    key2 = [k for k, s in enumerate(chain_all.stats) if s["key"]][1]
    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_accmv()
    eng.keep_accres(1)
    tr = Tracker(cap, 1)
    for k in range(key2):
        eng.decode([0], [cap.pictures[k]])
        tr.decoded(eng, 0, k)
    s = cap.pictures[key2 - 1].cur_slot
    assert s != cap.pictures[key2].cur_slot and eng.accres_held(0, s)
    want = want_engine(eng, cap, 0, s, maps[key2 - 1], tr.key_of(s), whole, "yuv", "int16")
    out = torch.empty((1, 3, 16 * h, 16 * w), dtype=torch.int16, device="cuda")
    assert eng.to_accres([0], [s], planes="yuv", out=out) is out
    eng.decode([0], [cap.pictures[key2]])               # copies key 2 into the only entry
    torch.cuda.synchronize()
    assert same(tensor_bytes(out), want) and want.any()
    assert not eng.accres_held(0, s) and not eng.to_accres([0], [s]).any()
    eng.close()


def concealment_passes(cap):
    """The two decode passes of a neighbour-based concealment (host/conceal.c)
    of the stream's first key picture with the lower half of its MBs lost, as
    pictures Engine.decode takes, with their record bytes, the MBs to conceal
    and the decoded flags.  Pass 1: the decoded MBs unfiltered, the lost ones
    grey I_PCM.  Pass 2: the decoded MBs as they were, each lost MB a
    zero-vector skip record that names the picture's own slot, filtered as
    intra with QP 40."""
    from broadway_amd.engine import CapturedPicture
    n, w = cap.w_mbs * cap.h_mbs, cap.w_mbs
    pic = cap.pictures[0]
    lost = list(range(n // 2, n))
    rec = np.frombuffer(cap.records_bytes(0), dtype=M.MBREC)
    coef = cap.coef_bytes(0) + bytes([128]) * 384               # the picture's blocks, then one grey MB (12 blocks)
    p1, p2 = rec.copy(), rec.copy()
    p1["avail"] &= 0x8F                                         # ~(DB_LEFT | DB_TOP | DB_INNER)
    for m in lost:
        sl = rec["slice"][m]
        p1[m] = np.zeros((), dtype=M.MBREC)
        p1["type"][m], p1["coef"][m], p1["slice"][m] = M.MBT_IPCM, pic.ncoef, sl
        p2[m] = np.zeros((), dtype=M.MBREC)
        p2["type"][m], p2["ref"][m], p2["dbf"][m], p2["slice"][m] = M.MBT_SKIP, pic.cur_slot, 1, sl
        p2["qp"][m], p2["qpc"][m] = 40, 36
        p2["avail"][m] = 64 | (16 if m % w else 0) | (32 if m >= w else 0)
    bufs = [C.create_string_buffer(p1.tobytes()), C.create_string_buffer(p2.tobytes()), C.create_string_buffer(coef)]
    pics = [CapturedPicture(C.addressof(b), C.addressof(bufs[2]), pic.ncoef + 12, pic.cur_slot, 0, 0, n, 0) for b in bufs[:2]]
    return pics, [p1.tobytes(), p2.tobytes()], lost, [int(m < n // 2) for m in range(n)], bufs


def test_the_concealment_passes_are_what_the_engine_looks_for(captured):
    """Pass 1 is a key picture by the record rule, pass 2 is none and its inter
    records name the picture's own slot."""
    cap, _, _ = captured
    pics, recs, lost, decoded, _ = concealment_passes(cap)
    assert A.is_key(cap.records_bytes(0)) and A.is_key(recs[0]) and not A.is_key(recs[1])
    r = np.frombuffer(recs[1], dtype=M.MBREC)
    inter = r["type"] <= M.MBT_SKIP
    assert inter.sum() == len(lost) and (r["ref"][inter] == pics[1].cur_slot).all() and sum(decoded) == len(lost)


@pytest.mark.gpu
def test_engine_key_copy_follows_a_concealment(captured):
    """The key store must hold the final samples of a key picture's slot.  A
    key picture is decoded (pass 1), concealed in place, and decoded again into
    its slot (pass 2); all three change the slot.  After each, the slot's
    export through its own identity map is all zeros exactly when the held key
    equals the slot's samples now.  The GOP's P pictures are then set against
    the concealed, filtered key -- and not against an earlier state of it."""
    import torch
    from broadway_amd.engine import Engine
    cap, _, _ = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    W, H = 16 * w, 16 * h
    whole = (0, 0, W, H)
    pics, recs, lost, decoded, bufs = concealment_passes(cap)
    slot = pics[0].cur_slot
    eng = Engine(w, h, 1, ns)
    eng.keep_accmv()
    eng.keep_accres(2)
    chain = A.Chain(w, h, ns)
    states = []

    def stage(tag):
        t = eng.to_accres([0], [slot], planes="yuv")
        torch.cuda.synchronize()
        states.append(eng.read(0, slot).tobytes())
        assert eng.accres_held(0, slot), tag
        assert not t.any(), tag                                  # the held key is the slot as it is now

    eng.decode([0], [pics[0]])
    chain.decode(recs[0], slot)
    stage("pass 1")
    eng.conceal(0, slot, lost, decoded)
    stage("concealed")
    eng.decode([0], [pics[1]])
    chain.decode(recs[1], slot)
    stage("pass 2")
    assert len(set(states)) == 3 and chain.key == 1              # every stage rewrote the slot; one key serial
    got = engine_maps(eng, 0, ns, W, H)
    assert same(got[slot], A.identity(w, h, 0))                  # (a concealed key picture's map is unanchored)
    keys = [R.from_packed(np.frombuffer(s, dtype=np.uint8), w, h) for s in states]
    told_apart = 0
    for k in range(1, 5):
        eng.decode([0], [cap.pictures[k]])
        chain.decode(cap.records_bytes(k), cap.pictures[k].cur_slot)
        s = cap.pictures[k].cur_slot
        got = engine_maps(eng, 0, ns, W, H)
        assert same(got[s], chain.maps[s]), k
        t = eng.to_accres([0], [s], planes="yuv")
        torch.cuda.synchronize()
        assert eng.accres_held(0, s), k
        assert same(tensor_bytes(t), want_engine(eng, cap, 0, s, got[s], keys[2], whole, "yuv", "int16")), k
        told_apart += any(not np.array_equal(want_engine(eng, cap, 0, s, got[s], keys[2], whole, "yuv", "int16"),
                                             want_engine(eng, cap, 0, s, got[s], old, whole, "yuv", "int16")) for old in keys[:2])
    assert told_apart > 0 and eng.errors() == 0
    # a picture that is no second pass, decoded into the key's slot, ends the slot's standing: a conceal there copies nothing
    # (picture 1's records with the slot they name changed: no picture references the slot it is decoded into)
    other = cap.pictures[1]
    from broadway_amd.engine import CapturedPicture
    r = np.frombuffer(cap.records_bytes(1), dtype=M.MBREC).copy()
    assert (r["ref"][r["type"] <= M.MBT_SKIP] == slot).any() and other.cur_slot != slot
    r["ref"][r["ref"] == slot] = other.cur_slot
    rbuf = C.create_string_buffer(r.tobytes())
    moved = CapturedPicture(C.addressof(rbuf), other.coef, other.ncoef, slot, 0, other.n_inter, other.n_intra, other.n_coded)
    eng.decode([0], [moved])
    eng.conceal(0, slot, lost, decoded)
    s = cap.pictures[4].cur_slot
    assert s != slot
    t = eng.to_accres([0], [s], planes="yuv")
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), want_engine(eng, cap, 0, s, engine_maps(eng, 0, ns, W, H)[s], keys[2], whole, "yuv", "int16"))
    eng.close()


@pytest.mark.gpu
def test_engine_forget_off_and_on(captured):
    import torch
    from broadway_amd.engine import Engine
    cap, _, _ = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    eng = Engine(w, h, 1, ns)
    eng.keep_accmv()
    eng.keep_accres(2)
    tr = Tracker(cap, 2)
    for k in range(4):
        eng.decode([0], [cap.pictures[k]])
        tr.decoded(eng, 0, k)
    s3 = cap.pictures[3].cur_slot
    assert eng.accres_held(0, s3) and eng.to_accres([0], [s3]).any()
    eng.forget_records(0, s3)                           # the slot's serial is cleared: no key, zeros
    tr.chain.forget(s3)
    assert not eng.accres_held(0, s3) and not eng.to_accres([0], [s3]).any()
    check_all_slots(eng, cap, 0, tr, ("forgot",))
    # switching the keys off then on starts from nothing: the maps stay, the pictures decoded before have no key
    eng.keep_accres(0)
    with pytest.raises(RuntimeError):
        eng.to_accres([0], [0])
    eng.keep_accres(2)
    tr.first = tr.chain.key + 1
    check_all_slots(eng, cap, 0, tr, ("off-on",))
    assert not any(eng.accres_held(0, s) for s in range(ns))
    for k in range(4, cap.npics):
        eng.decode([0], [cap.pictures[k]])
        tr.decoded(eng, 0, k)
    check_all_slots(eng, cap, 0, tr, ("after",))
    assert any(eng.accres_held(0, s) for s in range(ns))
    # switching the maps off switches the keys off with them
    eng.keep_accmv(False)
    with pytest.raises(RuntimeError):
        eng.accres_held(0, 0)
    with pytest.raises(RuntimeError):
        eng.keep_accres(2)
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.gpu
def test_engine_two_streams_at_different_phases_do_not_mix(captured):
    """Stream 1 runs three pictures behind stream 0 in one engine, so batches
    hold a key picture of one and a P picture of the other."""
    from broadway_amd.engine import Engine
    cap, _, _ = captured
    w, h, ns = cap.w_mbs, cap.h_mbs, cap.nslots
    eng = Engine(w, h, 2, ns)
    eng.keep_accmv()
    eng.keep_accres(2)
    trs = [Tracker(cap, 2), Tracker(cap, 2)]
    lag = 3
    for k in range(cap.npics + lag):
        streams = [s for s, i in ((0, k), (1, k - lag)) if 0 <= i < cap.npics]
        idx = [i for i in (k, k - lag) if 0 <= i < cap.npics]
        eng.decode(streams, [cap.pictures[i] for i in idx])
        for s, i in zip(streams, idx):
            trs[s].decoded(eng, s, i)
        if k in (4, 6, 8, cap.npics + lag - 1):
            for s in (0, 1):
                check_all_slots(eng, cap, s, trs[s], (k, s))
    assert eng.errors() == 0
    eng.close()


@pytest.mark.gpu
def test_engine_export_is_ordered_against_the_next_decode_into_the_slot(captured):
    """Export into ``out``, then decode the next picture into the same slot
    with no synchronisation in between: ``out`` holds the earlier picture's
    residual."""
    import torch
    from broadway_amd.engine import Engine
    cap, _, maps = captured
    slots = [p.cur_slot for p in cap.pictures]
    k1 = next(k for k in range(2, cap.npics) if slots[k] in slots[1:k])     # the first decode over a P picture's slot
    k0 = slots.index(slots[k1], 1)
    w, h = cap.w_mbs, cap.h_mbs
    whole = (0, 0, 16 * w, 16 * h)
    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_accmv()
    eng.keep_accres(2)
    tr = Tracker(cap, 2)
    for k in range(k1):
        eng.decode([0], [cap.pictures[k]])
        tr.decoded(eng, 0, k)
    want0 = want_engine(eng, cap, 0, slots[k0], maps[k0], tr.key_of(slots[k0]), whole, "yuv", "int16")
    out = torch.empty((1, 3, 16 * h, 16 * w), dtype=torch.int16, device="cuda")
    assert eng.to_accres([0], [slots[k0]], planes="yuv", out=out) is out
    eng.decode([0], [cap.pictures[k1]])
    after = eng.to_accres([0], [slots[k1]], planes="yuv")
    torch.cuda.synchronize()
    tr.decoded(eng, 0, k1)
    assert same(tensor_bytes(out), want0)
    assert same(tensor_bytes(after), want_engine(eng, cap, 0, slots[k1], maps[k1], tr.key_of(slots[k1]), whole, "yuv", "int16"))
    assert not np.array_equal(tensor_bytes(out), tensor_bytes(after))
    eng.close()
