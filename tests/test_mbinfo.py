"""Motion vectors and MB side information as device tensors (mbinfo.hip): the
MbRec batches of decoded pictures as planar (C, bh, bw) fields on the luma
4x4-block grid -- h264mi_mbinfo_device, record retention and
h264mi_engine_export_mbinfo (Engine.keep_records / to_mbinfo), and
H264SwDecKeepMbInfo / H264SwDecLastPictureMbInfo (Decoder's ``mbinfo`` option).

The oracle (tests/_mbinfo.py) restates the field definition of include/h264mi.h
in numpy over the raw record bytes.  Every comparison is exact equality of
bytes."""
import ctypes as C
import hashlib
from fractions import Fraction

import numpy as np
import pytest

import _crop
import _mbinfo as M
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CAP = 32                    # pictures per kernel launch (MBINFO_MAX_PICS)
CASE = _crop.cases()["crop_ltrb_6x4"]       # config 2, 6x4 MBs, 5 frames, gop 3, 2 slices, crop (6, 2) 86x52
CROP_BLOCKS = (1, 0, 22, 14)                # the blocks covering that crop window


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


@pytest.fixture(scope="module")
def captured():
    """(Capture, per picture the oracle field over the whole grid) of the stream"""
    from broadway_amd.engine import Capture
    cap = Capture(case_stream())
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs) == (6, 4)
    fields = [M.field(cap.records_bytes(i), cap.w_mbs, cap.h_mbs) for i in range(cap.npics)]
    for f in fields:
        f.setflags(write=False)
    return cap, fields


# ------------------------------------------------------------------ CPU ----
def test_zscan_is_a_bijection_and_matches_the_parsers_tables():
    from broadway_amd import _lib
    L = _lib.mi()
    bx = list((C.c_uint8 * 16).in_dll(L, "kBlkX"))
    by = list((C.c_uint8 * 16).in_dll(L, "kBlkY"))
    seen = set()
    for y in range(4):
        for x in range(4):
            b = M.zscan(x, y)
            assert 0 <= b < 16 and (bx[b], by[b]) == (x, y)
            seen.add(b)
    assert seen == set(range(16))


def test_exactness_premise():
    """For every constant set of these tests and every int16 v, float64(v) *
    float64(scale) + float64(bias) is exact (a 16-bit x 24-bit product plus a
    24-bit addend within 53 bits), so the oracle's one rounding to fp32 is the
    rounding of a fused multiply-add."""
    pairs = {(s, b) for scale, bias in M.CONSTS.values() for s, b in zip(scale, bias)}
    v = np.arange(-32768, 32768, dtype=np.int64)
    for s, b in sorted(pairs):
        assert float(np.float32(s)) == s and float(np.float32(b)) == b          # fp32-representable
        got = (v.astype(np.float64) * np.float64(s) + np.float64(b)).tolist()
        fs, fb = Fraction(s), Fraction(b)
        # over the common denominator q (a power of two: scaling a double by it is exact)
        # v * s + b = (v * ns + nb) / q; Python compares the int and the float exactly
        q = max(fs.denominator, fb.denominator)
        assert q & (q - 1) == 0 and fs == Fraction(fs * q, q) and (fs * q).denominator == (fb * q).denominator == 1
        ns, nb = int(fs * q), int(fb * q)
        for k, vk in enumerate(v.tolist()):
            assert got[k] * q == vk * ns + nb, (s, b, vk)


def test_library_exports_the_mbinfo_entry_points():
    from broadway_amd import _lib
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_mbinfo_device", 9), ("h264mi_engine_keep_records", 2),
                        ("h264mi_engine_forget_records", 3), ("h264mi_engine_export_mbinfo", 8),
                        ("H264SwDecKeepMbInfo", 2), ("H264SwDecLastPictureMbInfo", 4)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int bx, by, bw, bh, nch, dtype; int ch[16]; float scale[16], bias[16]; }
    D = _lib.MbInfoDesc
    assert C.sizeof(D) == 6 * 4 + 3 * 16 * 4
    assert [getattr(D, n).offset for n in ("bx", "by", "bw", "bh", "nch", "dtype")] == [0, 4, 8, 12, 16, 20]
    assert (D.ch.offset, D.scale.offset, D.bias.offset) == (24, 88, 152)
    assert _lib.TENSOR_I16 == 4 and _lib.MBINFO_MAX_CH == 16
    assert [_lib.MBINFO_CHANNELS[n] for n in M.CHANNELS] == list(range(9))


def test_decoder_option_validation():
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"window": (0, 0, 4, 4)}})           # the window is the crop window's blocks
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"channel": ("mvx",)}})
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"channels": ("mvx", "mvz")}})
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"channels": ()}})
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"dtype": np.int16}})
    with pytest.raises(ValueError):
        Decoder({"mbinfo": {"channels": ("mvx", "mvy"), "scale": (1.0, 2.0, 3.0)}})
    with pytest.raises(ValueError):                             # checked whatever the output mode
        Decoder({"mbinfo": {"channels": ("nope",)}, "rgb": True, "crop": True})


def test_mbinfo_desc_arguments():
    import torch
    from broadway_amd import _lib
    from broadway_amd.engine import mbinfo_desc
    d, n, dt = mbinfo_desc(("qp", "mvx", "qp"), (1, 2, 3, 4), torch.float16, scale=0.25, bias=(0.0, 1.0, 2.0))
    assert (n, dt) == (3, torch.float16) and (d.bx, d.by, d.bw, d.bh, d.nch, d.dtype) == (1, 2, 3, 4, 3, _lib.TENSOR_F16)
    assert list(d.ch)[:3] == [5, 0, 5] and list(d.scale)[:3] == [0.25] * 3 and list(d.bias)[:3] == [0.0, 1.0, 2.0]
    d, n, dt = mbinfo_desc("slice")
    assert (n, dt, d.bw, d.dtype) == (1, torch.int16, 0, _lib.TENSOR_I16) and d.ch[0] == 8 and d.scale[0] == 1.0
    assert mbinfo_desc(M.CHANNELS)[1] == 9
    for kw in (dict(channels=()), dict(channels=("mvx",) * 17), dict(channels=("MVX",)), dict(channels=(0,)),
               dict(channels=("mvx",), dtype=torch.uint8), dict(channels=("mvx",), dtype=torch.int32),
               dict(channels=("mvx", "mvy"), scale=(1.0,)), dict(channels=("mvx",), bias=(1.0, 2.0)),
               dict(channels=("mvx",), window=(0, 0, 4)), dict(channels=("mvx",), window=(0, 0, 0, 4)),
               dict(channels=("mvx",), window=(-1, 0, 4, 4))):
        with pytest.raises(ValueError):
            mbinfo_desc(**kw)


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


SIZES = {"1x1": (1, 1), "3x2": (3, 2), "5x3": (5, 3), "33x2": (33, 2)}      # MBs; 33x2: 132 columns, two workgroups a row
SENTINEL = 0xA5
FRONT = 64
ALL = list(range(9))


def windows(w, h):
    """The whole grid, one block, one starting and ending off MB boundaries,
    the last column, the last row, one whose row bytes are a multiple of 16
    for every element type (8 columns) and one for none (7 or 3 columns)."""
    BW, BH = 4 * w, 4 * h
    out = [(0, 0, BW, BH), (min(1, BW - 1), min(1, BH - 1), 1, 1), (BW - 1, 0, 1, BH), (0, BH - 1, BW, 1)]
    if BW > 5:
        out += [(3, 2, BW - 5, BH - 3), (1, 1, 8, BH - 2), (2, 0, 7, BH)]
    else:
        out += [(1, 0, 3, BH)]
    if BW > 128:
        out += [(1, 1, 128, 5), (3, 0, 129, 8)]         # a full workgroup part from inside an MB; one column more
    return out


@pytest.fixture(scope="module")
def synthetic():
    """size -> (3 record batches, their oracle fields) (read-only)"""
    rng = np.random.default_rng(29)
    out = {}
    for name, (w, h) in SIZES.items():
        recs = [M.synthetic_records(rng, w, h) for _ in range(3)]
        fields = [M.field(r, w, h) for r in recs]
        for f in fields:
            f.setflags(write=False)
        out[name] = (recs, fields)
    f = np.concatenate([f.reshape(9, -1) for fs in out.values() for f in fs[1]], axis=1)
    assert f[0].min() == -32768 and f[1].max() == 32767 and f[0].max() == 32767 and f[1].min() == -32768
    assert set(np.unique(f[4]).tolist()) == {-1, 0, 1, 2, 3, 4}
    return out


def make_desc(win, chans, dtype, consts="unit", nch=None):
    from broadway_amd import _lib
    d = _lib.MbInfoDesc()
    d.bx, d.by, d.bw, d.bh = win
    d.nch = len(chans) if nch is None else nch
    d.dtype = M.DTYPE_ID.get(dtype, dtype)
    d.ch[:len(chans)] = chans
    scale, bias = M.CONSTS[consts]
    d.scale[:] = scale
    d.bias[:] = bias
    return d


def run_mbinfo(recs, order, w, h, win, chans, dtype, consts="unit", in_pad=0, out_pad=0, skew=0, nch=None, npics=None,
               null=(), stride=None, offs=None, in_skew=0, dims=None):
    """h264mi_mbinfo_device over the batches `order` of `recs`; returns rc, the
    whole output buffer (FRONT + skew sentinel bytes, then pictures out_stride
    apart, then 64 sentinel bytes), the first picture's offset, out_stride and
    a picture's bytes."""
    import torch
    L = _mi()
    es = M.ELEM.get(dtype, 2)
    nbytes = max(len(chans), 1) * win[2] * win[3] * es if win[2] > 0 and win[3] > 0 else 16
    in_stride = len(recs[0]) + in_pad
    out_stride = nbytes + out_pad if stride is None else stride
    host = np.zeros(in_stride * len(recs) + 64, dtype=np.uint8)
    for k, r in enumerate(recs):
        host[k * in_stride:k * in_stride + len(r)] = np.frombuffer(r, dtype=np.uint8)
    d_in = torch.from_numpy(host).to("cuda")
    assert d_in.data_ptr() % 16 == 0
    n = len(order)
    offs = (C.c_size_t * n)(*([k * in_stride for k in order] if offs is None else offs))
    first = FRONT + skew
    d_out = torch.full((first + max(out_stride, nbytes) * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    desc = make_desc(win, chans, dtype, consts, nch)
    wm, hm = dims or (w, h)
    rc = L.h264mi_mbinfo_device(None if "in" in null else d_in.data_ptr() + in_skew, None if "offs" in null else offs,
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
    return ["unit"] if dtype == "int16" else sorted(M.CONSTS)       # int16 ignores scale and bias


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_kernel_vs_oracle(synthetic, size, dtype):
    """All nine channels over every window, with every constant set."""
    w, h = SIZES[size]
    recs, fields = synthetic[size]
    for win in windows(w, h):
        for consts in consts_of(dtype):
            rc, out, first, stride, nbytes = run_mbinfo(recs[:1], [0], w, h, win, ALL, dtype, consts)
            assert rc == 0, (win, consts)
            assert same(out[first:first + nbytes], M.expect(fields[0], ALL, win, dtype, consts)), (win, consts)
            assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (win, consts)


CHANNEL_LISTS = [[c] for c in ALL] + [ALL[::-1], [0, 1, 0, 5, 5, 2], [8] * 16]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("size", ["3x2", "5x3"])
def test_kernel_channel_lists(synthetic, size, dtype):
    """Each id alone, all nine reversed, lists with repeats (one of 16
    entries): the constants go with the channel position, not the id."""
    w, h = SIZES[size]
    recs, fields = synthetic[size]
    for chans in CHANNEL_LISTS:
        for win in ((0, 0, 4 * w, 4 * h), (3, 2, 4 * w - 5, 4 * h - 3)):
            rc, out, first, stride, nbytes = run_mbinfo(recs[1:2], [0], w, h, win, chans, dtype, "mixed")
            assert rc == 0, (chans, win)
            assert same(out[first:first + nbytes], M.expect(fields[1], chans, win, dtype, "mixed")), (chans, win)
            assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (chans, win)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("size", ["3x2", "5x3", "33x2"])
def test_kernel_batched_padded_strides_write_nothing_else(synthetic, size, dtype):
    """Picture list [2, 0, 2, 1] of three batches 96 pad bytes apart;
    out_stride padded by 5 elements (never a multiple of 16 bytes: the element
    path), by 48 bytes (16-byte rows keep the 16-byte stores) and by 48 bytes
    with d_out one element past a 16-byte boundary: every picture is right and
    no pad byte changes, the first one past each picture included."""
    w, h = SIZES[size]
    recs, fields = synthetic[size]
    es = M.ELEM[dtype]
    order = [2, 0, 2, 1]
    chans = [0, 1, 2]
    for win in [(0, 0, 4 * w, 4 * h), (1, 1, 8, 4 * h - 2), (3, 2, 4 * w - 5, 4 * h - 3)]:
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_mbinfo(recs, order, w, h, win, chans, dtype, "qpel", in_pad=96,
                                                        out_pad=out_pad, skew=skew)
            assert rc == 0, (win, out_pad, skew)
            assert (out[:first] == SENTINEL).all(), (win, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                assert same(out[o:o + nbytes], M.expect(fields[i], chans, win, dtype, "qpel")), (win, out_pad, skew, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (win, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (win, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_kernel_list_longer_than_one_launch(synthetic, dtype):
    w, h = SIZES["3x2"]
    recs, fields = synthetic["3x2"]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win = (3, 2, 7, 5)
    rc, out, first, stride, nbytes = run_mbinfo(recs, order, w, h, win, [1, 6], dtype, "mixed", in_pad=96)
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], M.expect(fields[i], [1, 6], win, dtype, "mixed")), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
def test_kernel_rejects_bad_arguments(synthetic):
    w, h = SIZES["3x2"]
    recs, _ = synthetic["3x2"]
    good = (1, 1, 4, 4)

    def refused(**kw):
        args = dict(win=good, chans=[0, 1], dtype="float16")
        args.update(kw)
        win, chans, dtype = args.pop("win"), args.pop("chans"), args.pop("dtype")
        rc, out, *_ = run_mbinfo(recs[:1], [0], w, h, win, chans, dtype, **args)
        assert rc == -1, kw
        assert (out == SENTINEL).all(), kw               # nothing was launched

    rc, out, first, _, nbytes = run_mbinfo(recs[:1], [0], w, h, good, [0, 1], "float16")
    assert rc == 0 and not (out[first:first + nbytes] == SENTINEL).all()        # the arguments below are one step away
    refused(nch=0)
    refused(nch=17)
    refused(nch=-1)
    for bad in (9, -1, 255):
        refused(chans=[0, bad])
    for dtype in (0, 5, -1):                             # uint8 and unknown types
        refused(dtype=dtype)
    for win in ((0, 0, 13, 8), (0, 0, 12, 9), (12, 0, 1, 1), (0, 8, 1, 1), (9, 0, 4, 1), (0, 6, 1, 3), (-1, 0, 4, 4),
                (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -4, 4)):
        refused(win=win)
    for null in ("in", "offs", "desc", "out"):
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


def tensor_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


def test_the_stream_exercises_the_field(captured):
    """What the engine and decoder tests below compare is not trivially zero."""
    cap, fields = captured
    f = np.stack(fields)
    assert (f[:, 0] != 0).any() and (f[:, 1] != 0).any()                    # a non-zero motion vector
    assert (f[:, 2] > 0).any()                                              # a reference index above 0
    assert {M.MBT_SKIP, M.MBT_I4x4, M.MBT_I16, M.MBT_INTER} <= set(np.unique(f[:, 4]).tolist())
    assert set(np.unique(f[:, 7]).tolist()) == {0, 1}                       # coded both ways
    assert len(np.unique(f[:, 8])) == 2                                     # two slices
    slots = [p.cur_slot for p in cap.pictures]
    assert len(set(slots)) < cap.npics and len(set(slots)) < cap.nslots    # a slot is reused, one never decoded into


@pytest.mark.gpu
def test_engine_keeps_records_per_slot(captured):
    """After each picture its slot's field is the oracle's over its records;
    at the end every slot holds the last picture decoded into it, the others
    "no information"; and retention changes no pixel."""
    import torch
    from broadway_amd.engine import Engine
    cap, fields = captured
    w, h = cap.w_mbs, cap.h_mbs
    plain = Engine(w, h, 1, cap.nslots)
    for pic in cap.pictures:
        plain.decode([0], [pic])
    want_pixels = [plain.read(0, s).tobytes() for s in range(cap.nslots)]
    with pytest.raises(RuntimeError):
        plain.to_mbinfo([0], [0])                       # retention is off
    with pytest.raises(RuntimeError):
        plain.forget_records(0, 0)
    plain.close()

    eng = Engine(w, h, 1, cap.nslots)
    eng.keep_records()
    side = torch.cuda.Stream()
    kinds = [("int16", "unit"), ("float16", "qpel"), ("float32", "mixed"), ("bfloat16", "mixed"), ("int16", "unit")]
    got, last = [], {}
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        dtype, consts = kinds[k % len(kinds)]
        scale, bias = M.CONSTS[consts]
        got.append(eng.to_mbinfo([0], [pic.cur_slot], channels=M.CHANNELS, dtype=getattr(torch, dtype), scale=scale[:9],
                                 bias=bias[:9], stream=side))
        last[pic.cur_slot] = k
    torch.cuda.synchronize()
    assert eng.errors() == 0
    whole = (0, 0, 4 * w, 4 * h)
    for k, t in enumerate(got):
        dtype, consts = kinds[k % len(kinds)]
        assert tuple(t.shape) == (1, 9, 4 * h, 4 * w) and t.dtype == getattr(torch, dtype) and t.is_cuda
        assert same(tensor_bytes(t), M.expect(fields[k], ALL, whole, dtype, consts)), k
    # every slot at once, with the default channels over a window
    win = CROP_BLOCKS
    t = eng.to_mbinfo([0] * cap.nslots, list(range(cap.nslots)), window=win)
    torch.cuda.synchronize()
    assert tuple(t.shape) == (cap.nslots, 2, win[3], win[2]) and t.dtype == torch.int16
    none = M.no_information(w, h)
    for s in range(cap.nslots):
        f = fields[last[s]] if s in last else none
        assert same(tensor_bytes(t[s]), M.expect(f, [0, 1], win, "int16")), s
    assert [eng.read(0, s).tobytes() for s in range(cap.nslots)] == want_pixels
    # forgetting a slot; a bad slot; switching off and on again starts empty
    s = cap.pictures[-1].cur_slot
    eng.forget_records(0, s)
    t = eng.to_mbinfo([0], [s], channels=M.CHANNELS)
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), M.expect(none, ALL, whole, "int16"))
    for kw in (dict(streams=[1], slots=[0]), dict(streams=[0], slots=[cap.nslots]),
               dict(streams=[0], slots=[0], window=(0, 0, 4 * w + 1, 1))):
        with pytest.raises(RuntimeError):
            eng.to_mbinfo(**kw)
    with pytest.raises(RuntimeError):
        eng.forget_records(0, cap.nslots)
    eng.keep_records(False)
    with pytest.raises(RuntimeError):
        eng.to_mbinfo([0], [s])
    eng.keep_records(True)
    t = eng.to_mbinfo([0], [cap.pictures[0].cur_slot], channels=M.CHANNELS)
    torch.cuda.synchronize()
    assert same(tensor_bytes(t), M.expect(none, ALL, whole, "int16"))
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
    eng.keep_records()
    out = torch.empty((1, 9, 4 * h, 4 * w), dtype=torch.int16, device="cuda")
    for k in range(k1):
        eng.decode([0], [cap.pictures[k]])
    assert eng.to_mbinfo([0], [slots[k0]], channels=M.CHANNELS, out=out) is out
    eng.decode([0], [cap.pictures[k1]])
    after = eng.to_mbinfo([0], [slots[k1]], channels=M.CHANNELS)
    torch.cuda.synchronize()
    whole = (0, 0, 4 * w, 4 * h)
    assert same(tensor_bytes(out), M.expect(fields[k0], ALL, whole, "int16"))
    assert same(tensor_bytes(after), M.expect(fields[k1], ALL, whole, "int16"))
    assert not np.array_equal(tensor_bytes(out), tensor_bytes(after))
    for bad in (torch.empty((1, 9, 4 * h, 4 * w + 1), dtype=torch.int16, device="cuda"),
                torch.empty((1, 9, 4 * h, 4 * w), dtype=torch.float16, device="cuda"),
                torch.empty((1, 9, 4 * h, 4 * w), dtype=torch.int16, device="cpu"),
                torch.empty((1, 9, 4 * w, 4 * h), dtype=torch.int16, device="cuda").transpose(2, 3)):
        with pytest.raises(ValueError):
            eng.to_mbinfo([0], [slots[k0]], channels=M.CHANNELS, out=bad)
    eng.close()


def decode_js(nals, opts):
    """(pictures, their mbinfo tensors, (w, h) per picture) of a Decoder run"""
    got, infos, dims = [], [], []
    dec = Decoder(opts)

    def on_picture(buf, w, h, _):
        # (a host picture is a view of the decoder's buffer: copied here; a tensor is the caller's)
        got.append(bytes(buf) if isinstance(buf, np.ndarray) else buf)
        infos.append(dec.mbinfo)
        dims.append((w, h))

    dec.onPictureDecoded = on_picture
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, infos, dims


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "tensor", "crop_rgb"])
def test_decoder_mbinfo_option(captured, mode):
    """decoder.mbinfo, set before each onPictureDecoded call, is the oracle's
    field of that picture over the blocks covering the crop window (this
    stream's output order is its decode order), whatever the output mode; and
    the pixels are those of the same run without ``mbinfo``."""
    import torch
    cap, fields = captured
    nals = split_annexb(case_stream())
    base = {"plain": {}, "tensor": {"tensor": True}, "crop_rgb": {"crop": True, "rgb": True}}[mode]
    want, none, wdims = decode_js(nals, base)
    assert none == [None] * len(want)
    got, infos, dims = decode_js(nals, dict(base, mbinfo=True))
    all9, infos9, _ = decode_js(nals, dict(base, mbinfo={"channels": M.CHANNELS, "dtype": torch.float32,
                                                          "scale": M.CONSTS["mixed"][0][:9],
                                                          "bias": M.CONSTS["mixed"][1][:9]}))
    assert len(got) == len(want) == len(all9) == cap.npics and dims == wdims
    bx, by, bw, bh = CROP_BLOCKS
    for k in range(cap.npics):
        if mode == "tensor":
            assert torch.equal(got[k], want[k]) and torch.equal(all9[k], want[k]), k
        else:
            assert got[k] == want[k] and all9[k] == want[k], k
        t = infos[k]
        assert tuple(t.shape) == (2, bh, bw) and t.dtype == torch.int16 and t.is_cuda, k
        assert same(tensor_bytes(t), M.expect(fields[k], [0, 1], CROP_BLOCKS, "int16")), k
        t = infos9[k]
        assert tuple(t.shape) == (9, bh, bw) and t.dtype == torch.float32, k
        assert same(tensor_bytes(t), M.expect(fields[k], ALL, CROP_BLOCKS, "float32", "mixed")), k


@pytest.mark.gpu
def test_swdec_last_picture_mbinfo_return_codes(captured):
    """H264SWDEC_OK before any picture; H264SWDEC_PARAM_ERR with retention
    never switched on and for what the export refuses; H264SWDEC_PIC_RDY and
    the field after a picture; a desc with its own window."""
    import torch
    from broadway_amd import _lib
    cap, fields = captured
    L = _mi()
    stream = case_stream()
    dst = torch.full((9 * 16 * 24 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
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

    whole = make_desc((0, 0, 0, 0), ALL, "int16")
    # retention never switched on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert first_picture(inst)
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    L.H264SwDecRelease(inst)
    # retention on
    inst = C.c_void_p()
    assert L.H264SwDecInit(C.byref(inst), 0) == _lib.H264SWDEC_OK
    assert L.H264SwDecKeepMbInfo(inst, 1) == _lib.H264SWDEC_OK
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_OK
    assert first_picture(inst)
    for bad in (make_desc((0, 0, 0, 0), ALL, "int16", nch=0), make_desc((0, 0, 0, 0), ALL, "int16", nch=17),
                make_desc((0, 0, 0, 0), [0, 9], "int16"), make_desc((0, 0, 0, 0), ALL, 0),
                make_desc((0, 0, 25, 1), ALL, "int16"), make_desc((0, 16, 1, 1), ALL, "int16"),
                make_desc((0, 0, 4, 0), ALL, "int16")):
        assert L.H264SwDecLastPictureMbInfo(inst, C.byref(bad), dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureMbInfo(inst, None, dst.data_ptr(), cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(whole), None, cur) == _lib.H264SWDEC_PARAM_ERR
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(whole), dst.data_ptr() + 1, cur) == _lib.H264SWDEC_PARAM_ERR
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()                       # nothing was queued
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(whole), dst.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    win = (3, 2, 7, 5)
    own = make_desc(win, [1, 6], "float16", "mixed")
    dst2 = torch.full((2 * 7 * 5 * 2 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert L.H264SwDecLastPictureMbInfo(inst, C.byref(own), dst2.data_ptr(), cur) == _lib.H264SWDEC_PIC_RDY
    torch.cuda.synchronize()
    n = 9 * CROP_BLOCKS[2] * CROP_BLOCKS[3] * 2
    got = dst.cpu().numpy()
    assert same(got[:n], M.expect(fields[0], ALL, CROP_BLOCKS, "int16")) and (got[n:] == SENTINEL).all()
    got = dst2.cpu().numpy()
    assert same(got[:140], M.expect(fields[0], [1, 6], win, "float16", "mixed")) and (got[140:] == SENTINEL).all()
    L.H264SwDecRelease(inst)
