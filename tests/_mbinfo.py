"""Helpers of tests/test_mbinfo.py: the field of motion vectors and MB side
information (include/h264mi.h, mbinfo.hip) restated in numpy over the raw bytes
of MbRec batches (include/h264mi_records.h), and the constant sets of the float
element types."""
import numpy as np

# struct MbRec, little endian, packed as the C compiler lays it out (no padding)
MBREC = np.dtype([("type", "u1"), ("qp", "u1"), ("qpc", "u1"), ("avail", "u1"), ("pred", "u1"), ("dbf", "u1"),
                  ("offA", "i1"), ("offB", "i1"), ("cbits", "<u4"), ("coef", "<u4"), ("i4", "u1", (8,)),
                  ("ref", "u1", (4,)), ("mv", "<i2", (16, 2)), ("slice", "<u2"), ("refidx", "<u2")])
assert MBREC.itemsize == 96

MBT_INTER, MBT_SKIP, MBT_I4x4, MBT_I16, MBT_IPCM, MBT_NONE = 0, 1, 2, 3, 4, 255
CHANNELS = ["mvx", "mvy", "ref_idx", "ref_slot", "mb_type", "qp", "intra_mode", "coded", "slice"]
DTYPES = ["int16", "float16", "bfloat16", "float32"]
DTYPE_ID = {"uint8": 0, "float16": 1, "bfloat16": 2, "float32": 3, "int16": 4}
ELEM = {"int16": 2, "float16": 2, "bfloat16": 2, "float32": 4}

# name -> (scale, bias) per channel position (16 each), fp32-representable
CONSTS = {
    "unit": ((1.0,) * 16, (0.0,) * 16),
    "qpel": ((0.25,) * 16, (0.0,) * 16),            # quarter-pel to pixels
    "mixed": (tuple([0.25, 0.25, 1.0, 0.5, 0.125, float(np.float32(1 / 51)), 2.0, 3.0][k % 8] for k in range(16)),
              tuple([0.0, 0.5, -1.0, 0.25, 1.0, -0.5, 0.0, 8.0][k % 8] for k in range(16))),
}


def zscan(x, y):
    """z-scan index of the 4x4 block at (x, y) inside its MB"""
    return (y >> 1) * 8 + (x >> 1) * 4 + (y & 1) * 2 + (x & 1)


def field(rec_bytes, w_mbs, h_mbs):
    """The nine channels over the whole block grid of one picture's record
    batch: (9, 4 * h_mbs, 4 * w_mbs) int64."""
    r = np.frombuffer(bytes(rec_bytes), dtype=MBREC)
    assert r.size == w_mbs * h_mbs
    BH, BW = 4 * h_mbs, 4 * w_mbs
    Y, X = np.mgrid[0:BH, 0:BW]
    m = (Y >> 2) * w_mbs + (X >> 2)
    b = zscan(X & 3, Y & 3)
    part = b >> 2
    t = r["type"][m].astype(np.int64)
    inter, skip, none = t == MBT_INTER, t == MBT_SKIP, t == MBT_NONE
    mc = inter | skip
    mv = r["mv"][m, b].astype(np.int64)                                  # (BH, BW, 2)
    refidx = (r["refidx"][m].astype(np.int64) >> (4 * part)) & 15
    i4 = (r["i4"][m, b >> 1].astype(np.int64) >> ((b & 1) * 4)) & 15
    out = np.empty((9, BH, BW), dtype=np.int64)
    out[0] = np.where(mc, mv[..., 0], 0)
    out[1] = np.where(mc, mv[..., 1], 0)
    out[2] = np.where(inter, refidx, np.where(skip, 0, -1))
    out[3] = np.where(mc, r["ref"][m, part].astype(np.int64), -1)
    out[4] = np.where(none, -1, t)
    out[5] = np.where(none, -1, r["qp"][m].astype(np.int64))
    out[6] = np.where(t == MBT_I4x4, i4, np.where(t == MBT_I16, 16 + (r["pred"][m].astype(np.int64) & 3), -1))
    out[7] = np.where(none, 0, (r["cbits"][m].astype(np.int64) >> b) & 1)
    out[8] = np.where(none, -1, r["slice"][m].astype(np.int64))
    return out


def no_information(w_mbs, h_mbs):
    """the field of a batch of 0xFF bytes"""
    return field(b"\xff" * (96 * w_mbs * h_mbs), w_mbs, h_mbs)


def select(f, chans, win):
    """channels `chans` (ids) of the window (bx, by, bw, bh) of field f"""
    bx, by, bw, bh = win
    return f[list(chans), by:by + bh, bx:bx + bw]


def convert(v, dtype, scale, bias):
    """The bytes of the tensor of values v (C, bh, bw) int64: int16 keeps the
    low 16 bits; the float types float64(v) * float64(scale) + float64(bias) --
    exact for the constant sets here (test_exactness_premise) --, rounded once
    to float32 (so: a hardware fma), then converted to the target type (numpy
    and torch round to nearest-even)."""
    if dtype == "int16":
        return np.ascontiguousarray((v & 0xFFFF).astype(np.uint16)).view(np.uint8).reshape(-1)
    n = v.shape[0]
    s = np.asarray(scale[:n], dtype=np.float32).astype(np.float64).reshape(n, 1, 1)
    b = np.asarray(bias[:n], dtype=np.float32).astype(np.float64).reshape(n, 1, 1)
    f = (v.astype(np.float64) * s + b).astype(np.float32)
    if dtype == "float32":
        out = f
    elif dtype == "float16":
        with np.errstate(over="ignore"):                # beyond 65504: infinity, as v_cvt_f16_f32 gives
            out = f.astype(np.float16)
    else:
        import torch
        return torch.from_numpy(f).to(torch.bfloat16).contiguous().view(torch.uint8).numpy().reshape(-1)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)


def expect(f, chans, win, dtype, consts="unit"):
    scale, bias = CONSTS[consts]
    return convert(select(f, chans, win), dtype, scale, bias)


def synthetic_records(rng, w_mbs, h_mbs):
    """Seeded random bytes with `type` drawn from {0, 1, 2, 3, 4, 255}: inter
    records keep random i4 bytes and intra records random mv / ref / refidx
    (what the type gating is tested with); the first two records carry the
    extreme motion vectors."""
    n = w_mbs * h_mbs
    r = np.frombuffer(rng.integers(0, 256, 96 * n, dtype=np.uint8).tobytes(), dtype=MBREC).copy()
    r["type"] = rng.choice(np.array([0, 1, 2, 3, 4, 255], dtype=np.uint8), n)
    r["type"][0] = MBT_INTER
    r["mv"][0, :, 0] = -32768
    r["mv"][0, :, 1] = 32767
    if n > 1:
        r["type"][1] = MBT_SKIP
        r["mv"][1, ::2] = (32767, -32768)
    return r.tobytes()
