"""Helpers of tests/test_residual.py: the decoded residual (include/h264mi.h,
residual.hip) restated in numpy over the raw bytes of MbRec batches and
coefficient pools (include/h264mi_records.h) -- dequantisation, the two DC
transforms and the 4x4 inverse transform in int64, then the clamp -- and the
constant sets of the float element types."""
import numpy as np

from _mbinfo import (DTYPE_ID, DTYPES, ELEM, MBREC, MBT_I4x4, MBT_I16, MBT_INTER, MBT_IPCM, MBT_NONE,  # noqa: F401
                     MBT_SKIP, convert)

PLANES = {"y": 0, "uv": 1, "yuv": 2}
NPLANES = {"y": 1, "uv": 2, "yuv": 3}

# name -> (scale, bias) per plane position, fp32-representable
_N = float(np.float32(1 / 255))
CONSTS = {
    "unit": ((1.0,) * 3, (0.0,) * 3),
    "norm": ((_N,) * 3, (0.0,) * 3),                    # samples to [-2, 2]: what the models take
    "mixed": ((0.5, _N, 2.0), (0.25, -0.5, 8.0)),
}

# LevelScale(qp % 6, position class): both coordinates even, both odd, mixed
LEVEL_SCALE = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)         # raster position of scan position s
BLK_X = tuple(((b >> 2) & 1) * 2 + (b & 1) for b in range(16))          # z-scan block -> column, row inside its MB
BLK_Y = tuple(((b >> 3) & 1) * 2 + ((b >> 1) & 1) for b in range(16))

# the largest magnitude any intermediate of the functions below has taken
# (test_no_intermediate_leaves_int32 resets and reads it)
peak = [0]


def _seen(*xs):
    for x in xs:
        peak[0] = max(peak[0], int(np.abs(np.asarray(x, dtype=np.int64)).max()))
    return xs[0]


def _cls(rr):
    x, y = rr & 3, rr >> 2
    return 0 if not (x & 1) and not (y & 1) else 1 if (x & 1) and (y & 1) else 2


def dequant(levels, qp, skip0):
    """16 levels in scan order -> 16 raster coefficients (position 0 left 0 when skip0)"""
    d = np.zeros(16, dtype=np.int64)
    for s in range(1 if skip0 else 0, 16):
        rr = ZIGZAG[s]
        d[rr] = int(levels[s]) * (LEVEL_SCALE[qp % 6][_cls(rr)] << (qp // 6))
    return _seen(d)


def luma_dc(levels, qp):
    """the I16 luma-DC transform of 16 levels in scan order: (4, 4), [row, column] of the MB's blocks"""
    c = np.zeros(16, dtype=np.int64)
    for s in range(16):
        c[ZIGZAG[s]] = int(levels[s])
    a = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)
    f = _seen(a @ _seen(a @ c.reshape(4, 4)).T).T           # rows, then columns
    x = _seen(f * LEVEL_SCALE[qp % 6][0])
    q6 = qp // 6
    return _seen(x << (q6 - 2)) if q6 >= 2 else (_seen((x << q6) + 2) >> 2)


def chroma_dc(c, qpc):
    """the chroma-DC transform of one plane's 4 levels: its blocks 0..3"""
    c0, c1, c2, c3 = (int(v) for v in c[:4])
    f = np.array([c0 + c1 + c2 + c3, c0 - c1 + c2 - c3, c0 + c1 - c2 - c3, c0 - c1 - c2 + c3], dtype=np.int64)
    return _seen(_seen(f * LEVEL_SCALE[qpc % 6][0]) << (qpc // 6)) >> 1


def inverse4x4(d):
    """16 raster coefficients -> (4, 4) samples, (x + 32) >> 6, clamped to int16"""
    d = np.asarray(d, dtype=np.int64).reshape(4, 4)
    t = np.empty((4, 4), dtype=np.int64)
    for i in range(4):
        a, b = d[i, 0] + d[i, 2], d[i, 0] - d[i, 2]
        c, e = (d[i, 1] >> 1) - d[i, 3], d[i, 1] + (d[i, 3] >> 1)
        t[i] = _seen(np.array([a + e, b + c, b - c, a - e]), np.array([a, b, c, e]))
    o = np.empty((4, 4), dtype=np.int64)
    for j in range(4):
        a, b = t[0, j] + t[2, j], t[0, j] - t[2, j]
        c, e = (t[1, j] >> 1) - t[3, j], t[1, j] + (t[3, j] >> 1)
        o[:, j] = _seen(np.array([a + e + 32, b + c + 32, b - c + 32, a - e + 32]), np.array([a, b, c, e])) >> 6
    return np.clip(o, -32768, 32767)


def res_mask(mb_type, cbits):
    m = cbits & 0xFFFFFF
    if mb_type == MBT_I16 and (cbits >> 24) & 1:
        m |= 0xFFFF
    if (cbits >> 25) & 1:
        m |= 0xF0000
    if (cbits >> 26) & 1:
        m |= 0xF00000
    return m


def _popcount(v):
    return bin(v).count("1")


def mb_residual(r, pool, coef_base=0, coef_blocks=None):
    """(Y (16, 16), Cb (8, 8), Cr (8, 8)) int64 of record r over the pool
    ((n, 16) int16 blocks), of which the first coef_blocks count"""
    y, cb_, cr = np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)
    t, cbits = int(r["type"]), int(r["cbits"])
    if t not in (MBT_INTER, MBT_I4x4, MBT_I16):
        return y, cb_, cr
    first = coef_base + int(r["coef"])
    nblk = len(pool) if coef_blocks is None else coef_blocks
    if first + _popcount(cbits & 0x7FFFFFF) > nblk:
        return y, cb_, cr
    m = res_mask(t, cbits)

    def block(bit):
        return pool[first + _popcount(cbits & ((1 << bit) - 1))].astype(np.int64)

    i16 = t == MBT_I16
    ldc = luma_dc(block(24), int(r["qp"])) if i16 and (cbits >> 24) & 1 else np.zeros((4, 4), np.int64)
    cdc = [chroma_dc(block(25 + k), int(r["qpc"])) if (cbits >> (25 + k)) & 1 else np.zeros(4, np.int64)
           for k in range(2)]
    for b in range(24):
        if not (m >> b) & 1:
            continue
        luma = b < 16
        qp = int(r["qp"]) if luma else int(r["qpc"])
        d = dequant(block(b), qp, not luma or i16) if (cbits >> b) & 1 else np.zeros(16, np.int64)
        if luma:
            if i16:
                d[0] = ldc[BLK_Y[b], BLK_X[b]]
            y[4 * BLK_Y[b]:4 * BLK_Y[b] + 4, 4 * BLK_X[b]:4 * BLK_X[b] + 4] = inverse4x4(d)
        else:
            k, c = (b - 16) >> 2, b & 3
            d[0] = cdc[k][c]
            (cb_, cr)[k][4 * (c >> 1):4 * (c >> 1) + 4, 4 * (c & 1):4 * (c & 1) + 4] = inverse4x4(d)
    return y, cb_, cr


def field(rec_bytes, coef_bytes, w_mbs, h_mbs, coef_base=0, coef_blocks=None):
    """The three planes of one picture: (Y (16h, 16w), Cb (8h, 8w), Cr (8h, 8w)) int64"""
    r = np.frombuffer(bytes(rec_bytes), dtype=MBREC)
    assert r.size == w_mbs * h_mbs
    pool = np.frombuffer(bytes(coef_bytes), dtype="<i2").reshape(-1, 16)
    y = np.zeros((16 * h_mbs, 16 * w_mbs), np.int64)
    cb, cr = np.zeros((8 * h_mbs, 8 * w_mbs), np.int64), np.zeros((8 * h_mbs, 8 * w_mbs), np.int64)
    for m in range(r.size):
        my, mx = divmod(m, w_mbs)
        a, b, c = mb_residual(r[m], pool, coef_base, coef_blocks)
        y[16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = a
        cb[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = b
        cr[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = c
    return y, cb, cr


def zero_field(w_mbs, h_mbs):
    return (np.zeros((16 * h_mbs, 16 * w_mbs), np.int64), np.zeros((8 * h_mbs, 8 * w_mbs), np.int64),
            np.zeros((8 * h_mbs, 8 * w_mbs), np.int64))


def select(f, planes, win):
    """the planes of the window (x, y, cw, ch), in luma samples, of field f: (1 | 2 | 3, rows, columns)"""
    x, y, cw, ch = win
    yy, cb, cr = f
    if planes == "y":
        return yy[None, y:y + ch, x:x + cw]
    if planes == "uv":
        assert not (x | y | cw | ch) & 1
        return np.stack([p[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2] for p in (cb, cr)])
    Y, X = np.mgrid[y:y + ch, x:x + cw]
    return np.stack([yy[y:y + ch, x:x + cw], cb[Y >> 1, X >> 1], cr[Y >> 1, X >> 1]])


def expect(f, planes, win, dtype, consts="unit"):
    scale, bias = CONSTS[consts]
    return convert(select(f, planes, win), dtype, scale, bias)


def synthetic_batch(rng, w_mbs, h_mbs):
    """(record bytes, pool bytes): seeded random records with `type` drawn
    from {0, 1, 2, 3, 4, 255}, qp and qpc from 0..51, random cbits (27 bits) for
    every type -- skip, I_PCM and type-255 records keep them, and skip and
    type-255 records a random coef: what the type gating is tested with -- and
    consistent coef indices for the others; an I_PCM MB owns 12 pool blocks of
    random bytes.  Levels: |level| <= 2047 (test_no_intermediate_leaves_int32),
    mostly small and sparse, some blocks large enough to leave [-512, 511] and
    to hit the clamp."""
    n = w_mbs * h_mbs
    r = np.frombuffer(rng.integers(0, 256, 96 * n, dtype=np.uint8).tobytes(), dtype=MBREC).copy()
    r["type"] = rng.choice(np.array([0, 1, 2, 3, 4, 255], dtype=np.uint8), n)
    r["type"][0] = MBT_I16
    r["qp"] = rng.integers(0, 52, n)
    r["qpc"] = rng.integers(0, 52, n)
    r["cbits"] = rng.integers(0, 1 << 27, n)
    r["cbits"][0] |= 7 << 24
    blocks = [rng.integers(-32768, 32768, (3, 16))]         # (three blocks no record owns)
    nblk = 3
    for m in range(n):
        t = int(r["type"][m])
        if t in (MBT_SKIP, MBT_NONE):
            continue
        r["coef"][m] = nblk
        if t == MBT_IPCM:
            k = 12
            blocks.append(rng.integers(-32768, 32768, (k, 16)))
        else:
            k = _popcount(int(r["cbits"][m]) & 0x7FFFFFF)
            kind = rng.choice(3, k, p=[0.6, 0.25, 0.15])
            bound = np.array([3, 64, 2047])[kind][:, None]
            lv = rng.integers(-bound, bound + 1, (k, 16))
            lv[rng.random((k, 16)) < 0.5] = 0
            blocks.append(lv)
        nblk += k
    pool = np.concatenate(blocks).astype("<i2")
    assert len(pool) == nblk
    return r.tobytes(), pool.tobytes()
