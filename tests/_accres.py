"""Helpers of tests/test_accres.py: the accumulated residual (include/h264mi.h,
accres.hip) restated in numpy over frame bytes in the engine's slot layout and
origin-map words (tests/_accmv.py's layout), with tests/_mbinfo.py's element
conversions and tests/_colour.py's rgb_of; and the classification of an
export's groups of four elements into the kernel's two gather paths."""
import numpy as np

import _accmv as A
import _colour as COL
import _mbinfo as M

PLANES = {"y": 0, "uv": 1, "yuv": 2, "rgb": 3}
NPLANES = {"y": 1, "uv": 2, "yuv": 3, "rgb": 3}
POLICY = {"key": 0, "zero": 1}


def cpitch(w_mbs):
    return (8 * w_mbs + 127) & ~127


def slot_bytes(w_mbs, h_mbs):
    return 256 * w_mbs * h_mbs + 2 * cpitch(w_mbs) * 8 * h_mbs


def split(frame, w_mbs, h_mbs):
    """(Y, Cb, Cr) views of a frame in the slot layout (chroma rows cpitch apart)"""
    f = np.frombuffer(bytes(frame), dtype=np.uint8) if not isinstance(frame, np.ndarray) else frame.reshape(-1)
    W, H, cp = 16 * w_mbs, 16 * h_mbs, cpitch(w_mbs)
    assert f.size == slot_bytes(w_mbs, h_mbs)
    y = f[:W * H].reshape(H, W)
    cb = f[W * H:W * H + cp * H // 2].reshape(H // 2, cp)[:, :W // 2]
    cr = f[W * H + cp * H // 2:].reshape(H // 2, cp)[:, :W // 2]
    return y, cb, cr


def from_packed(i420, w_mbs, h_mbs, pad=0):
    """a packed I420 picture (Engine.read) as a frame in the slot layout"""
    a = np.frombuffer(bytes(i420), dtype=np.uint8) if not isinstance(i420, np.ndarray) else i420.reshape(-1)
    W, H, cp = 16 * w_mbs, 16 * h_mbs, cpitch(w_mbs)
    f = np.full(slot_bytes(w_mbs, h_mbs), pad, dtype=np.uint8)
    f[:W * H] = a[:W * H]
    c = W * H // 4
    f[W * H:W * H + cp * H // 2].reshape(H // 2, cp)[:, :W // 2] = a[W * H:W * H + c].reshape(H // 2, W // 2)
    f[W * H + cp * H // 2:].reshape(H // 2, cp)[:, :W // 2] = a[W * H + c:W * H + 2 * c].reshape(H // 2, W // 2)
    return f


def origins(m, W, H):
    """(jx, jy, anchored) of map words, clamped to the picture"""
    jx = np.minimum((m & 0x7FFF).astype(np.int64), W - 1)
    jy = np.minimum(((m >> 16) & 0x7FFF).astype(np.int64), H - 1)
    return jx, jy, (m >> 31).astype(np.int64)


def field(cur, key, m, w_mbs, h_mbs, planes, policy="key", colour=0):
    """The planes over the whole picture: (1 | 2 | 3, rows, columns) int64 of
    frame `cur` against frame `key` (None: no key) through map m (H, W)."""
    W, H = 16 * w_mbs, 16 * h_mbs
    hs = 1 if planes == "uv" else 0
    if key is None:
        return np.zeros((NPLANES[planes], H >> hs, W >> hs), dtype=np.int64)
    cy, cb, cr = (p.astype(np.int64) for p in split(cur, w_mbs, h_mbs))
    ky, kb, kr = (p.astype(np.int64) for p in split(key, w_mbs, h_mbs))
    if planes == "uv":
        jx, jy, a = origins(m[::2, ::2], W, H)
        v = np.stack([cb - kb[jy >> 1, jx >> 1], cr - kr[jy >> 1, jx >> 1]])
    else:
        jx, jy, a = origins(m, W, H)
        Y, X = np.mgrid[0:H, 0:W]
        if planes == "y":
            v = (cy - ky[jy, jx])[None]
        elif planes == "yuv":
            v = np.stack([cy - ky[jy, jx], cb[Y >> 1, X >> 1] - kb[jy >> 1, jx >> 1],
                          cr[Y >> 1, X >> 1] - kr[jy >> 1, jx >> 1]])
        else:
            c = COL.rgb_of(cy, cb[Y >> 1, X >> 1], cr[Y >> 1, X >> 1], colour)
            k = COL.rgb_of(ky[jy, jx], kb[jy >> 1, jx >> 1], kr[jy >> 1, jx >> 1], colour)
            v = np.stack([c[i] - k[i] for i in range(3)])
    if policy == "zero":
        v = np.where(a[None] == 1, v, 0)
    return v


def select(v, win, planes):
    x, y, cw, ch = win
    hs = 1 if planes == "uv" else 0
    return v[:, y >> hs:(y + ch) >> hs, x >> hs:(x + cw) >> hs]


def expect(cur, key, m, w_mbs, h_mbs, win, planes, dtype, policy="key", colour=0, consts="unit"):
    scale, bias = M.CONSTS[consts]
    return M.convert(select(field(cur, key, m, w_mbs, h_mbs, planes, policy, colour), win, planes), dtype, scale, bias)


def gather_paths(m, w_mbs, h_mbs, win, planes):
    """How k_accres gathers the window's groups of four consecutive elements of
    an output row (the 16-byte path; the window's output width is a multiple of
    4): a group whose origins lie in one row of the plane at consecutive columns
    is a run, one fetch -- from which byte offset 0..3, and whether it crosses
    into a second dword --, every other group is four byte loads.  Returns
    dict(runs, singles, offsets=set, crossing, at_end) where at_end counts the
    runs that end on the last sample of the plane."""
    W, H = 16 * w_mbs, 16 * h_mbs
    x, y, cw, ch = win
    hs = 1 if planes == "uv" else 0
    mm = m[y:y + ch:1 + hs, x:x + cw:1 + hs]
    assert mm.shape[1] % 4 == 0
    jx, jy, _ = origins(mm, W, H)
    gx, gy = (jx >> hs).reshape(mm.shape[0], -1, 4), (jy >> hs).reshape(mm.shape[0], -1, 4)
    run = (gy == gy[..., :1]).all(-1) & (gx == gx[..., :1] + np.arange(4)).all(-1)
    x0, y0 = gx[..., 0][run], gy[..., 0][run]
    return dict(runs=int(run.sum()), singles=int((~run).sum()), offsets=set((x0 & 3).tolist()),
                crossing=int(((x0 & 3) != 0).sum()),
                at_end=int(((x0 + 3 == (W >> hs) - 1) & (y0 == (H >> hs) - 1)).sum()))


def planted_map(rng, w_mbs, h_mbs):
    """An identity map with random ANCHORED bits and planted groups (every size
    from 1 x 1 MB on has room for them):
      row 1, columns 4 o .. 4 o + 3, o = 0..3: a luma run from key column o of key row 5;
      row 2, columns 0..3: the last four samples of the key's last row (the last byte of Y, and of Cb and Cr);
             columns 4..7: the same one column to the left;
      row 4, even columns 0..6: key columns W - 8 .. W - 2 of its last row -- a UV run that ends on the last byte of
             Cb and Cr; even columns 8..14: a UV run from chroma column 1;
      row 6, even columns 0..6 / 8..14: UV runs from chroma columns 2 / 3 of chroma row 4;
      row 8, columns 0..3: JX = 0x7FFF; 4..7: JY = 0x7FFF with consecutive JX; 8: JX = W; 9: JY = H; 10: both."""
    W, H = 16 * w_mbs, 16 * h_mbs
    Y, X = np.mgrid[0:H, 0:W]
    m = A.pack(X, Y, 0) | (rng.integers(0, 2, (H, W)).astype(np.uint32) << np.uint32(31))
    top = m & np.uint32(1 << 31)

    def put(y, x, jx, jy):
        m[y, x] = np.uint32(jx) | np.uint32(jy) << np.uint32(16) | top[y, x]

    for o in range(4):
        for k in range(4):
            put(1, 4 * o + k, o + k, 5)
    for k in range(4):
        put(2, k, W - 4 + k, H - 1)
        put(2, 4 + k, W - 5 + k, H - 1)
        put(4, 2 * k, W - 8 + 2 * k, H - 1)
        put(4, 2 * k + 1, 0, 0)
        put(4, 8 + 2 * k, 2 * (1 + k) + 1, 6)
        put(6, 2 * k, 2 * (2 + k), 9)
        put(6, 8 + 2 * k, 2 * (3 + k) + 1, 8)
        put(8, k, 0x7FFF, 3)
        put(8, 4 + k, 2 + k, 0x7FFF)
    put(8, 8, W, 2)
    put(8, 9, 2, H)
    put(8, 10, 0x7FFF, 0x7FFF)
    return m
