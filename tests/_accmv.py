"""Helpers of tests/test_accmv.py: the accumulated motion (include/h264mi.h,
accmv.hip) restated in numpy over the raw bytes of MbRec batches -- one step of
an origin map, the export channels, the engine's chain under its serial rule --
and a per-sample trace written out by hand to check the vectorised step with."""
import numpy as np

from _mbinfo import MBREC, MBT_SKIP, zscan

CHANNELS = ["adx", "ady", "jx", "jy", "anchored"]
ANCHORED = 1 << 31


def pack(jx, jy, anchored):
    """origin-map words: JX | JY << 16 | ANCHORED << 31"""
    return (np.asarray(jx).astype(np.uint32) | np.asarray(jy).astype(np.uint32) << np.uint32(16) |
            np.uint32(ANCHORED if anchored else 0))


def identity(w_mbs, h_mbs, anchored):
    """(x, y, anchored) for every sample: a key picture (1), a slot without a map (0)"""
    Y, X = np.mgrid[0:16 * h_mbs, 0:16 * w_mbs]
    return pack(X, Y, anchored)


def is_key(rec_bytes):
    """a picture without a single MBT_INTER / MBT_SKIP record"""
    return not (np.frombuffer(bytes(rec_bytes), dtype=MBREC)["type"] <= MBT_SKIP).any()


def step(rec_bytes, w_mbs, h_mbs, refs, key=False, stats=None):
    """One step: the (H, W) uint32 map of the picture with records `rec_bytes`
    from refs[s], an (H, W) uint32 map or None per slot.  `stats`: a dict that
    receives the share of samples with a clamped source, the slots read through
    a map, and -- given refs' hop counts in stats["hops_in"] -- the hop counts."""
    W, H = 16 * w_mbs, 16 * h_mbs
    Y, X = np.mgrid[0:H, 0:W]
    if key:
        if stats is not None:
            stats.update(clamped=0.0, slots=set(), hops=np.zeros((H, W), dtype=np.int64))
        return pack(X, Y, 1)
    r = np.frombuffer(bytes(rec_bytes), dtype=MBREC)
    assert r.size == w_mbs * h_mbs
    m = (Y >> 4) * w_mbs + (X >> 4)
    b = zscan((X >> 2) & 3, (Y >> 2) & 3)
    inter = r["type"][m] <= MBT_SKIP
    d = (r["mv"][m, b].astype(np.int64) + 2) >> 2                       # integer-pel, round half up
    ux, uy = X + d[..., 0], Y + d[..., 1]
    qx, qy = np.clip(ux, 0, W - 1), np.clip(uy, 0, H - 1)
    s = r["ref"][m, b >> 2].astype(np.int64)
    out = np.where(inter, pack(qx, qy, 0), pack(X, Y, 0))
    hops = np.zeros((H, W), dtype=np.int64)
    read = set()
    for si, M in enumerate(refs):
        if M is None:
            continue
        sel = inter & (s == si)
        out[sel] = M[qy[sel], qx[sel]]
        if sel.any():
            read.add(si)
        if stats is not None and stats.get("hops_in") is not None:
            hops[sel] = stats["hops_in"][si][qy[sel], qx[sel]] + 1
    if stats is not None:
        stats.update(clamped=float((inter & ((qx != ux) | (qy != uy))).mean()), slots=read, hops=hops)
    return out


def channels(M):
    """the five channels of map M over the whole picture: (5, H, W) int64"""
    H, W = M.shape
    Y, X = np.mgrid[0:H, 0:W]
    jx, jy = (M & 0x7FFF).astype(np.int64), ((M >> 16) & 0x7FFF).astype(np.int64)
    return np.stack([jx - X, jy - Y, jx, jy, (M >> 31).astype(np.int64)])


def select(f, chans, win):
    """channels `chans` (ids) of the window (x, y, cw, ch) of channels(M)"""
    x, y, cw, ch = win
    return f[list(chans), y:y + ch, x:x + cw]


def trace(x, y, t, pictures, w_mbs, h_mbs):
    """(JX, JY, ANCHORED) of sample (x, y) of picture t, followed hop by hop.
    pictures[t] = (MBREC array, key, {slot: index of the picture whose map the
    slot holds}); a slot missing from the dict has no map."""
    W, H = 16 * w_mbs, 16 * h_mbs
    while True:
        r, key, refs = pictures[t]
        if key:
            return x, y, 1
        rec = r[(y >> 4) * w_mbs + (x >> 4)]
        if rec["type"] > MBT_SKIP:
            return x, y, 0
        bx, by = (x >> 2) & 3, (y >> 2) & 3
        b = (by >> 1) * 8 + (bx >> 1) * 4 + (by & 1) * 2 + (bx & 1)
        dx, dy = (int(rec["mv"][b][0]) + 2) >> 2, (int(rec["mv"][b][1]) + 2) >> 2
        x, y = min(max(x + dx, 0), W - 1), min(max(y + dy, 0), H - 1)
        s = int(rec["ref"][b >> 2])
        if s not in refs:
            return x, y, 0
        t = refs[s]


class Chain:
    """The engine's retention for one stream (include/h264mi.h,
    h264mi_engine_keep_accmv): per slot a map and the key serial it was written
    under; a slot counts as a reference iff its serial is the current one; the
    slot being written counts as none."""

    def __init__(self, w_mbs, h_mbs, nslots):
        self.w, self.h, self.nslots = w_mbs, h_mbs, nslots
        self.maps = [identity(w_mbs, h_mbs, 0) for _ in range(nslots)]
        self.hops = [np.zeros((16 * h_mbs, 16 * w_mbs), dtype=np.int64) for _ in range(nslots)]
        self.ser = [0] * nslots
        self.key = 0
        self.stats = []             # per decoded picture: dict(key, clamped, slots, unanchored, max_hops)

    def decode(self, rec_bytes, slot):
        key = is_key(rec_bytes)
        if key:
            self.key += 1
        usable = [s != slot and self.key > 0 and self.ser[s] == self.key for s in range(self.nslots)]
        st = {"hops_in": self.hops}
        M = step(rec_bytes, self.w, self.h, [self.maps[s] if usable[s] else None for s in range(self.nslots)], key, st)
        self.maps[slot], self.hops[slot], self.ser[slot] = M, st["hops"], self.key
        self.stats.append(dict(key=key, clamped=st["clamped"], slots=st["slots"],
                               unanchored=float(((M >> 31) == 0).mean()), max_hops=int(st["hops"].max())))
        return M

    def forget(self, slot):
        self.maps[slot] = identity(self.w, self.h, 0)
        self.hops[slot] = np.zeros_like(self.hops[slot])
        self.ser[slot] = 0
