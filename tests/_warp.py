"""The oracle of the affine-warped tensor export: the definition
of include/h264mi.h restated in Python / numpy int64 on top of what the other
exports' tests pin already -- _tensor.samples (the reference converter's R, G,
B, or luma), _colour.samples_colour (sets 1..3) and _tensor.convert (the
elements).  warped tensor == convert(warp(samples(window)))."""
import functools

import numpy as np

import _colour as K
import _crop
import _tensor as T

CONSTANT, REPLICATE = 0, 1
IDENTITY = (65536, 0, 0, 0, 65536, 0)


def axis(P, n):
    """(first tap, fraction) of the Q16 positions P (int64 array or Python
    int) on an axis of n samples; the first tap saturated to [-2, n]."""
    r = (P + 128) >> 8                  # arithmetic: floor
    q = r >> 8
    f = r & 255
    if isinstance(q, np.ndarray):
        return np.clip(q, -2, n), f
    return min(max(q, -2), n), f


def taps_one(m, i, j, cw, ch, border):
    """warp_taps (common/warp_geom.h) in Python integers: (fx, fy, x0, x1, y0,
    y1, mask) of output (i, j)."""
    x0, fx = axis(m[0] * j + m[1] * i + m[2], cw)
    y0, fy = axis(m[3] * j + m[4] * i + m[5], ch)
    mx = (1 if 0 <= x0 < cw else 0) | (2 if 0 <= x0 + 1 < cw else 0)
    my = (1 if 0 <= y0 < ch else 0) | (2 if 0 <= y0 + 1 < ch else 0)
    mask = 15 if border == REPLICATE else (mx if my & 1 else 0) | (mx << 2 if my & 2 else 0)
    cl = lambda v, n: min(max(v, 0), n - 1)         # noqa: E731
    return fx, fy, cl(x0, cw), cl(x0 + 1, cw), cl(y0, ch), cl(y0 + 1, ch), mask


def warp_planes(c, m, size, border=CONSTANT, pad=(0, 0, 0)):
    """(planes, oh, ow) uint8: the samples c (planes, ch, cw) warped by the six
    Q16 integers m -- the definition, tap by tap."""
    planes, ch, cw = c.shape
    oh, ow = size
    m = [int(v) for v in m]
    assert all(-2 ** 31 <= v < 2 ** 31 for v in m)
    i = np.arange(oh, dtype=np.int64).reshape(oh, 1)
    j = np.arange(ow, dtype=np.int64).reshape(1, ow)
    x0, fx = axis(m[0] * j + m[1] * i + m[2], cw)
    y0, fy = axis(m[3] * j + m[4] * i + m[5], ch)
    c = c.astype(np.int64)
    acc = np.full((planes, oh, ow), 32768, dtype=np.int64)
    padv = np.asarray(pad[:planes], dtype=np.int64).reshape(planes, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            inside = (x >= 0) & (x < cw) & (y >= 0) & (y < ch)
            s = c[:, np.clip(y, 0, ch - 1), np.clip(x, 0, cw - 1)]
            if border == CONSTANT:
                s = np.where(inside[None], s, padv)
            acc += ((fx if dx else 256 - fx) * (fy if dy else 256 - fy))[None] * s
    v = acc >> 16
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def window_samples(i420, cw, ch, mode, colour=0):
    """(planes, ch, cw) uint8 samples of a cropped packed I420 window."""
    if mode == "rgb" and colour:
        return K.samples_colour(i420, cw, ch, colour)
    return T.samples(i420, cw, ch, mode)


_PICS = {}


@functools.lru_cache(maxsize=None)
def _samples_cached(key, w, h, cp, win, mode, colour):
    x, y, cw, ch = win
    s = window_samples(_crop.crop_i420(_PICS[key], w, h, x, y, cw, ch, cpitch=cp), cw, ch, mode, colour)
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


def elements(v, dtype, consts, hwc=False):
    """The bytes of the warped samples v (planes, oh, ow): _tensor.convert's
    elements, interleaved (oh, ow, planes) with hwc."""
    scale, bias = T.CONSTS[consts]
    if not hwc or v.shape[0] == 1:
        return T.convert(v, dtype, scale, bias)
    es = T.ELEM[dtype]
    planar = T.convert(v, dtype, scale, bias).reshape(v.shape[0], v.shape[1], v.shape[2], es)
    return np.ascontiguousarray(planar.transpose(1, 2, 0, 3)).reshape(-1)


def expect(pic, w, h, cp, win, m, size, mode, dtype, consts="unit", colour=0, border=CONSTANT, pad=(0, 0, 0), hwc=False):
    """Bytes the warp m of window `win` of `pic` (chroma rows cp apart) holds.
    The window's samples are computed once per (picture, window, mode, set)."""
    key = id(pic)
    _PICS[key] = pic
    c = _samples_cached(key, w, h, cp, tuple(win), mode, colour)
    return elements(warp_planes(c, m, size, border, pad), dtype, consts, hwc)


def frame_expect(frame, w, h, win, m, size, mode, dtype, consts="unit", colour=0, border=CONSTANT, pad=(0, 0, 0)):
    """The same for a decoded packed frame (not cached)."""
    x, y, cw, ch = win
    c = window_samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode, colour)
    return elements(warp_planes(c, m, size, border, pad), dtype, consts)


# ---- the digest tests/warp_geom_check.c prints ---------------------------------
SPECIAL = (0, 1, -1, 65535, -65535, 65536, -65536, 1 << 24, -(1 << 24), -2 ** 31, 2 ** 31 - 1)
MASK64 = (1 << 64) - 1


class Rng:
    """xorshift64* (Vigna): the check program's generator."""

    def __init__(self, seed):
        self.s = seed

    def next(self):
        s = self.s
        s ^= s >> 12
        s ^= (s << 25) & MASK64
        s ^= s >> 27
        self.s = s
        return ((s * 0x2545F4914F6CDD1D) & MASK64) >> 32

    def coef(self):
        """A coefficient: one of SPECIAL, any int32, or within +-2^18 (scales near 1)."""
        kind = self.next() % 3
        v = self.next()
        if kind == 0:
            return SPECIAL[v % len(SPECIAL)]
        if kind == 1:
            return v - (1 << 32) if v >= 1 << 31 else v
        return (v % (1 << 19)) - (1 << 18)


def geometry_digest(cases=4096, seed=0x9E3779B97F4A7C15):
    """FNV-1a (64 bits) over the seven integers of warp_taps, as 4 little-endian
    bytes each, of `cases` generated (matrix, window, border, output) tuples."""
    rng = Rng(seed)
    hsh = 0xCBF29CE484222325
    for _ in range(cases):
        m = [rng.coef() for _ in range(6)]
        cw, ch = 2 + 2 * (rng.next() % 24), 2 + 2 * (rng.next() % 16)
        border = rng.next() & 1
        i, j = rng.next() % 16384, rng.next() % 16384
        for v in taps_one(m, i, j, cw, ch, border):
            for b in (v & 0xFFFFFFFF).to_bytes(4, "little"):
                hsh = ((hsh ^ b) * 0x100000001B3) & MASK64
    return hsh
