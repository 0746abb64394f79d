"""Helpers of tests/test_colour.py: the colour sets of the RGB tensor exports
 derived with fractions.Fraction from their definition, the
conversion restated in numpy integers, and the expected tensors on top of
tests/_tensor.py (convert) and tests/_resize.py (resize_planes), unchanged."""
import functools
from fractions import Fraction as F

import numpy as np

import _crop
import _resize as R
import _tensor as T

NAMES = ("reference", "bt601-full", "bt709", "bt709-full")
STREAM = 15
UNSPEC = {"bt601": 0, "bt709": 1, "size": 2}
# (Kr, Kb) and full range of ids 1..3
FAMILY = {1: (F("0.299"), F("0.114"), True), 2: (F("0.2126"), F("0.0722"), False), 3: (F("0.2126"), F("0.0722"), True)}


def rational(cid):
    """(ky, yoff, crv, cgu, cgv, cbu) of ids 1..3 as exact rationals."""
    kr, kb, full = FAMILY[cid]
    kg = 1 - kr - kb
    ky, yoff, f = (F(1), 0, F(1)) if full else (F(255, 219), 16, F(255, 224))
    return ky, yoff, f * 2 * (1 - kr), f * 2 * kb * (1 - kb) / kg, f * 2 * kr * (1 - kr) / kg, f * 2 * (1 - kb)


def _round(c):
    return (1024 * c + F(1, 2)).__floor__()


@functools.lru_cache(maxsize=None)
def coeffs(cid):
    """The six integers (ky, k0, crv, cgu, cgv, cbu) of set `cid`.  Set 0 is
    the reference's converter verbatim (no rounding term); 1..3 come from the
    definition: floor(1024 c + 1/2), k0 = 512 - ky yoff."""
    if cid == 0:
        return (1192, -1192 * 16, 1634, 400, 832, 2066)
    ky, yoff, crv, cgu, cgv, cbu = rational(cid)
    ky = _round(ky)
    return (ky, 512 - ky * yoff, _round(crv), _round(cgu), _round(cgv), _round(cbu))


def mode(cid, unspec=0, layout=0):
    return layout | cid << 8 | unspec << 12


def rgb_of(y, u, v, cid):
    """R, G, B (int64 arrays, clamped) of integer arrays y, u, v."""
    ky, k0, crv, cgu, cgv, cbu = coeffs(cid)
    y, u, v = (np.asarray(a, dtype=np.int64) for a in (y, u, v))
    u, v = u - 128, v - 128
    a0 = ky * y + k0
    return (np.clip((a0 + crv * v) >> 10, 0, 255), np.clip((a0 - cgu * u - cgv * v) >> 10, 0, 255),
            np.clip((a0 + cbu * u) >> 10, 0, 255))


def samples_colour(i420, cw, ch, cid):
    """(3, ch, cw) uint8 R, G, B of a packed I420 picture of cw x ch (both
    even) under set `cid`; the chroma sample of a 2x2 block is replicated."""
    a = np.frombuffer(bytes(i420), dtype=np.uint8) if not isinstance(i420, np.ndarray) else i420
    y = a[:cw * ch].reshape(ch, cw)
    u = a[cw * ch:cw * ch + (cw // 2) * (ch // 2)].reshape(ch // 2, cw // 2).repeat(2, axis=0).repeat(2, axis=1)
    v = a[cw * ch + (cw // 2) * (ch // 2):cw * ch + 2 * (cw // 2) * (ch // 2)].reshape(ch // 2, cw // 2)
    v = v.repeat(2, axis=0).repeat(2, axis=1)
    return np.stack(rgb_of(y, u, v, cid)).astype(np.uint8)


EXTREMES = (0, 1, 16, 127, 128, 129, 240, 254, 255)


def extremes_picture():
    """256 x 162, packed: luma is the column index; row pair r has the (U, V)
    pair r of EXTREMES x EXTREMES, so every clamp and both signs of every
    term occur."""
    w, h = 256, 2 * len(EXTREMES) ** 2
    y = np.tile(np.arange(w, dtype=np.uint8), (h, 1))
    u = np.repeat(np.array([a for a in EXTREMES for _ in EXTREMES], dtype=np.uint8)[:, None], w // 2, axis=1)
    v = np.repeat(np.array([b for _ in EXTREMES for b in EXTREMES], dtype=np.uint8)[:, None], w // 2, axis=1)
    p = np.concatenate([y.ravel(), u.ravel(), v.ravel()])
    p.setflags(write=False)
    return p, w, h, w // 2


_PICS = {}


@functools.lru_cache(maxsize=None)
def _samples_cached(key, w, h, cp, win, cid):
    x, y, cw, ch = win
    s = samples_colour(_crop.crop_i420(_PICS[key], w, h, x, y, cw, ch, cpitch=cp), cw, ch, cid)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _resized_cached(key, w, h, cp, win, cid, oh, ow):
    r = R.resize_planes(_samples_cached(key, w, h, cp, win, cid), oh, ow)
    r.setflags(write=False)
    return r


def expect(pic, w, h, cp, win, cid, dtype, consts="unit", size=None):
    """Bytes the RGB export of window `win` of `pic` (chroma rows cp apart)
    holds under set `cid`; size = (oh, ow): the resized export.  The samples
    are computed once per (picture, window, set[, size])."""
    key = id(pic)
    _PICS[key] = pic
    scale, bias = T.CONSTS[consts]
    c = (_samples_cached(key, w, h, cp, tuple(win), cid) if size is None
         else _resized_cached(key, w, h, cp, tuple(win), cid, int(size[0]), int(size[1])))
    return T.convert(c, dtype, scale, bias)


def frame_expect(frame, w, h, win, cid, dtype, consts="unit", size=None):
    """The same for a decoded packed frame (not cached)."""
    x, y, cw, ch = win
    c = samples_colour(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, cid)
    if size is not None:
        c = R.resize_planes(c, int(size[0]), int(size[1]))
    scale, bias = T.CONSTS[consts]
    return T.convert(c, dtype, scale, bias)


def resolve(matrix, full, unspec, cw, ch):
    """The colour id STREAM gives a picture whose SPS has matrix_coefficients
    `matrix` (2: none given) and full-range flag `full`."""
    if matrix == 1:
        bt709 = True
    elif matrix in (5, 6):
        bt709 = False
    else:
        bt709 = unspec == UNSPEC["bt709"] or (unspec == UNSPEC["size"] and (cw >= 1280 or ch > 576))
    return (2 if bt709 else 0) + (1 if full else 0)
