"""Helpers of tests/test_resize.py: DESIGN 3.5c's resize restated in Python
integers (numpy int64), straight from its definition -- every source sample's
weight is evaluated and the positive ones are kept --, on top of
tests/_tensor.py: resized tensor == convert(resize(samples(window)))."""
import functools

import numpy as np

import _tensor as T

MAX_TAPS = 64
MAX_DIM = 16384


@functools.lru_cache(maxsize=None)
def taps(n, m):
    """One axis, n source samples -> m outputs: per output j the pair (first
    source index, int64 array q of its contiguous taps), sum(q) == 16384."""
    R = 2 * max(m, n)
    out = []
    k = np.arange(n, dtype=np.int64)
    for j in range(m):
        C = (2 * j + 1) * n - m
        w = R - np.abs(2 * m * k - C)
        keep = np.flatnonzero(w > 0)
        assert keep.size and (np.diff(keep) == 1).all()
        w = w[keep]
        W = int(w.sum())
        q = (w * 16384 + W // 2) // W
        q[int(np.argmax(w))] += 16384 - int(q.sum())        # (argmax: the first of the largest)
        out.append((int(keep[0]), q))
    return out


def resize(plane, oh, ow):
    """(ch, cw) uint8 -> (oh, ow) uint8: horizontal pass to a 6-bit fractional
    intermediate, then vertical."""
    ch, cw = plane.shape
    s = plane.astype(np.int64)
    t = np.empty((ch, ow), dtype=np.int64)
    for j, (f, q) in enumerate(taps(cw, ow)):
        t[:, j] = (s[:, f:f + q.size] @ q + 128) >> 8
    assert t.max() <= 255 * 64
    out = np.empty((oh, ow), dtype=np.int64)
    for i, (f, q) in enumerate(taps(ch, oh)):
        out[i] = (q @ t[f:f + q.size] + (1 << 19)) >> 20
    assert 0 <= out.min() and out.max() <= 255
    return out.astype(np.uint8)


def resize_planes(c, oh, ow):
    return np.stack([resize(p, oh, ow) for p in c])


@functools.lru_cache(maxsize=None)
def _resized_cached(key, w, h, cp, win, mode, oh, ow):
    r = resize_planes(T._samples_cached(key, w, h, cp, win, mode), oh, ow)
    r.setflags(write=False)
    return r


def expect(pic, w, h, cp, win, size, mode, dtype, consts="unit"):
    """Bytes the resized export of window `win` of `pic` to size = (oh, ow)
    holds.  The resized samples are computed once per (picture, window, mode,
    size)."""
    key = id(pic)
    T._PICS[key] = pic
    scale, bias = T.CONSTS[consts]
    return T.convert(_resized_cached(key, w, h, cp, tuple(win), mode, int(size[0]), int(size[1])), dtype, scale, bias)
