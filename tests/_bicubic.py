"""Helpers of tests/test_bicubic*.py: DESIGN 3.5o's bicubic resize (Keys, a =
-0.5, antialiased) restated in Python integers (numpy int64), straight from its
definition -- every source sample's distance is evaluated and those inside the
support are kept --, on top of tests/_tensor.py:
resized tensor == convert(resize(samples(window)))."""
import functools

import numpy as np

import _tensor as T

MAX_TAPS = 64
MAX_DIM = 16384
MAX_RATIO = 16          # source samples per output and axis, at most
FILTER = 2              # H264MI_RESIZE_BICUBIC


@functools.lru_cache(maxsize=None)
def taps(n, m):
    """One axis, n source samples -> m outputs: per output j the pair (first
    source index, int64 array q of its contiguous taps), sum(q) == 16384; q may
    be negative."""
    R = 2 * max(m, n)
    R3 = 2 * R ** 3
    s = max(0, R3.bit_length() - 16)
    out = []
    k = np.arange(n, dtype=np.int64)
    for j in range(m):
        C = (2 * j + 1) * n - m
        d = np.abs(2 * m * k - C)
        keep = np.flatnonzero(d < 2 * R)
        assert keep.size and (np.diff(keep) == 1).all()
        d = d[keep]
        w = np.where(d < R, 3 * d ** 3 - 5 * R * d ** 2 + R3, -d ** 3 + 5 * R * d ** 2 - 8 * R * R * d + 2 * R3)
        w = w >> s                                          # (arithmetic: floor)
        assert int(np.abs(w).max()) < 1 << 16
        W = int(w.sum())
        assert W > 0 and int(np.abs(w).max()) * 16384 + W // 2 < 1 << 31
        q = (w * 16384 + W // 2) // W                       # (floor division)
        q[int(np.argmax(w))] += 16384 - int(q.sum())        # (argmax: the first of the largest)
        out.append((int(keep[0]), q))
    return out


def resize_unclamped(plane, oh, ow):
    """(ch, cw) uint8 -> (oh, ow) int64 before the clamp: horizontal pass to a
    signed 6-bit fractional intermediate (an int16), then vertical."""
    ch, cw = plane.shape
    s = plane.astype(np.int64)
    t = np.empty((ch, ow), dtype=np.int64)
    for j, (f, q) in enumerate(taps(cw, ow)):
        t[:, j] = (s[:, f:f + q.size] @ q + 128) >> 8
    assert -32768 <= t.min() and t.max() <= 32767
    out = np.empty((oh, ow), dtype=np.int64)
    for i, (f, q) in enumerate(taps(ch, oh)):
        acc = q @ t[f:f + q.size]
        assert np.abs(acc).max() < (1 << 31) - (1 << 19)
        out[i] = (acc + (1 << 19)) >> 20
    return out


def resize(plane, oh, ow):
    return np.clip(resize_unclamped(plane, oh, ow), 0, 255).astype(np.uint8)


def resize_planes(c, oh, ow):
    return np.stack([resize(p, oh, ow) for p in c])


@functools.lru_cache(maxsize=None)
def _resized_cached(key, w, h, cp, win, mode, oh, ow):
    r = resize_planes(T._samples_cached(key, w, h, cp, win, mode), oh, ow)
    r.setflags(write=False)
    return r


def resized_samples(pic, w, h, cp, win, size, mode):
    """The (planes, oh, ow) uint8 samples of window `win` of `pic` resized to
    size = (oh, ow); computed once per (picture, window, mode, size), read-only."""
    key = id(pic)
    T._PICS[key] = pic
    return _resized_cached(key, w, h, cp, tuple(win), mode, int(size[0]), int(size[1]))


def expect(pic, w, h, cp, win, size, mode, dtype, consts="unit"):
    """Bytes the bicubic resized export of window `win` of `pic` to size = (oh,
    ow) holds."""
    scale, bias = T.CONSTS[consts]
    return T.convert(resized_samples(pic, w, h, cp, win, size, mode), dtype, scale, bias)
