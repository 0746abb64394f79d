"""Helpers of tests/test_field_resize.py: the resized field exports
(include/h264mi.h) restated in numpy int64, straight from the
definition -- the taps of tests/_resize.py, both axes with no intermediate
rounding, one rounding to units of 1 / 16 --, with tests/_mbinfo.py's element
conversion applied to r / 16."""
import numpy as np

import _mbinfo as M
from _resize import taps


def resize_acc(s, oh, ow):
    """(..., gh, gw) integers -> (acc (..., oh, ow), the largest |inner sum|),
    acc = sum_l qy_l * (sum_k qx_k * s[l][k]) in int64"""
    s = np.asarray(s, dtype=np.int64)
    gh, gw = s.shape[-2:]
    t = np.empty(s.shape[:-1] + (ow,), dtype=np.int64)
    for j, (f, q) in enumerate(taps(gw, ow)):
        t[..., j] = s[..., f:f + q.size] @ q
    acc = np.empty(s.shape[:-2] + (oh, ow), dtype=np.int64)
    for i, (f, q) in enumerate(taps(gh, oh)):
        acc[..., i, :] = np.einsum("l,...lj->...j", q, t[..., f:f + q.size, :])
    return acc, int(np.abs(t).max())


def resize_field(s, oh, ow):
    """(..., gh, gw) integers -> r (..., oh, ow) int64: the filtered field in
    units of 1 / 16"""
    acc, inner = resize_acc(s, oh, ow)
    assert inner < 1 << 29 and int(np.abs(acc).max()) < 1 << 43
    return (acc + (1 << 23)) >> 24


def convert(r, dtype, scale, bias):
    """The bytes of the tensor of filtered values r (C, oh, ow): int16 (r + 8)
    >> 4; the float types _mbinfo.convert of r / 16 (exact in float64)."""
    if dtype == "int16":
        return M.convert((r + 8) >> 4, dtype, scale, bias)
    return M.convert(r.astype(np.float64) / 16.0, dtype, scale, bias)


def expect(v, size, dtype, consts="unit"):
    """the bytes of the resized export of the window's field v (C, gh, gw) to size = (oh, ow)"""
    scale, bias = M.CONSTS[consts]
    return convert(resize_field(v, int(size[0]), int(size[1])), dtype, scale, bias)
