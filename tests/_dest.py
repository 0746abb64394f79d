"""Where a strided destination (h264mi_tensor_dest) puts the bytes
the existing oracles give: no arithmetic of its own, only addresses.  An item's
packed bytes -- planar (planes, rows, cols) from _tensor / _resize / _bicubic /
_letterbox / _warp, or interleaved (rows, cols, planes) from _layout -- are
scattered into a sentinel-filled buffer by the rules of include/h264mi.h:
item k starts (k // clip) * out_stride + (k % clip) * frame bytes in, element
(p, i, j) at p * plane + i * row + j * es (planar) or i * row + (j * planes + p)
* es (interleaved)."""
import ctypes as C
from collections import namedtuple

import numpy as np

SENTINEL = 0xA5

# the five fields of the descriptor as the caller sets them (0: the default)
Dest = namedtuple("Dest", "row plane frame clip", defaults=(0, 0, 0, 1))


def resolve(dest, es, planes, rows, cols, interleaved):
    """(row, plane, frame, clip) with the descriptor's zeros filled in; None: packed."""
    d = dest if dest is not None else Dest()
    row = d.row or cols * es * (planes if interleaved else 1)
    plane = 0 if interleaved else (d.plane or rows * row)
    return Dest(row, plane, d.frame, d.clip)


def item_offsets(dest, es, planes, rows, cols, interleaved):
    """The byte offsets, from an item's start, of its packed bytes in order."""
    row, plane, _, _ = resolve(dest, es, planes, rows, cols, interleaved)
    if interleaved:
        return (np.arange(rows, dtype=np.int64)[:, None] * row + np.arange(cols * planes * es, dtype=np.int64)).reshape(-1)
    return (np.arange(planes, dtype=np.int64)[:, None, None] * plane + np.arange(rows, dtype=np.int64)[None, :, None] * row +
            np.arange(cols * es, dtype=np.int64)).reshape(-1)


def item_start(dest, k, out_stride):
    clip, frame = (dest.clip, dest.frame) if dest is not None else (1, 0)
    return (k // clip) * out_stride + (k % clip) * frame


def extent(dest, nitems, out_stride, es, planes, rows, cols, interleaved):
    """One past the last byte the nitems items address."""
    off = item_offsets(dest, es, planes, rows, cols, interleaved)
    return max(item_start(dest, k, out_stride) for k in range(nitems)) + int(off.max()) + 1


def scatter(total, base, items, dest, out_stride, es, planes, rows, cols, interleaved):
    """The buffer of `total` bytes an export of `items` (each the packed bytes
    of one item) to `base` leaves behind: sentinels wherever the descriptor
    addresses nothing.  No byte is addressed twice (dest_ok's rule), which is
    checked here too."""
    out = np.full(total, SENTINEL, dtype=np.uint8)
    seen = np.zeros(total, dtype=bool)
    off = item_offsets(dest, es, planes, rows, cols, interleaved)
    for k, b in enumerate(items):
        assert b.size == off.size, (b.size, off.size)
        at = base + item_start(dest, k, out_stride) + off
        assert at.min() >= 0 and at.max() < total and not seen[at].any()
        seen[at] = True
        out[at] = b
    return out


def c_dest(dest):
    """The _lib.TensorDest of a Dest (None: NULL)."""
    from broadway_amd import _lib
    if dest is None:
        return None
    return C.byref(_lib.TensorDest(dest.row, dest.plane, dest.frame, dest.clip, 0))
