"""The numpy oracle of the statistics export (stats.hip): exact
integers from the samples that are pinned already -- _crop.planes (the stored
Y, U, V of a picture in the (width, cpitch) layout), _tensor.samples (R, G, B of
the reference converter) and _colour.samples_colour (colour sets 1..3)."""
import numpy as np

import _colour as K
import _crop
import _tensor as T

WORDS, BINS = 8, 256
PLANES = {"y": 1, "yuv": 3, "rgb": 3}
PLANE_IDS = {"y": 0, "yuv": 1, "rgb": 2}
FIELDS = ("count", "sum", "sumsq", "min", "max", "sad", "ssd")


def words(planes, hist):
    """(P, L) of an item."""
    return PLANES[planes], WORDS + (BINS if hist else 0)


def plane_samples(pic, w, h, cp, win, planes, colour=0):
    """The item's samples, one 2-D uint8 array per plane: the window of the
    stored luma ("y"), with the chroma planes at their own resolution ("yuv"),
    or the R, G, B of the unresized tensor export under colour id ``colour``."""
    x, y, cw, ch = win
    if planes == "rgb":
        i420 = _crop.crop_i420(pic, w, h, x, y, cw, ch, cpitch=cp)
        s = T.samples(i420, cw, ch, "rgb") if colour == 0 else K.samples_colour(i420, cw, ch, colour)
        return [s[p] for p in range(3)]
    Y, U, V = _crop.planes(pic, w, h, cp)
    out = [Y[y:y + ch, x:x + cw]]
    if planes == "yuv":
        out += [U[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2], V[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2]]
    return out


def record(s, r=None, hist=False):
    """One plane record, L int64 words, of samples s against reference samples r."""
    s = np.asarray(s).astype(np.int64).ravel()
    out = np.zeros(WORDS + (BINS if hist else 0), dtype=np.int64)
    out[0], out[1], out[2], out[3], out[4] = s.size, s.sum(), (s * s).sum(), s.min(), s.max()
    if r is not None:
        d = s - np.asarray(r).astype(np.int64).ravel()
        out[5], out[6] = np.abs(d).sum(), (d * d).sum()
    if hist:
        out[WORDS:] = np.bincount(s, minlength=BINS)
    return out


def expect(pic, w, h, cp, win, planes, colour=0, hist=False, ref=None):
    """The (P, L) int64 words of the item `win` of `pic` (against the same window of `ref`)."""
    s = plane_samples(pic, w, h, cp, win, planes, colour)
    r = plane_samples(ref, w, h, cp, win, planes, colour) if ref is not None else [None] * len(s)
    return np.stack([record(a, b, hist) for a, b in zip(s, r)])


def expect_items(pics, refs, w, h, cp, items, planes, colour=0, hist=False):
    """(len(items), P, L): items = [(k, x, y, cw, ch), ...] over the picture
    list `pics` (and `refs`, a list of as many pictures, or None)."""
    return np.stack([expect(pics[k], w, h, cp, (x, y, cw, ch), planes, colour, hist, refs[k] if refs is not None else None)
                     for k, x, y, cw, ch in items])
