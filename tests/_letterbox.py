"""Helpers of tests/test_letterbox.py: DESIGN 3.5l's letterboxed export
restated on top of tests/_resize.py (tests/_colour.py for a colour set) and
tests/_tensor.py: inside the content rectangle the resized tensor of the window
at the content size, everywhere else the element tests/_tensor.py's conversion
makes of the pad sample.  The fit is restated from its definition with exact
fractions, not with the library's integer expression."""
import math
from fractions import Fraction

import numpy as np

import _colour as K
import _crop
import _resize as R
import _tensor as T

FITS = {"stretch": 0, "letterbox": 1, "topleft": 2}


def fit(cw, ch, size, how):
    """(rw, rh, px, py) of a cw x ch window in the canvas size = (oh, ow)."""
    oh, ow = size
    if how == "stretch":
        return ow, oh, 0, 0

    def minor(n_minor, n_major, m_major):
        exact = Fraction(n_minor * m_major, n_major)
        return max(math.floor(exact + Fraction(1, 2)), -(-n_minor // 32), 1)

    if Fraction(cw, ch) >= Fraction(ow, oh):
        rw, rh = ow, minor(ch, cw, ow)
    else:
        rw, rh = minor(cw, ch, oh), oh
    if how == "topleft":
        return rw, rh, 0, 0
    return rw, rh, (ow - rw) // 2, (oh - rh) // 2


def compose(content, size, place, planes, dtype, consts, pad):
    """The canvas's bytes: `content`, the bytes of the (planes, rh, rw) resized
    tensor, at (px, py) of (planes, oh, ow) pad elements."""
    oh, ow = size
    rw, rh, px, py = place
    es = T.ELEM[dtype]
    scale, bias = T.CONSTS[consts]
    bars = np.broadcast_to(np.asarray(pad[:planes], dtype=np.uint8).reshape(planes, 1, 1), (planes, oh, ow))
    out = T.convert(bars, dtype, scale, bias).reshape(planes, oh, ow, es).copy()
    out[:, py:py + rh, px:px + rw] = content.reshape(planes, rh, rw, es)
    return out.reshape(-1)


def expect(pic, w, h, cp, win, size, mode, dtype, consts, how, pad, colour=0):
    """Bytes the letterboxed export of window `win` of `pic` into the canvas
    size = (oh, ow) holds; pad: a sample per plane."""
    place = fit(win[2], win[3], size, how)
    inner = (place[1], place[0])
    if colour == 0:
        content = R.expect(pic, w, h, cp, win, inner, mode, dtype, consts)
    else:
        content = K.expect(pic, w, h, cp, tuple(win), colour, dtype, consts, size=inner)
    return compose(content, size, place, T.MODES[mode], dtype, consts, pad)


def frame_expect(frame, w, h, win, size, mode, dtype, consts, how, pad, colour=0):
    """The same of a packed I420 frame (the reference decoder's output)."""
    place = fit(win[2], win[3], size, how)
    inner = (place[1], place[0])
    if mode == "rgb" and colour:
        content = K.frame_expect(frame, w, h, win, colour, dtype, consts, size=inner)
    else:
        x, y, cw, ch = win
        scale, bias = T.CONSTS[consts]
        c = T.samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode)
        content = T.convert(R.resize_planes(c, inner[0], inner[1]), dtype, scale, bias)
    return compose(content, size, place, T.MODES[mode], dtype, consts, pad)
