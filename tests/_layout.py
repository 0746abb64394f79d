"""Helper of tests/test_layout.py: DESIGN 3.5m's interleaved layout restated on
top of the planar oracles (tests/_tensor.py, _resize.py, _colour.py,
_letterbox.py), which give a picture's (planes, rows, cols) elements as bytes.
Elements are transposed, never bytes: element (p, i, j) goes to index
(i * cols + j) * planes + p."""
import numpy as np

import _tensor as T


def interleave(planar, planes, rows, cols, dtype):
    """The bytes of the (rows, cols, planes) picture holding the elements of
    `planar`, the bytes of a (planes, rows, cols) picture of `dtype`."""
    es = T.ELEM[dtype]
    e = np.asarray(planar, dtype=np.uint8).reshape(planes, rows, cols, es)
    return np.ascontiguousarray(e.transpose(1, 2, 0, 3)).reshape(-1)
