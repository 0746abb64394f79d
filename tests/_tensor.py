"""Helpers of tests/test_tensor.py: the constant sets, and the numpy / torch-CPU
restatement of the tensor export (tensor.hip) on top of what is pinned to the
reference already -- _crop.crop_i420 (CropPicture) and oracle.yuv2rgba (the
reference converter's arithmetic, tests/test_rgba.py)."""
import functools

import numpy as np

import oracle as O
import _crop
from broadway_amd.engine import tensor_affine

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# name -> (scale triple, bias triple), fp32-representable
CONSTS = {
    "identity": ((1.0,) * 3, (0.0,) * 3),
    "unit": ((float(np.float32(1.0 / 255.0)),) * 3, (0.0,) * 3),
    "imagenet": tensor_affine(IMAGENET_MEAN, IMAGENET_STD),
}

DTYPES = ["uint8", "float16", "bfloat16", "float32"]
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
MODES = {"rgb": 3, "gray": 1}


def torch_dtype(name):
    import torch
    return getattr(torch, name)


def samples(i420, cw, ch, mode):
    """(planes, ch, cw) uint8 samples of a cropped packed I420 picture: R, G,
    B de-interleaved from oracle.yuv2rgba, or the luma plane."""
    i420 = np.frombuffer(bytes(i420), dtype=np.uint8) if not isinstance(i420, np.ndarray) else i420
    if mode == "gray":
        return i420[:cw * ch].reshape(1, ch, cw)
    rgba = np.frombuffer(O.yuv2rgba(i420.tobytes(), cw, ch), dtype=np.uint8).reshape(ch, cw, 4)
    return np.ascontiguousarray(rgba[:, :, :3].transpose(2, 0, 1))


def convert(c, dtype, scale, bias):
    """The bytes of the tensor of samples c (planes, ch, cw): float64(c) *
    float64(scale) + float64(bias) -- exact for the constant sets here
    (test_exactness_premise) --, rounded once to float32 (so: a hardware fma),
    then converted to the target type (numpy and torch round to nearest-even)."""
    if dtype == "uint8":
        return np.ascontiguousarray(c).reshape(-1)
    planes = c.shape[0]
    s = np.asarray(scale[:planes], dtype=np.float32).astype(np.float64).reshape(planes, 1, 1)
    b = np.asarray(bias[:planes], dtype=np.float32).astype(np.float64).reshape(planes, 1, 1)
    f = (c.astype(np.float64) * s + b).astype(np.float32)
    if dtype == "float32":
        out = f
    elif dtype == "float16":
        out = f.astype(np.float16)
    else:
        import torch
        return torch.from_numpy(f).to(torch.bfloat16).contiguous().view(torch.uint8).numpy().reshape(-1)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def _samples_cached(key, w, h, cp, win, mode):
    pic = _PICS[key]
    x, y, cw, ch = win
    return samples(_crop.crop_i420(pic, w, h, x, y, cw, ch, cpitch=cp), cw, ch, mode)


_PICS = {}


def expect(pic, w, h, cp, win, mode, dtype, consts="unit"):
    """Bytes the export of window `win` of `pic` (chroma rows cp apart) holds.
    The uint8 samples are computed once per (picture, window, mode)."""
    key = id(pic)
    _PICS[key] = pic
    scale, bias = CONSTS[consts]
    return convert(_samples_cached(key, w, h, cp, tuple(win), mode), dtype, scale, bias)
