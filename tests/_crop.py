"""Helpers of tests/test_crop.py and tests/golden/make_crop_golden.py: the
committed cropped-output fixtures (tests/golden/crop.json), the reference
testbench run with -C, and a numpy restatement of its CropPicture layout."""
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CROP_JSON = os.path.join(HERE, "golden", "crop.json")
REFDEC = os.path.join(ROOT, "oracle", "_ref", "refdec")


def cases():
    with open(CROP_JSON) as f:
        return json.load(f)["cases"]


def refdec_crop(stream: bytes):
    """DecTestBench -C -O on `stream`: (cropped frames, (left, top, width,
    height) as the testbench prints them, (picWidth, picHeight))."""
    if not os.path.exists(REFDEC):
        raise FileNotFoundError(REFDEC)
    with tempfile.TemporaryDirectory() as td:
        src, yuv = os.path.join(td, "in.h264"), os.path.join(td, "out.yuv")
        with open(src, "wb") as f:
            f.write(stream)
        out = subprocess.run([REFDEC, "-C", "-O" + yuv, src], capture_output=True, text=True)
        crop = size = None
        for line in out.stdout.splitlines():
            if line.startswith("Width"):
                p = line.split()
                size = (int(p[1]), int(p[3]))
            elif line.startswith("Cropping params:"):
                # "Cropping params: (6, 2) 86x52"
                a, b = line.split("(", 1)[1].split(")")
                l, t = (int(v) for v in a.split(","))
                w, h = (int(v) for v in b.strip().split("x"))
                crop = (l, t, w, h)
        data = open(yuv, "rb").read() if os.path.exists(yuv) else b""
    assert crop and size, out.stdout[-400:]
    fb = crop[2] * crop[3] * 3 // 2
    return [data[i:i + fb] for i in range(0, len(data), fb)], crop, size


def planes(buf, width, height, cpitch=None):
    """(Y, U, V) views of an I420 picture whose chroma rows are cpitch apart."""
    cpitch = cpitch or width // 2
    a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    ysz, csz = width * height, cpitch * (height // 2)
    return (a[:ysz].reshape(height, width), a[ysz:ysz + csz].reshape(height // 2, cpitch),
            a[ysz + csz:ysz + 2 * csz].reshape(height // 2, cpitch))


def crop_i420(buf, width, height, x, y, cw, ch, cpitch=None) -> np.ndarray:
    """CropPicture's output (DecTestBench.c:588-666): luma cw x ch from
    (y, x), then Cb and Cr (cw/2) x (ch/2) from (y/2, x/2), packed."""
    Y, U, V = planes(buf, width, height, cpitch)
    return np.concatenate([Y[y:y + ch, x:x + cw].ravel(),
                           U[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2].ravel(),
                           V[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2].ravel()])
