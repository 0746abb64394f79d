#!/usr/bin/env python3
"""Generate tests/golden/colour.json: streams of the in-tree generator whose
SPS carries a VUI with colour signalling (GenParams.vui_matrix /
vui_full_range), decoded by the REFERENCE decoder (oracle/_ref/refdec, built
from the reference C sources by oracle/Makefile.ref).

Runs only where that binary exists; never a test.  The fixture records the
generator parameters, each stream's SHA-256, what H264SwDecGetInfo reports of
the VUI (videoRange, matrixCoefficients) and the MD5 of every output frame
(MB-aligned I420).  A VUI changes no sample: every case's MD5s are those of
its parameters without the two knobs, which the script asserts.  Nothing from
the reference itself is stored.

    python tests/golden/make_colour_golden.py          # rewrites colour.json
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

# the geometry of crop.json's crop_ltrb_6x4
BASE = dict(nframes=5, w_mbs=6, h_mbs=4, slices=2, gop=3, crop_left=6, crop_right=4, crop_top=2, crop_bottom=10)
# name -> (seed, vui_matrix, vui_full_range, further overrides, videoRange, matrixCoefficients)
CASES = {
    "m1": (61, 1, 0, {}, 0, 1),
    "m1_full": (61, 1, 1, {}, 1, 1),
    "m6_full": (61, 6, 1, {}, 1, 6),
    "m7_full": (61, 7, 1, {}, 1, 7),
    "m2": (61, 2, 0, {}, 0, 2),
    "m5": (61, 5, 0, {}, 0, 5),
    "signal_only_full": (61, -1, 1, {}, 1, 2),
    # the two halves of the two-SPS stream: display reordering in the first
    "m1_poc0": (61, 1, 0, dict(poc_type=0), 0, 1),
    "m6_full_s62": (62, 6, 1, {}, 1, 6),
}


def main():
    from broadway_amd import gen
    import oracle as O

    out = {"generator": "broadway_amd.gen (libh264gen.so)",
           "decoder": "reference C (Decoder/src, make.py file list + DecTestBench.c), gcc -O2",
           "frame_md5": "MD5 of each output frame (width*height*3/2 bytes, MB-aligned I420), output order",
           "config": 2, "base_overrides": BASE, "cases": {}}
    for name, (seed, matrix, full, more, vr, mc) in CASES.items():
        ov = dict(BASE, **more)
        plain = gen.generate(2, seed, **ov)
        stream = gen.generate(2, seed, vui_matrix=matrix, vui_full_range=full, **ov)
        frames = [hashlib.md5(f).hexdigest() for f in O.refdec_frames(stream)]
        assert frames and frames == [hashlib.md5(f).hexdigest() for f in O.refdec_frames(plain)], name
        out["cases"][name] = {
            "seed": seed, "overrides": dict(more, vui_matrix=matrix, vui_full_range=full),
            "stream_bytes": len(stream), "stream_sha256": hashlib.sha256(stream).hexdigest(),
            "plain_sha256": hashlib.sha256(plain).hexdigest(),
            "videoRange": vr, "matrixCoefficients": mc, "frames": frames,
        }
        print(f"{name}: {len(frames)} frames, {len(stream) - len(plain)} bytes of VUI", flush=True)
    with open(os.path.join(HERE, "colour.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
