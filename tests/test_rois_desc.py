"""The rule of the region-of-interest export, rois_ok in
broadway_amd/csrc/common/export_desc.h, on the CPU: tests/rois_desc_check.c
walks it over a grid on three pictures of 6 x 4 MBs (96 x 64) under
AddressSanitizer + UBSan and prints accept or refuse per row.  The expected
column below is written out from the rules of include/h264mi.h:

  at least one box; every pic in [0, npics); every box x, y >= 0, cw, ch > 0,
  all four even, inside 96 x 64, at most 32 source samples per output and axis
  (upscaling allowed); the descriptor's output size 1 .. 16384, element type U8
  .. F32, filter H264MI_RESIZE_TRIANGLE, and its own window all zero; one bad
  box refuses the list."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

A, R = "accept", "refuse"

ROIS = {
    "whole": A, "flush_right_bottom": A, "box_2x2": A, "pic_last": A, "pic_npics": R, "pic_minus_1": R,
    "x_odd": R, "y_odd": R, "cw_odd": R, "ch_odd": R,
    "right_plus_1": R, "right_plus_2": R, "bottom_plus_1": R, "bottom_plus_2": R, "cw_0": R, "ch_negative": R,
    "cw_32x": A, "cw_32x_plus_2": R, "ch_32x": A, "ch_32x_plus_2": R, "upscaled": A,
    "four_good": A, "nrois_0": R, "nrois_negative": R, "bad_box_last": R,
    "reserved_window_set": R, "reserved_x_set": R, "reserved_y_set": R, "ow_0": R, "filter_1": R, "dtype_i16": R,
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("rois_desc_check")
    exe = str(td / "rois_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "rois_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_validator_grid(lines):
    got = {}
    for ln in lines:
        f = ln.split()
        if f[0] == "rois":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(ROIS)
    assert {k: v for k, v in got.items() if v != ROIS[k]} == {}


def test_box_size_and_launch_bound(lines):
    """typedef struct { int pic, x, y, cw, ch; } h264mi_roi; 32 boxes per launch (TENSOR_MAX_PICS)."""
    assert "sizeof_roi 20 max_per_launch 32" in lines
