"""The rules of the affine-warped export, warp_desc_fixed_ok,
warp_window_ok and warps_ok in broadway_amd/csrc/common/export_desc.h, on the
CPU: tests/warp_desc_check.c walks them over a grid on three pictures of 6 x 4
MBs (96 x 64) under AddressSanitizer + UBSan and prints accept or refuse per
row.  The expected column below is written out from include/h264mi.h:

  at least one warp, every pic in [0, npics), any matrix; the window x, y >= 0,
  cw, ch > 0, all four even, inside 96 x 64, at most 16384 a side; the output
  size 1 .. 16384; element type U8 .. F32; filter H264MI_WARP_BILINEAR; border
  CONSTANT or REPLICATE; pad[3] zero, and pad all zero with REPLICATE; layout
  PLANAR or INTERLEAVED.  Every refused row is one step from an accepted one."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

A, R = "accept", "refuse"

WARPS = {
    "four_good": A, "one_good": A, "any_matrix": A, "nwarps_0": R, "nwarps_negative": R,
    "pic_last": A, "pic_npics_last": R, "pic_minus_1_last": R,
    "sub_window": A, "window_2x2_far_corner": A, "window_empty": R, "x_odd": R, "y_odd": R, "cw_odd": R, "ch_odd": R,
    "right_plus_2": R, "bottom_plus_2": R, "x_negative": R, "ch_negative": R,
    "size_1x1": A, "size_max": A, "ow_0": R, "oh_0": R, "ow_max_plus_1": R, "oh_max_plus_1": R,
    "filter_1": R, "border_2": R, "border_minus_1": R, "pad3_set": R, "replicate_with_pad": R,
    "replicate_with_pad2": R, "replicate": A, "interleaved": A, "layout_2": R,
    "dtype_u8": A, "dtype_f32": A, "dtype_i16": R, "dtype_minus_1": R,
    "window_16386": R, "window_16384": A,
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("warp_desc_check")
    exe = str(td / "warp_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "warp_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_validator_grid(lines):
    got = {}
    for ln in lines:
        f = ln.split()
        if f[0] == "warp":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(WARPS)
    assert {k: v for k, v in got.items() if v != WARPS[k]} == {}


def test_struct_sizes_and_launch_bound(lines):
    """typedef struct { int pic; int m[6]; } h264mi_warp; the descriptor is the
    48-byte tensor descriptor, four ints, four pad bytes and the layout; 32
    warps per launch (TENSOR_MAX_PICS)."""
    assert "sizeof_warp 28 sizeof_desc 72 max_per_launch 32" in lines
