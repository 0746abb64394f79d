"""The rules of the destination descriptor, dest_ok in
broadway_amd/csrc/common/export_desc.h, on the CPU: tests/dest_desc_check.c
walks them over items of 3 x 32 x 48 fp16 elements under AddressSanitizer +
UBSan and prints accept or refuse per row.  The expected column is written out
from include/h264mi.h:

  every stride (row, plane, frame, out_stride) a non-negative multiple of the
  element size; row at least the packed row; plane 0 when interleaved; clip >=
  1 dividing the items; frame 0 with clip 1; reserved 0; and of the levels
  (row, rows), (plane, planes), (frame, clip), (out_stride, items / clip) with
  a count above 1, sorted by stride, each steps over the span of those below --
  in whatever order they come."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

A, R = "accept", "refuse"

ROWS = {
    "null": A, "null_interleaved": A, "all_zero": A, "all_zero_interleaved": A, "explicit_contiguous": A,
    "explicit_contiguous_interleaved": A, "ncthw": A, "row_padded_16": A, "row_padded_one_element": A,
    "channel_slice": A, "permuted_clip": A, "tile_grid": A, "tile_grid_interleaved": A, "one_item_any_out_stride": A,
    "row_not_multiple_of_es": R, "plane_not_multiple_of_es": R, "frame_not_multiple_of_es": R,
    "out_stride_not_multiple_of_es": R, "row_one_element_short": R, "row_one_element_short_interleaved": R,
    "plane_set_interleaved": R, "plane_overlaps_last_row": R, "frame_overlaps": R, "frame_zero_in_clip": R,
    "out_stride_overlaps": R, "out_stride_zero": R, "ncthw_clips_overlap": R, "clip_0": R, "clip_minus_1": R,
    "nitems_not_multiple_of_clip": R, "frame_set_clip_1": R, "reserved_1": R, "row_negative": R, "plane_negative": R,
    "frame_negative": R, "tile_grid_tiles_overlap": R, "plane_span_overflows": R, "row_span_overflows": R,
    "row_span_overflows_late": R,
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("dest_desc_check")
    exe = str(td / "dest_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "dest_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_validator_table(lines):
    got = {}
    for ln in lines:
        f = ln.split()
        if f[0] == "dest":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(ROWS)
    assert {k: v for k, v in got.items() if v != ROWS[k]} == {}


def test_descriptor_size(lines):
    """typedef struct { int64_t row, plane, frame; int32_t clip, reserved; } h264mi_tensor_dest;"""
    import ctypes as C
    from broadway_amd import _lib
    assert "sizeof_dest 32 row 0 plane 8 frame 16 clip 24 reserved 28" in lines
    T = _lib.TensorDest
    assert C.sizeof(T) == 32
    assert (T.row.offset, T.plane.offset, T.frame.offset, T.clip.offset, T.reserved.offset) == (0, 8, 16, 24, 28)
