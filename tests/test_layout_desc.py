"""The rules of the layout descriptor, layout_desc_fixed_ok /
layout_window_ok / rois_layout_ok in broadway_amd/csrc/common/export_desc.h, on
the CPU: tests/layout_desc_check.c walks them on pictures of 96 x 64 under
AddressSanitizer + UBSan and prints accept or refuse per row.  The expected
column is written out from include/h264mi.h:

  layout PLANAR or INTERLEAVED; no size (ow == oh == 0) is the unresized export
  -- the tensor descriptor's rules, fit STRETCH, pad all zero, filter 0 --; any
  other size is the fit descriptor with its own rules (both of ow, oh 1..16384,
  fit one of three, pad[3] == 0, at most 32 source samples per output and axis
  of the content); boxes require a size and a reserved (zero) window."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

A, R = "accept", "refuse"

ROWS = {
    "plain_planar": A, "plain_interleaved": A, "plain_layout_2": R, "plain_layout_minus_1": R,
    "plain_gray_interleaved": A,
    "plain_fit_letterbox": R, "plain_fit_topleft": R, "plain_pad0": R, "plain_pad2": R, "plain_pad3": R,
    "plain_filter_1": R, "only_oh_0": R, "only_ow_0": R, "plain_dtype_i16": R, "plain_x_odd": R, "plain_too_wide": R,
    "stretch_planar": A, "stretch_interleaved": A, "letterbox_interleaved": A, "topleft_planar": A,
    "letterbox_layout_2": R, "letterbox_pad3": R, "fit_3": R, "stretch_filter_1": R, "stretch_beyond_32x": R,
    "stretch_ow_16385": R,
    "boxes_stretch_interleaved": A, "boxes_letterbox_planar": A, "boxes_no_size": R, "boxes_only_oh_0": R,
    "boxes_window_set": R, "boxes_window_x_set": R, "boxes_layout_2": R, "boxes_nrois_0": R, "boxes_bad_pic_last": R,
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("layout_desc_check")
    exe = str(td / "layout_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "layout_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_validator_table(lines):
    got = {}
    for ln in lines:
        f = ln.split()
        if f[0] == "layout":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(ROWS)
    assert {k: v for k, v in got.items() if v != ROWS[k]} == {}


def test_descriptor_size(lines):
    """typedef struct { h264mi_tensor_fit_desc f; int layout; } h264mi_tensor_layout_desc;"""
    import ctypes as C
    from broadway_amd import _lib
    assert "sizeof_layout_desc 72 fit_desc 68" in lines
    assert C.sizeof(_lib.TensorLayoutDesc) == 72 and _lib.TensorLayoutDesc.layout.offset == 68
