"""The fit and the rules of the letterboxed tensor export,
letterbox_fit, fit_desc_fixed_ok, fit_window_ok and rois_fit_ok in
broadway_amd/csrc/common/export_desc.h, on the CPU: tests/letterbox_fit_check.c
runs them under AddressSanitizer + UBSan and prints one line per row.  The
expected columns below are written out from the rules of include/h264mi.h:

  the major axis fills the canvas, the minor axis is the nearest integer to
  its exact size (halves up), raised to ceil(n / 32) and to 1; letterbox
  centres (floored), topleft does not, stretch is the canvas;

  a descriptor passes with the resized export's rules, the window judged
  against its content size (cw <= 32 rw, ch <= 32 rh), fit in 0..2 and
  pad[3] == 0; a list passes when its own window is zero and every box
  passes with its own fit -- one bad box refuses the list."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

A, R = "accept", "refuse"
STRETCH, BOX, TOPLEFT = 0, 1, 2

# (cw, ch, ow, oh, fit) -> (rw, rh, px, py)
FITS = {
    (1920, 1080, 640, 640, BOX): (640, 360, 0, 140),
    (1920, 1080, 224, 224, BOX): (224, 126, 0, 49),
    (64, 128, 224, 224, BOX): (112, 224, 56, 0),
    (38, 26, 9, 7, BOX): (9, 6, 0, 0),
    # 47 rows at exactly 32 : 1: (2 * 47 * 47 + 1504) // 3008 = 1, raised to ceil(47 / 32) = 2
    (1504, 47, 47, 47, BOX): (47, 2, 0, 22),
    (47, 1504, 47, 47, BOX): (2, 47, 22, 0),
    (1920, 1080, 640, 640, TOPLEFT): (640, 360, 0, 0),
    (1920, 1080, 640, 640, STRETCH): (640, 640, 0, 0),
    (38, 26, 70, 40, BOX): (58, 40, 6, 0),              # 2 * 38 * 40 + 26 = 3066, // 52 = 58
    (2, 2, 70, 40, BOX): (40, 40, 15, 0),
    (256, 32, 8, 3, BOX): (8, 1, 0, 1),
    (64, 2, 2, 2, BOX): (2, 1, 0, 0),                   # the minor axis rounds to 0: at least 1
    (4, 2, 3, 3, BOX): (3, 2, 0, 0),                    # 1.5 rows: halves up
    (16384, 16384, 16384, 1, BOX): (512, 1, 7936, 0),   # (beyond 32 : 1 on the major axis: the rules refuse it)
}

DESC = {
    "whole_letterbox": A, "whole_topleft": A, "whole_stretch": A, "fit_3": R, "fit_minus_1": R, "pad3_set": R,
    "pad3_set_stretch": R, "major_32x": A, "major_32x_plus_2": R, "major_32x_tall": A, "major_32x_plus_2_tall": R,
    "minor_kept_by_the_raise": A, "stretch_33x": R, "letterbox_of_the_same": R, "stretch_minor_33x": R, "upscaled": A,
    "x_odd": R, "cw_odd": R, "right_plus_2": R, "cw_0": R, "ow_0": R, "oh_16385": R,
}

ROIS = {
    "four_good_fit_0": A, "four_good_fit_1": A, "four_good_fit_2": A, "fit_3": R, "pad3_set": R, "reserved_window_set": R,
    "nrois_0": R, "bad_box_last_odd": R, "bad_box_pic": R, "bad_box_over_the_edge": R, "one_box_beyond_32x": R,
    "tall_box_beyond_32x_stretched": R, "tall_box_beyond_32x": R, "all_within_32x": A,
}


def run_check(td):
    """The lines tests/letterbox_fit_check.c prints (test_letterbox_cpu.py reads its fit table too)."""
    exe = str(td / "letterbox_fit_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "letterbox_fit_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def fit_table(lines):
    """(cw, ch, ow, oh, fit) -> (rw, rh, px, py) of the program's "fit" lines."""
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("fit ")]
    return {r[:5]: r[5:] for r in rows}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    return run_check(tmp_path_factory.mktemp("letterbox_fit_check"))


def test_fit_reference_values(lines):
    got = fit_table(lines)
    assert set(FITS) <= set(got)
    assert {k: (got[k], v) for k, v in FITS.items() if got[k] != v} == {}


def test_fit_invariants_over_the_sweep(lines):
    """Content inside the canvas and both axes within 32 : 1 wherever the major axis is."""
    assert "sweep ok" in lines and not [ln for ln in lines if ln.startswith("sweep bad")]


@pytest.mark.parametrize("kind,want", [("fit_desc", DESC), ("rois_fit", ROIS)])
def test_validator_grid(lines, kind, want):
    got = {}
    for ln in lines:
        f = ln.split()
        if f[0] == kind:
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_descriptor_layout(lines):
    """typedef struct { h264mi_tensor_resize_desc r; int fit; unsigned char pad[4]; } h264mi_tensor_fit_desc;"""
    assert "sizeof_fit_desc 68 fits 0 1 2" in lines
