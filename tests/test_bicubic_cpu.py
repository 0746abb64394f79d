"""The bicubic filter of the resized tensor exports (DESIGN 3.5o,
H264MI_RESIZE_BICUBIC) without a GPU: the integer oracle (tests/_bicubic.py)
against torch's antialiased bicubic interpolation, the invariants of its taps,
the descriptor rules (tests/bicubic_desc_check.c on
broadway_amd/csrc/common/export_desc.h), the Python surface, and the host side
of the H264SwDec calls on the CPU stand-in of the engine
(tests/bicubic_host_check.c)."""
import os
import subprocess

import numpy as np
import pytest

import _bicubic as B
from test_resize import TORCH_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (ch, cw, oh, ow)
SHAPES = TORCH_SHAPES + [(18, 22, 37, 45), (34, 50, 33, 49), (16, 16, 1, 1), (2, 2, 7, 5), (30, 46, 8, 40)]


def inputs(ch, cw, rng):
    """Random bytes, and a 0 / 255 pattern (which drives the overshoot)."""
    return {"random": rng.integers(0, 256, (ch, cw), dtype=np.uint8),
            "0/255": (rng.integers(0, 2, (ch, cw), dtype=np.uint8) * 255).astype(np.uint8)}


def test_oracle_is_torch_antialiased_bicubic():
    """The integer arithmetic is torch's antialiased bicubic interpolation
    (float64, half-pixel centres, a = -0.5), clamped to 0..255, with one final
    rounding: within half a sample, plus the intermediate's 1/128 amplified by
    sum |qy| / 16384 <= 1.3, plus room for the 14-bit weights -- 0.5 + 1/32.
    Measured worst over these shapes and inputs: 0.5206.  On the 0 / 255 inputs
    the unclamped result leaves 0..255 at both ends, so the clamp is used."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    lowest, highest = 0, 255
    for ch, cw, oh, ow in SHAPES:
        for name, plane in inputs(ch, cw, rng).items():
            raw = B.resize_unclamped(plane, oh, ow)
            got = B.resize(plane, oh, ow)
            assert np.array_equal(got, np.clip(raw, 0, 255))
            ref = F.interpolate(torch.from_numpy(plane.astype(np.float64))[None, None], size=(oh, ow), mode="bicubic",
                                antialias=True, align_corners=False)[0, 0].clamp(0, 255).numpy()
            worst = float(np.abs(got.astype(np.float64) - ref).max())
            print(f"({ch},{cw})->({oh},{ow}) {name}: max |oracle - torch| = {worst:.4f}, unclamped "
                  f"[{int(raw.min())}, {int(raw.max())}]")
            assert worst <= 0.5 + 1 / 32, (ch, cw, oh, ow, name)
            if name == "0/255":
                lowest, highest = min(lowest, int(raw.min())), max(highest, int(raw.max()))
    print(f"unclamped over the 0 / 255 inputs: [{lowest}, {highest}]")
    assert lowest < 0 and highest > 255


def test_identity_size_returns_the_plane():
    rng = np.random.default_rng(2)
    for ch, cw in ((32, 46), (2, 2), (1, 17), (16, 16)):
        for plane in inputs(ch, cw, rng).values():
            assert np.array_equal(B.resize(plane, ch, cw), plane)
    for first, q in B.taps(16, 16)[1:-1]:
        assert q.tolist() == [0, 16384, 0]


@pytest.mark.parametrize("n,m", [(1920, 224), (1080, 224), (256, 16), (16384, 1024), (3840, 240), (2, 64), (46, 45),
                                 (17, 16)])
def test_taps_invariants(n, m):
    tp = B.taps(n, m)
    assert len(tp) == m
    most, negative = 0, False
    for first, q in tp:
        assert 0 <= first and first + q.size <= n and q.size >= 1        # contiguous by construction, inside [0, n)
        assert int(q.sum()) == 16384
        assert int(np.abs(q).sum()) < 32768
        assert -32768 <= int(q.min()) and int(q.max()) <= 32767          # the kernel's tables are int16
        most = max(most, q.size)
        negative = negative or bool((q < 0).any())
    assert most <= B.MAX_TAPS
    if n == B.MAX_RATIO * m:
        assert most == B.MAX_TAPS
    assert negative                                                      # (otherwise it is not a cubic)


# ------------------------------------------------------------ the rules ----
A, R = "accept", "refuse"

ROWS = {
    "filter_bicubic": A, "filter_triangle": A, "filter_1": R, "filter_minus_1": R, "filter_3": R,
    "fit_filter_bicubic": A, "fit_filter_1": R, "fit_filter_3": R,
    "layout_filter_bicubic": A, "layout_filter_3": R, "layout_unresized_filter_bicubic": R,
    "layout_unresized_filter_0": A,
    "rois_filter_bicubic": A, "rois_filter_1": R, "rois_filter_3": R,
    "bicubic_cw_16_ow": A, "bicubic_cw_16_ow_plus_2": R, "triangle_cw_16_ow_plus_2": A,
    "bicubic_ch_16_oh": A, "bicubic_ch_16_oh_plus_2": R, "triangle_ch_16_oh_plus_2": A,
    "triangle_cw_32_ow": A, "bicubic_cw_32_ow": R, "bicubic_upscale": A,
    "fit_bicubic_cw_16_ow": A, "fit_bicubic_cw_16_ow_plus_2": R, "fit_triangle_cw_16_ow_plus_2": A,
    "letterbox_bicubic_minor_within_16": A, "letterbox_bicubic_minor_beyond_16": R,
    "letterbox_triangle_minor_beyond_16": A, "letterbox_bicubic_major_beyond_16": R,
    "layout_bicubic_cw_16_ow_plus_2": R, "layout_letterbox_bicubic_minor_beyond_16": R,
    "rois_bicubic_cw_16_ow": A, "rois_bicubic_cw_16_ow_plus_2": R, "rois_triangle_cw_16_ow_plus_2": A,
    "rois_fit_bicubic_minor_within_16": A, "rois_fit_bicubic_minor_beyond_16": R,
    "rois_fit_triangle_minor_beyond_16": A,
    "rois_layout_bicubic_cw_16_ow": A, "rois_layout_bicubic_cw_16_ow_plus_2": R,
    "accmv_filter_triangle": A, "accres_filter_triangle": A, "accmv_filter_bicubic": R, "accres_filter_bicubic": R,
}


@pytest.fixture(scope="module")
def desc_lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("bicubic_desc_check")
    exe = str(td / "bicubic_desc_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "bicubic_desc_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def test_validator_table(desc_lines):
    got = {}
    for ln in desc_lines:
        f = ln.split()
        if f[0] == "bicubic":
            assert f[1] not in got, ln
            got[f[1]] = f[2]
    assert sorted(got) == sorted(ROWS)
    assert {k: v for k, v in got.items() if v != ROWS[k]} == {}


def test_letterbox_fit_is_the_triangles(desc_lines):
    """One public fit for both filters: 320 x 34 into 20 x 20 is 20 x 2 -- 17
    rows per output, which the bicubic rows above refuse."""
    from broadway_amd import _lib
    from broadway_amd.engine import letterbox_fit
    assert "fit_320x34_into_20x20 20 2 0 9" in desc_lines
    assert letterbox_fit(320, 34, (20, 20)) == (20, 2, 0, 9)
    assert "enum triangle 0 bicubic 2" in desc_lines
    assert (_lib.RESIZE_TRIANGLE, _lib.RESIZE_BICUBIC) == (0, 2)


# --------------------------------------------------- the Python surface ----
def test_python_surface_builds_the_filter():
    from broadway_amd import _lib
    from broadway_amd.decoder import Decoder, rois_args
    from broadway_amd.engine import rois_desc, tensor_desc
    d, planes, _ = tensor_desc((2, 4, 6, 8), mode="gray", size=(3, 5), filter="bicubic")
    assert isinstance(d, _lib.TensorResizeDesc) and (d.oh, d.ow, d.filter, planes) == (3, 5, 2, 1)
    # the default, and its name: today's descriptors
    for kw in ({}, {"filter": "triangle"}, {"filter": None}):
        d, _, _ = tensor_desc((2, 4, 6, 8), size=(3, 5), **kw)
        assert isinstance(d, _lib.TensorResizeDesc) and d.filter == 0
        d, arr, _, _ = rois_desc([(0, 0, 0, 34, 2)], (1, 2), 1, 64, 64, **kw)
        assert isinstance(d, _lib.TensorResizeDesc) and d.filter == 0 and len(arr) == 1
        assert rois_args([(0, 0, 34, 2)], (1, 2), 64, 64, **kw)[0].filter == 0
    assert isinstance(tensor_desc((2, 4, 6, 8))[0], _lib.TensorDesc)
    assert tensor_desc((2, 4, 6, 8), size=(3, 5), layout="nhwc")[0].f.r.filter == 0
    # under a layout, a fit, and over boxes
    assert tensor_desc((2, 4, 6, 8), size=(3, 5), layout="nhwc", filter="bicubic")[0].f.r.filter == 2
    d, arr, _, _ = rois_desc([(0, 0, 0, 32, 2), (1, 2, 2, 4, 4)], (1, 2), 2, 64, 64, filter="bicubic")
    assert d.filter == 2 and len(arr) == 2
    assert rois_desc([(0, 0, 0, 32, 2)], (4, 2), 1, 64, 64, filter="bicubic", fit="letterbox")[0].r.filter == 2
    assert rois_desc([(0, 0, 0, 32, 2)], (4, 2), 1, 64, 64, filter="bicubic", pad=3, layout="nhwc")[0].f.r.filter == 2
    assert rois_args([(0, 0, 32, 2)], (1, 2), 64, 64, filter="bicubic")[0].filter == 2
    # 16 source samples per output and axis where the triangle takes 32
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 34, 2)], (1, 2), 1, 64, 64, filter="bicubic")
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 320, 34)], (20, 20), 1, 512, 64, filter="bicubic", fit="letterbox")
    assert rois_desc([(0, 0, 0, 320, 34)], (20, 20), 1, 512, 64, fit="letterbox")[0].r.filter == 0
    # the Decoder's option reaches the same builder (no instance is made for a bad one)
    for opts in ({"filter": "bicubic"}, {"size": (4, 4), "filter": "lanczos"}, {"size": (4, 4), "filter": 2},
                 {"filter": "triangle"}):
        with pytest.raises(ValueError):
            Decoder({"tensor": opts})


def test_python_surface_rejects_bad_filters():
    from broadway_amd.engine import Engine, rois_desc, tensor_desc
    for kw in ({"filter": "bicubic"}, {"filter": "triangle"}, {"size": (3, 5), "filter": "lanczos"},
               {"size": (3, 5), "filter": 2}, {"size": (3, 5), "filter": "BICUBIC"}, {"size": (3, 5), "filter": 1},
               {"filter": "bicubic", "layout": "nhwc"}):
        with pytest.raises(ValueError):
            tensor_desc((2, 4, 6, 8), **kw)
    with pytest.raises(ValueError):
        rois_desc([(0, 0, 0, 4, 4)], (2, 2), 1, 64, 64, filter="cubic")
    # the Engine's methods check before they touch the library: no instance needed
    eng = object.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 4, 4
    with pytest.raises(ValueError, match="filter"):
        eng.to_tensor([0], [0], size=(4, 4), warps=[(0, (65536, 0, 0, 0, 65536, 0))], filter="bicubic")
    with pytest.raises(ValueError, match="filter"):
        eng.to_tensor([0], [0], filter="bicubic")
    with pytest.raises(ValueError, match="filter"):
        eng.to_tensor([0], [0], rois=[(0, 0, 0, 4, 4)], size=(2, 2), filter="nearest")
    with pytest.raises(ValueError, match="filter"):
        eng.to_accmv([0], [0], size=(4, 4), filter="bicubic")
    with pytest.raises(ValueError, match="filter"):
        eng.to_accres([0], [0], size=(4, 4), filter="bicubic")
    with pytest.raises(ValueError, match="filter"):
        eng.to_accmv([0], [0], filter="triangle")


# ------------------------------------------------------ the host paths ----
OK, PIC_RDY, PARAM_ERR = 0, 2, -1


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    """The program's output lines (tests/test_rois_host.py's build: shift
    excluded from UBSan, as in oracle/Makefile)."""
    td = tmp_path_factory.mktemp("bicubic_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c"),
                                               os.path.join(HERE, "bicubic_host_check.c")]
    cxxsrc = [os.path.join(ROOT, "oracle", "null_device.cpp"), os.path.join(P, "host", "hipback.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=undefined"]
    common = ["-O1", "-g", "-fno-omit-frame-pointer"] + san
    cc, cxx = os.environ.get("CC", "gcc"), os.environ.get("CXX", "g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    jobs = [(f, str(td / (os.path.basename(f) + ".o")), [cc] + common + ["-std=gnu11", "-Wno-unused-parameter"])
            for f in csrc]
    jobs += [(f, str(td / (os.path.basename(f) + ".o")),
              [cxx] + common + ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include"]) for f in cxxsrc]
    procs = [subprocess.Popen(cmd + ["-c", f, "-o", o]) for f, o, cmd in jobs]
    assert all(p.wait() == 0 for p in procs)
    exe = str(td / "bicubic_host_check")
    subprocess.run([cxx] + common + [o for _, o, _ in jobs] + ["-o", exe, "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
        "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
    assert not bad and p.returncode == 0, (p.returncode, bad[:3], p.stderr[-2000:])
    return p.stdout.splitlines()


@pytest.mark.timeout(600)
def test_host_before_headers_filter_2_is_ok_and_a_bad_filter_is_not(host_lines):
    """No headers yet: OK from all six resized calls under the bicubic filter,
    PARAM_ERR under filters 1, -1 and 3."""
    names = ("resized", "fit", "layout", "rois", "rois_fit", "rois_layout")
    assert "before " + " ".join(f"{n} {OK}" for n in names) in host_lines
    for bad in (1, -1, 3):
        want = f"before_bad {bad} " + " ".join(f"{n} {PARAM_ERR}" for n in names)
        assert want in [" ".join(ln.split()) for ln in host_lines], bad


@pytest.mark.timeout(600)
def test_host_calls_hand_the_engine_the_filter(host_lines):
    """Every picture and, after it, its boxes: PIC_RDY through the three forms
    in turn, the engine's descriptor carrying the caller's filter and size; the
    last picture takes the triangle to 5 columns (86 : 5), which the bicubic
    filter refuses."""
    pics = [ln.split() for ln in host_lines if ln.startswith("pic ")]
    boxes = [ln.split() for ln in host_lines if ln.startswith("box ")]
    assert len(pics) == len(boxes) == 4
    for k, (p, b) in enumerate(zip(pics, boxes)):
        want = ["filter", "0", "size", "5,4"] if k == 3 else ["filter", "2", "size", "6,4"]
        assert p[1:6] == [str(k), "form", str(k % 3), "ret", str(PIC_RDY)] and p[6:8] == ["calls", str(2 * k + 1)], p
        assert b[1:6] == [str(k), "form", str(k % 3), "ret", str(PIC_RDY)] and b[6:8] == ["calls", str(2 * k + 2)], b
        assert p[8:] == want and b[8:] == want, (p, b)


@pytest.mark.timeout(600)
def test_host_bad_descriptors_are_refused_without_consuming_a_picture(host_lines):
    """16 bad picture calls in front of every fetch attempt and 15 bad box
    calls after every picture -- filters 1, -1 and 3, 86 columns to 5 and 52
    rows to 3 under the bicubic filter, the unresized layout form with a
    filter --: all PARAM_ERR, none reaches the engine, all 4 pictures arrive."""
    ref = [ln.split() for ln in host_lines if ln.startswith("refused ")]
    assert len(ref) == 1
    refused, tried, pics = int(ref[0][1]), int(ref[0][3]), int(ref[0][5])
    assert pics == 4 and refused == tried and tried >= 16 * 4 + 15 * 4 and (tried - 15 * 4) % 16 == 0
