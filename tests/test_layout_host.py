"""The host side of H264SwDecNextPictureTensorLayout and
H264SwDecLastPictureTensorRoisLayout without a GPU:
tests/layout_host_check.c runs the product host path on the CPU stand-in of the
engine under AddressSanitizer + UBSan, with an engine export that records the
descriptor it is handed."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, PIC_RDY, PARAM_ERR = 0, 2, -1


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's output lines (tests/test_rois_host.py's build: shift
    excluded from UBSan, as in oracle/Makefile)."""
    td = tmp_path_factory.mktemp("layout_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c"),
                                               os.path.join(HERE, "layout_host_check.c")]
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
    exe = str(td / "layout_host_check")
    subprocess.run([cxx] + common + [o for _, o, _ in jobs] + ["-o", exe, "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
        "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
    assert not bad and p.returncode == 0, (p.returncode, bad[:3], p.stderr[-2000:])
    return p.stdout.splitlines()


def calls(lines, what):
    out = []
    for ln in lines:
        f = ln.split()
        if f[0] == what:
            d = dict(zip(f[2:24:2], f[3:24:2]))
            ints = lambda s: tuple(int(v) for v in s.split(","))      # noqa: E731
            out.append(dict(ret=int(d["ret"]), calls=int(d["calls"]), colour=int(d["colour"]), mode=int(d["mode"], 16),
                            layout=int(d["layout"]), fit=int(d["fit"]), size=ints(d["size"]), win=ints(d["win"]),
                            pad=ints(d["pad"]), nrois=int(d["nrois"]), stride=int(d["stride"]),
                            boxes=[ints(b) for b in f[25:]] if what == "box" else None))
    return out


@pytest.mark.timeout(600)
def test_return_codes_before_any_delivery_are_the_mirrored_calls(lines):
    """No headers yet: OK from both calls, as from ...TensorFit and
    ...TensorRoisFit; a bad descriptor is PARAM_ERR even then."""
    assert f"before next {OK} mirrored {OK} rois {OK} mirrored {OK} bad_next {PARAM_ERR} bad_rois {PARAM_ERR}" in lines


@pytest.mark.timeout(600)
def test_picture_call_hands_the_engine_its_descriptor(lines):
    """Every picture: PIC_RDY, the engine's descriptor the caller's -- layout,
    fit, size and pad as given, in the three forms in turn -- with the SPS crop
    window (6, 2, 86, 52) filled in and STREAM resolved from the picture's VUI
    (matrix 1, full range: set 3) and reported; the single-window form (no
    boxes, stride 0)."""
    pics = calls(lines, "pic")
    assert len(pics) == 5
    for k, c in enumerate(pics):
        form = k % 3
        assert (c["ret"], c["calls"], c["colour"], c["mode"], c["layout"]) == (PIC_RDY, 2 * k + 1, 3, 3 << 8, 1), k
        assert c["fit"] == (1 if form == 2 else 0) and c["size"] == ((9, 7) if form else (0, 0)), k
        assert c["win"] == (6, 2, 86, 52) and c["pad"] == ((114, 7, 250) if form == 2 else (0, 0, 0)), k
        assert (c["nrois"], c["stride"]) == (0, 0), k


@pytest.mark.timeout(600)
def test_rois_call_hands_the_engine_its_descriptor(lines):
    """After every picture: PIC_RDY, the window still reserved, the boxes moved
    by the crop offset, packed 3 x 7 x 9 fp16 = 378 bytes apart, stretch and
    letterbox in turn."""
    boxes = calls(lines, "box")
    assert len(boxes) == 5
    for k, c in enumerate(boxes):
        assert (c["ret"], c["calls"], c["colour"], c["mode"], c["layout"]) == (PIC_RDY, 2 * k + 2, 3, 3 << 8, 1), k
        assert c["fit"] == k % 2 and c["size"] == (9, 7) and c["win"] == (0, 0, 0, 0), k
        assert c["pad"] == ((114, 7, 250) if k % 2 else (0, 0, 0)), k
        assert (c["nrois"], c["stride"]) == (2, 378) and c["boxes"] == [(0, 6, 2, 86, 52), (0, 88, 50, 4, 4)], k


@pytest.mark.timeout(600)
def test_bad_descriptors_are_refused_without_consuming_a_picture(lines):
    """18 bad picture calls in front of every fetch attempt (5 pictures and the
    attempts that find none) and 11 bad rois calls after every picture: all
    PARAM_ERR, none reaches the engine, and all 5 pictures still arrive."""
    ref = [ln.split() for ln in lines if ln.startswith("refused ")]
    assert len(ref) == 1
    refused, tried, pics = int(ref[0][1]), int(ref[0][3]), int(ref[0][5])
    assert pics == 5 and refused == tried and tried >= 18 * 5 + 11 * 5 and (tried - 11 * 5) % 18 == 0
