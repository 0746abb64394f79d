"""H264SwDecLastPictureTensorRois' host side without a GPU:
tests/rois_host_check.c runs the product host path on the CPU stand-in of the
engine under AddressSanitizer + UBSan, once with an engine export that records
what it is handed and once without one (the backend then has no member for the
call)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, PIC_RDY, PARAM_ERR = 0, 2, -1


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The output lines of the two programs (tests/test_colour.py's build of
    its host check: shift excluded from UBSan, as in oracle/Makefile)."""
    td = tmp_path_factory.mktemp("rois_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c")]
    cxxsrc = [os.path.join(ROOT, "oracle", "null_device.cpp"), os.path.join(P, "host", "hipback.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=undefined"]
    common = ["-O1", "-g", "-fno-omit-frame-pointer"] + san
    cc, cxx = os.environ.get("CC", "gcc"), os.environ.get("CXX", "g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    main = os.path.join(HERE, "rois_host_check.c")
    jobs = [(f, str(td / (os.path.basename(f) + ".o")), [cc] + common + ["-std=gnu11", "-Wno-unused-parameter"])
            for f in csrc]
    jobs += [(f, str(td / (os.path.basename(f) + ".o")),
              [cxx] + common + ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include"]) for f in cxxsrc]
    jobs += [(main, str(td / "with.o"), [cc] + common + ["-std=gnu11"]),
             (main, str(td / "without.o"), [cc] + common + ["-std=gnu11", "-DNO_EXPORT", "-Wno-unused-variable"])]
    procs = [subprocess.Popen(cmd + ["-c", f, "-o", o]) for f, o, cmd in jobs]
    assert all(p.wait() == 0 for p in procs)
    objs = [o for _, o, _ in jobs[:-2]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    out = {}
    for name in ("with", "without"):
        exe = str(td / f"rois_host_check_{name}")
        subprocess.run([cxx] + common + objs + [str(td / f"{name}.o"), "-o", exe, "-lpthread"], check=True)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
            "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
        assert not bad and p.returncode == 0, (name, p.returncode, bad[:3], p.stderr[-2000:])
        out[name] = p.stdout.splitlines()
    return out


def pic_lines(lines):
    out = []
    for ln in lines:
        f = ln.split()
        if f[0] == "pic":
            d = dict(zip(f[2:14:2], f[3:14:2]))
            out.append((int(d["ret"]), int(d["calls"]), int(d["colour"]), int(d["mode"], 16), int(d["pics"]),
                        int(d["stride"]), [tuple(int(v) for v in b.split(",")) for b in f[15:]]))
    return out


@pytest.mark.timeout(600)
def test_call_on_the_cpu_stand_in(runs):
    """Before any picture OK; for every delivered picture PIC_RDY, the boxes
    moved by the SPS crop offset (6, 2), STREAM resolved from the picture's VUI
    (matrix 1, full range: set 3) and reported, one picture, boxes packed
    (3 planes x 7 x 9 fp16 = 378 bytes apart); every bad call refused before it
    reaches the engine; after a decode that delivered nothing, OK."""
    lines = runs["with"]
    assert "before 0" in lines
    pics = pic_lines(lines)
    assert len(pics) == 5
    for k, (ret, calls, colour, mode, n, stride, boxes) in enumerate(pics):
        assert (ret, calls, colour, mode, n, stride) == (PIC_RDY, k + 1, 3, 3 << 8, 1, 378), k
        assert boxes == [(0, 6, 2, 86, 52), (0, 88, 50, 4, 4)], k
    ref = [ln.split() for ln in lines if ln.startswith("refused ")]
    assert len(ref) == 1 and ref[0][1] == ref[0][3] == str(18 * 5)
    after = [ln.split()[1:] for ln in lines if ln.startswith("after_decode")]
    assert len(after) == 1 and len(after[0]) >= 4 and set(after[0]) == {str(OK)}


@pytest.mark.timeout(600)
def test_backend_without_the_member_refuses(runs):
    """No engine export, no backend member: H264SWDEC_PARAM_ERR whenever it is
    called, and there is no host fallback."""
    lines = runs["without"]
    assert f"before {PARAM_ERR}" in lines
    pics = pic_lines(lines)
    assert len(pics) == 5 and {(p[0], p[1], p[2]) for p in pics} == {(PARAM_ERR, 0, -1)}
    after = [ln.split()[1:] for ln in lines if ln.startswith("after_decode")]
    assert len(after) == 1 and set(after[0]) == {str(PARAM_ERR)}
