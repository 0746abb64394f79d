"""The host side of H264SwDecLastPictureTensorWarps without a GPU:
tests/warp_host_check.c runs the product host path on the CPU stand-in of the
engine under AddressSanitizer + UBSan, with an engine export that records the
descriptor and the matrices it is handed."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, PIC_RDY, PARAM_ERR = 0, 2, -1
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
BAD_CALLS = 23              # bad_calls() of the program, in front of every good call


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's output lines (tests/test_layout_host.py's build: shift
    excluded from UBSan, as in oracle/Makefile)."""
    td = tmp_path_factory.mktemp("warp_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c"),
                                               os.path.join(HERE, "warp_host_check.c")]
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
    exe = str(td / "warp_host_check")
    subprocess.run([cxx] + common + [o for _, o, _ in jobs] + ["-o", exe, "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
        "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
    assert not bad and p.returncode == 0, (p.returncode, bad[:3], p.stderr[-2000:])
    return p.stdout.splitlines()


def pic_lines(lines):
    out = []
    ints = lambda s: tuple(int(v) for v in s.split(","))      # noqa: E731
    for ln in lines:
        f = ln.split()
        if f[0] == "pic":
            d = dict(zip(f[2:26:2], f[3:26:2]))
            out.append(dict(form=int(d["form"]), ret=int(d["ret"]), calls=int(d["calls"]), colour=int(d["colour"]),
                            mode=int(d["mode"], 16), pics=int(d["pics"]), stride=int(d["stride"]), win=ints(d["win"]),
                            size=ints(d["size"]), border=int(d["border"]), pad=ints(d["pad"]), layout=int(d["layout"]),
                            warps=[(int(w.split(":")[0]), ints(w.split(":")[1])) for w in f[27:]]))
    return out


@pytest.mark.timeout(600)
def test_return_codes_before_and_after_delivery(lines):
    """No headers yet: OK, and PARAM_ERR for a bad descriptor even then; after
    a decode that delivered nothing: OK again."""
    assert f"before {OK} bad {PARAM_ERR}" in lines
    after = [ln.split()[1:] for ln in lines if ln.startswith("after_decode")]
    assert len(after) == 1 and len(after[0]) >= 4 and set(after[0]) == {str(OK)}


@pytest.mark.timeout(600)
def test_call_hands_the_engine_window_and_matrices(lines):
    """Every picture: PIC_RDY, one picture, warps packed 3 x 7 x 9 fp16 = 378
    bytes apart, STREAM resolved from the picture's VUI (matrix 1, full range:
    set 3) and reported.  The SPS crop offset (6, 2) is applied to the window
    -- the crop window itself (form 0) or the caller's inside it (form 1: (4,
    2, 80, 48) becomes (10, 4, 80, 48)) -- and never to the matrices, which
    arrive as the caller's, extremes included; border, pad and layout as given."""
    pics = pic_lines(lines)
    assert len(pics) == 5
    want = [(0, (65536, 0, 0, 0, 65536, 0)), (0, (INT_MIN, INT_MAX, -1, 1, INT_MAX, INT_MIN))]
    for k, c in enumerate(pics):
        assert (c["form"], c["ret"], c["calls"], c["colour"], c["mode"]) == (k % 2, PIC_RDY, k + 1, 3, 3 << 8), k
        assert (c["pics"], c["stride"], c["size"]) == (1, 378, (9, 7)), k
        assert c["win"] == ((10, 4, 80, 48) if k % 2 else (6, 2, 86, 52)), k
        assert (c["border"], c["pad"], c["layout"]) == ((1, (0, 0, 0), 1) if k % 2 else (0, (114, 7, 250), 0)), k
        assert c["warps"] == want, k


@pytest.mark.timeout(600)
def test_bad_calls_are_refused_without_reaching_the_engine(lines):
    """23 bad calls in front of every good one: all PARAM_ERR, none reaches the
    engine (the good calls' count stays k + 1), and all 5 pictures arrive."""
    ref = [ln.split() for ln in lines if ln.startswith("refused ")]
    assert len(ref) == 1
    assert (int(ref[0][1]), int(ref[0][3]), int(ref[0][5])) == (BAD_CALLS * 5, BAD_CALLS * 5, 5)
