"""The host side of H264SwDecNextPictureTensorDest without a GPU:
tests/dest_host_check.c runs the product host path on the CPU stand-in of the
engine under AddressSanitizer + UBSan, with an engine export that records what
it is handed -- and, built a second time without that export, on a backend that
has no export_tensor_dest member."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, PIC_RDY, PARAM_ERR = 0, 2, -1


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(lines with the export, lines without it): tests/test_layout_host.py's
    build, the check program compiled twice over the same objects."""
    td = tmp_path_factory.mktemp("dest_host_check")
    P = os.path.join(ROOT, "broadway_amd", "csrc")
    check = os.path.join(HERE, "dest_host_check.c")
    csrc = [os.path.join(P, f) for f in (
        "common/bits.c", "common/tables.c", "common/cavlc.c", "common/mbctx.c", "common/resid.c", "host/syntax.c",
        "host/slicedata.c", "host/dpb.c", "host/decoder.c", "host/conceal.c", "host/specparse.c", "host/api.c",
        "host/capture.c", "gen/h264gen.c")] + [os.path.join(ROOT, "oracle", "recon_cpu.c")]
    cxxsrc = [os.path.join(ROOT, "oracle", "null_device.cpp"), os.path.join(P, "host", "hipback.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=undefined"]
    common = ["-O1", "-g", "-fno-omit-frame-pointer"] + san
    cc, cxx = os.environ.get("CC", "gcc"), os.environ.get("CXX", "g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    ccmd = [cc] + common + ["-std=gnu11", "-Wno-unused-parameter"]
    jobs = [(f, str(td / (os.path.basename(f) + ".o")), ccmd) for f in csrc]
    jobs += [(f, str(td / (os.path.basename(f) + ".o")),
              [cxx] + common + ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include"]) for f in cxxsrc]
    mains = [(check, str(td / "with.o"), ccmd), (check, str(td / "without.o"), ccmd + ["-DNO_DEST_EXPORT"])]
    procs = [subprocess.Popen(cmd + ["-c", f, "-o", o]) for f, o, cmd in jobs + mains]
    assert all(p.wait() == 0 for p in procs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", H264MI_PARSE_THREADS="2")
    out = []
    for _, main, _ in mains:
        exe = main[:-2]
        subprocess.run([cxx] + common + [o for _, o, _ in jobs] + [main, "-o", exe, "-lpthread"], check=True)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        bad = [ln for ln in p.stderr.splitlines() if any(r in ln for r in (
            "ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))]
        assert not bad and p.returncode == 0, (p.returncode, bad[:3], p.stderr[-2000:])
        out.append(p.stdout.splitlines())
    return out


def pics(lines):
    out = []
    for ln in lines:
        f = ln.split()
        if f[0] == "pic":
            d = dict(zip(f[2::2], f[3::2]))
            ints = lambda s: tuple(int(v) for v in s.split(","))      # noqa: E731
            out.append(dict(ret=int(d["ret"]), calls=int(d["calls"]), layout=int(d["layout"]), size=ints(d["size"]),
                            win=ints(d["win"]), dest=ints(d["dest"]), null=int(d["null"]), dst=int(d["dst"]),
                            nrois=int(d["nrois"]), stride=int(d["stride"]), n=int(d["n"])))
    return out


@pytest.mark.timeout(600)
def test_return_codes_before_any_delivery(programs):
    """No headers yet: OK as from the call it extends; clip = 2 is PARAM_ERR even then."""
    assert f"before dest {OK} bad {PARAM_ERR}" in programs[0]


@pytest.mark.timeout(600)
def test_descriptor_and_destination_arrive_unchanged(programs):
    """Four pictures through the call, planar unresized and interleaved 9 x 7
    in turn: PIC_RDY, the engine's layout descriptor the caller's with the SPS
    crop window (6, 2, 86, 52) filled in, the destination's five fields as
    given (NULL stays NULL), d_dst the caller's pointer, one picture, the
    single-window form (no boxes, out_stride 0)."""
    got = pics(programs[0])
    assert len(got) == 4
    for k, c in enumerate(got):
        form = k % 2
        assert (c["ret"], c["calls"], c["layout"], c["n"], c["nrois"], c["stride"]) == (PIC_RDY, k + 1, form, 1, 0, 0), k
        assert c["size"] == ((9, 7) if form else (0, 0)) and c["win"] == (6, 2, 86, 52), k
        assert c["dst"] == 2 * (k % 4), k
        if k % 4 == 3:
            assert c["null"] == 1, k
        else:
            assert c["null"] == 0 and c["dest"] == ((64, 0, 0, 1, 0) if form else (176, 53 * 176, 0, 1, 0)), k


@pytest.mark.timeout(600)
def test_bad_destinations_are_refused_with_the_picture_left_in_the_dpb(programs):
    """14 bad calls (clip = 2 first) in front of every fetch: all PARAM_ERR,
    none reaches the engine; every third picture is then taken by the plain
    H264SwDecNextPicture right after them, and all 6 pictures arrive."""
    lines = programs[0]
    ref = [ln.split() for ln in lines if ln.startswith("refused ")]
    assert len(ref) == 1
    refused, tried = int(ref[0][1]), int(ref[0][3])
    assert refused == tried and tried >= 14 * 6 and tried % 14 == 0
    assert "plain 2 dest 4" in lines


@pytest.mark.timeout(600)
def test_backend_without_the_member_is_param_err(programs):
    """No h264mi_engine_export_tensor_dest in the program: the weak reference
    is NULL, the member absent, the call PARAM_ERR, and the plain call still
    delivers all 6 pictures."""
    assert f"missing {PARAM_ERR} calls 0 plain 6" in programs[1]
