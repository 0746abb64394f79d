"""k_wgpp's one list of instances and the selection among them
(broadway_amd/csrc/hip/wgpp_variants.h), on the CPU: tests/wgpp_variant_check.cpp
holds the expected instance, diagnostic name and event placement of every
launch shape the engine can produce -- frame-pipelined x {rows, cols} and
single-step x (MC waves, rows per workgroup) in {(3,1), (3,2), (3,3), (2,1),
(2,2), (6,1)}, each plain, profiling, checker and both -- and asserts them, the
block size 64 * (NMC + 2) * RPW <= 1024, that the list has no duplicate and no
instance that nothing selects, and that the shapes launch_batch cannot ask for
find none.  Built with AddressSanitizer + UBSan; the header is plain C++17."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "broadway_amd", "csrc", "hip", "wgpp_variants.h")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("wgpp_variant_check")
    exe = str(td / "wgpp_variant_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "wgpp_variant_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-4000:])
    return p.stdout.splitlines()


def test_selection_table(lines):
    """8 frame-pipelined and 6 x 4 x 2 single-step inputs (both engine
    dependency modes), 23 instances."""
    assert lines[-1] == "ok 56 inputs 23 variants"
    assert sum(" -> <" in ln for ln in lines) == 56


def test_unproducible_shapes_find_no_instance(lines):
    """(2 waves, 3 rows), (6 waves, 2 or 3 rows), and every frame-pipelined
    shape but (2 waves, 1 row): four flavours, two modes each."""
    assert sum(ln.endswith("-> none") for ln in lines) == (3 + 8) * 4 * 2


def test_list_has_23_rows():
    """One X(...) row per instance in the header's list."""
    with open(HEADER) as f:
        src = f.read()
    body = src[src.index("#define WGPP_VARIANTS(X)"):src.index("struct WgppVariant")]
    assert sum(ln.lstrip().startswith("X(") for ln in body.splitlines()) == 23
