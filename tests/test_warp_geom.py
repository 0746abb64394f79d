"""Where the affine-warped export samples,
broadway_amd/csrc/common/warp_geom.h, proven on the CPU: tests/warp_geom_check.c
walks warp_taps over extreme and random matrices under AddressSanitizer + UBSan
and asserts that no tap position leaves the window; its digest over 4096
generated cases is reproduced by the Python oracle (tests/_warp.py), which ties
the oracle's geometry to the header the kernel takes its taps from."""
import os
import subprocess

import pytest

import _warp as W

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("warp_geom_check")
    exe = str(td / "warp_geom_check")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "warp_geom_check.c"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    return p.stdout.splitlines()


def test_no_tap_leaves_the_window(lines):
    """Every matrix of the coefficient sweep (11^6, two windows, both borders,
    three outputs each) and the random cases against the definition in wide
    integers; every tile called outside holds no sample."""
    assert lines[0] == f"sweep {11 ** 6} {11 ** 6 * 12} ok"
    f = lines[1].split()
    assert f[0] == "random" and int(f[1]) == 64 * 24 * 16 * 2 and f[2] == "tiles_outside" and int(f[3]) > 1000 and \
        f[4] == "ok"


def test_the_oracle_reproduces_the_digest(lines):
    assert lines[2] == f"digest {W.geometry_digest():016x}"


def test_oracle_taps_at_the_window_edges():
    """taps_one by hand: half a sample left of a 4 x 2 window, and on its last
    sample."""
    m = (65536, 0, -32768, 0, 65536, 0)                 # x = j - 0.5
    assert W.taps_one(m, 0, 0, 4, 2, W.CONSTANT) == (128, 0, 0, 0, 0, 1, 0b1010)
    assert W.taps_one(m, 0, 0, 4, 2, W.REPLICATE) == (128, 0, 0, 0, 0, 1, 15)
    assert W.taps_one(W.IDENTITY, 1, 3, 4, 2, W.CONSTANT) == (0, 0, 3, 3, 1, 1, 0b0001)
    assert W.taps_one((0, 0, -2 ** 31, 0, 0, 2 ** 31 - 1), 5, 5, 4, 2, W.CONSTANT)[6] == 0
