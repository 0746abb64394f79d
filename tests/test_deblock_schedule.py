"""The two-step deblocking pass's schedule on the CPU
(tests/deblock_schedule_check.cpp): a 64-lane wave driven by the lane map the
kernel ships (broadway_amd/csrc/hip/deblock_lanes.h) -- step A the MB edge of
every line, step B every internal edge at once with the one p2 hand-over --
must leave exactly the samples that a plain restatement of 8.7.2.3 / 8.7.2.4
leaves when it runs the edges of a line one after another.  Every bS
combination (edge 0: 0..4, edges 1..3: 0..3; chroma: its two edges), the
(alpha, beta, tc0) of indexA / indexB 0..51 from common/tables.c, random lines
of several spreads, flat, step and ramp lines, more than 10^6 lines per plane
and direction, rows (dword and 16-bit stores) and columns (byte stores).  The
program first proves from the header alone, per step and direction: no sample
has two owners or is stored twice, every sample the sequential filter can
change has an owner, and a lane's filter reads nothing a lane of an earlier
edge owns in the step but the p2 it is handed.  Built with AddressSanitizer +
UBSan; integer work, no tolerance."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "broadway_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    td = tmp_path_factory.mktemp("deblock_schedule_check")
    exe, tables = str(td / "deblock_schedule_check"), str(td / "tables.o")
    subprocess.run([os.environ.get("CC", "gcc")] + SAN + ["-c", os.path.join(CSRC, "common", "tables.c"), "-o", tables],
                   check=True)
    subprocess.run([os.environ.get("CXX", "g++")] + SAN + ["-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "deblock_schedule_check.cpp"), tables, "-o", exe, "-lpthread"], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-4000:])
    return p.stdout.splitlines()


def test_schedule_equals_edge_order(lines):
    """5 x 4^3 luma and 5 x 4 chroma bS combinations, both directions."""
    assert lines[-1] == "ok 320 luma 20 chroma bS combinations, 2 directions, 0 mismatches"


def test_line_counts(lines):
    """At least 10^6 lines per plane and direction, and the filter changes a
    good part of them (the check is not run on lines it leaves alone)."""
    words = lines[-2].replace(";", "").split()
    luma, chroma, changed = int(words[3]), int(words[5]), int(words[7])
    assert luma >= 10**6 and chroma >= 10**6
    assert changed > (luma + chroma) // 10
