"""The MC reference-window geometry on the CPU (tests/mc_window_check.cpp):
broadway_amd/csrc/common/mc_window.h -- the one statement of which bytes of a
reference slot a macroblock's motion compensation reads, which k_wgpp's
dependency checker and the host's MbRec.i4 encoding and line count are built
on, and which the kernel's loads and column waits spell out -- against a
brute-force list of the touched bytes.  Ten
picture sizes (W16 % 128 zero and non-zero, chroma rows narrower than a line,
padded chroma rows, a 16-sample-wide picture), MBs at the corners, the edges
and inside, every block, MVs leaving the picture by more than a window on
every side in every fractional phase:
  containment  the columns the interpolation reads lie inside the load, the
               load inside its row and plane;
  lane map     64 lanes load every (block, row) of luma and every (block,
               component, row) of chroma, inside the rows the waits hold the
               lane to;
  lines        per access, the MB rows and last MB column the header gives
               equal those of the bytes of the 128-B lines it touches; the
               spans (mcw_span_cells) cover their accesses, exactly where the
               header says so, and a copy of dep_wait_cols' hand-written
               lines -- the kernel does not call the header there -- gives
               the same spans;
  host         for random inter records, the header's MbRec.i4 rows and line
               count equal the ones counted byte by byte.
Built with AddressSanitizer + UBSan; integer work, no tolerance."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mc_window_check") / "mc_window_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                   [os.path.join(HERE, "mc_window_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def test_header_equals_touched_bytes(lines):
    words = lines[-1].replace(",", "").split()
    assert words[0] == "ok" and words[-2:] == ["0", "mismatches"], lines[-1]
    assert int(words[1]) == 10 and words[2] == "sizes"


def test_sweep_reaches_the_edges(lines):
    """The sweep is not run on windows that stay inside: a good part leave the
    picture, and some accesses lie on lines that hold the end of an earlier row."""
    words = lines[-2].replace("(", "").split()
    windows, leaving, accesses, two_rows, records = (int(words[i]) for i in (0, 2, 6, 8, 15))
    assert windows >= 10**6 and leaving > windows // 4
    assert accesses >= 5 * windows and two_rows > 0 and records > 0
