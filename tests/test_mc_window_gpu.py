"""Frame-pipelined launches under the dependency checker at picture widths
whose luma rows do not end on 128-B lines (9 and 13 MBs: W16 % 128 != 0), with
no hook injected: dep_wait_cols' "a line holds the end of an earlier row"
case (stated in broadway_amd/csrc/common/mc_window.h, mcw_span_cells) and the
checker's walk over that header's accesses run clean where they matter --
the clean checker runs of tests/test_depcheck.py are all 1080p, whose rows
end on lines.  Two and three pictures per launch, whole-row and column waits;
every picture byte for byte against the oracle's decode (integer work: no
tolerance), no checker bit.

The streams must exercise the geometry: counted from the captured records on
the CPU, with the window rule restated in numpy as in tests/test_ref_lines.py,
luma windows clamped at the left, the right, the top and the bottom edge, and
touched luma lines that hold bytes of two rows, must all occur at each size.
(Two sample rows: MB rows start 256 w bytes apart, so no line holds bytes of
two MB rows at any width -- tests/mc_window_check.cpp proves it -- and the
end of an earlier sample row is what sends dep_wait_cols to the row's last
column.)"""
import functools

import numpy as np
import pytest

import oracle as O
from _mbinfo import MBREC, MBT_SKIP
from broadway_amd import _lib, gen
from broadway_amd.engine import Capture

NFRAMES = 6
SEEDS = {(9, 5): (60, 61, 62), (13, 7): (63, 64, 65)}


@functools.lru_cache(maxsize=None)
def _streams(w, h):
    """The size's streams and the oracle's pictures of each (computed once,
    shared by every case of the size; read only)."""
    out = []
    for seed in SEEDS[(w, h)]:
        s = gen.generate(2, seed, nframes=NFRAMES, gop=NFRAMES, slices=2, crop_bottom=0, offpic_pct=25, mv_jitter=64,
                         w_mbs=w, h_mbs=h)
        frames, errs = O.decode(s)[:2]
        assert errs == 0 and len(frames) == NFRAMES
        out.append((s, tuple(frames)))
    return tuple(out)


def edge_counts(rec, w, h):
    """Luma windows of the inter MBs clamped left, right, top, bottom, and
    the touched luma lines that hold bytes of two rows."""
    W16, H16 = w * 16, h * 16
    b = np.arange(16)
    bx = ((b >> 2) & 1) * 2 + (b & 1)
    by = ((b >> 3) & 1) * 2 + ((b >> 1) & 1)
    inter = np.flatnonzero(rec["type"] <= MBT_SKIP)
    mbx, mby = (inter % w)[:, None], (inter // w)[:, None]
    mvx, mvy = rec["mv"][inter, :, 0].astype(np.int64), rec["mv"][inter, :, 1].astype(np.int64)
    x0 = mbx * 16 + bx * 4 + (mvx >> 2) - 2
    y0 = mby * 16 + by * 4 + (mvy >> 2) - 2
    ax = np.clip(x0 & ~3, 0, W16 - 12)
    lines = set()
    for k in range(9):
        o = np.clip(y0 + k, 0, H16 - 1) * W16 + ax
        lines.update((o // 128).ravel().tolist(), ((o + 11) // 128).ravel().tolist())
    two_rows = sum(1 for ln in lines if (ln * 128) // W16 != (ln * 128 + 127) // W16)
    return np.array([(x0 < 0).sum(), (x0 + 8 > W16 - 1).sum(), (y0 < 0).sum(), (y0 + 8 > H16 - 1).sum(), two_rows])


@pytest.mark.parametrize("w,h", sorted(SEEDS))
def test_streams_reach_every_edge(w, h):
    """A condition on the inputs of the GPU cases below; runs without a GPU."""
    total = np.zeros(5, dtype=np.int64)
    for s, _ in _streams(w, h):
        cap = Capture(s)
        assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs, cap.npics) == (w, h, NFRAMES)
        for i in range(1, cap.npics):
            total += edge_counts(np.frombuffer(cap.records_bytes(i), dtype=MBREC), w, h)
    assert w * 16 % 128 != 0
    assert (total > 0).all(), dict(zip(("left", "right", "top", "bottom", "two_row_lines"), total.tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", sorted(SEEDS))
@pytest.mark.parametrize("mode", ["rows", "cols"])
@pytest.mark.parametrize("pipe", [2, 3])
def test_pipelined_checker_clean_vs_oracle(w, h, mode, pipe, monkeypatch):
    import bench
    monkeypatch.setenv("BENCH_DEP_MODE", mode)
    monkeypatch.setenv("H264MI_CHECK", "1")
    data = _streams(w, h)
    caps = [Capture(s) for s, _ in data]
    refs = [r for _, r in data]
    run = bench.DeviceRun(_lib.mi(), caps, 0, NFRAMES, pipe)
    try:
        assert run.P == pipe and len(run.launches) == NFRAMES // pipe
        for i, launch in enumerate(run.launches):
            run.launch(i)
            run.eng.sync()
            for step in launch:
                for s, k in enumerate(step):
                    got = run.eng.read(s, int(run.slot_of[k][s])).tobytes()
                    assert got == refs[s][k], f"stream {s} picture {k}"
            assert run.eng.last_deps() == (1 if mode == "rows" else 2)
        assert run.eng.kernel_name() == "k_wgpp_check"
        assert run.eng.error_bits() == 0, f"dependency checker flags {run.eng.error_bits():#x}"
        assert run.eng.errors() == 0
    finally:
        run.free()
