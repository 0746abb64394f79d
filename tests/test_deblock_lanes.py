"""The row wave's deblocking passes (recon_kernels.hip deblock_dir): two steps
per pass on the lane map of broadway_amd/csrc/hip/deblock_lanes.h -- the MB
edge of every line, then all internal edges at once with one cross-lane
hand-over.  Every picture is compared byte for byte with the oracle's decode
(integer work: no tolerance).

Sizes in MBs: 1x1 (internal edges only), 2x1 (the left MB edge and the hdone
branch), 1x2 (the top MB edge and the mailbox), 3x3 (both row waves and the
hand-off patch) and 5x4 (an odd width: the two row waves' last MBs differ).
Each run decodes four streams of one size, deblocking on everywhere:
  0  skip-like: no intra MBs in P pictures, no coefficients -- the
     wave-uniform skips of both steps fire
  1  coded inter at QP 30..44: every edge has bS >= 1
  2  intra-rich P pictures at the same QP: bS 4 on MB edges, 3 inside;
     carries a non-zero chroma_qp_offset (the chroma threshold classes differ)
  3  QP 10..20: the thresholds switch the filter off
Shapes: one picture per launch with 2 and 3 MC waves, three rows per
workgroup, and three pictures per launch with row dependencies.  Flavours:
the plain instances and the dependency checker's (H264MI_CHECK=1)."""
import functools

import numpy as np
import pytest

import oracle as O
from _mbinfo import MBREC, MBT_I4x4, MBT_INTER, MBT_SKIP
from broadway_amd import _lib, gen
from broadway_amd.engine import Capture

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 4)]
NFRAMES = 6

MIXES = [
    dict(pm_intra=0, coef_pct=0),
    dict(pm_intra=0, coef_pct=90, qp_min=30, qp_max=44),
    dict(pm_intra=40, coef_pct=90, qp_min=30, qp_max=44, chroma_qp_offset=-5),
    dict(qp_min=10, qp_max=20),
]


@functools.lru_cache(maxsize=None)
def _streams(w, h):
    """The run's streams and the oracle's pictures of each (computed once,
    shared by every case of the size; read only)."""
    out = []
    for i, mix in enumerate(MIXES):
        s = gen.generate(2, 40 + i, nframes=NFRAMES, w_mbs=w, h_mbs=h, crop_bottom=0, slices=1, gop=NFRAMES,
                         dbf_idc1_pct=0, dbf_idc2_pct=0, **mix)
        frames, errs = O.decode(s)[:2]
        assert errs == 0 and len(frames) == NFRAMES
        out.append((s, tuple(frames)))
    return tuple(out)


# (pipe, BENCH_DEP_MODE, environment, MC waves expected at the last launch)
SHAPES = {
    "pipe1_mc2": (1, None, {"H264MI_MC_WAVES": "2"}, 2),
    "pipe1_mc3": (1, None, {"H264MI_MC_WAVES": "3"}, 3),
    "pipe1_rpw3": (1, None, {"H264MI_RPW": "3"}, None),
    "pipe3_rows": (3, "rows", {}, 2),
}
CASES = [(wh, shape, flavour) for wh in SIZES for shape in sorted(SHAPES) for flavour in ("plain", "check")]


def _p_records(cap):
    """MB records of the P pictures (every picture after the first: one GOP)."""
    return np.concatenate([np.frombuffer(cap.records_bytes(i), dtype=MBREC) for i in range(1, cap.npics)])


@pytest.mark.parametrize("wh,shape,flavour", CASES, ids=[f"{wh[0]}x{wh[1]}-{shape}-{fl}" for wh, shape, fl in CASES])
def test_deblock_passes_vs_oracle(wh, shape, flavour, monkeypatch):
    """Six pictures (one I, five P) of the four streams, every picture byte
    for byte; the streams' parsed records hold the mix they are named for."""
    import bench
    pipe, mode, env, nmc = SHAPES[shape]
    check = flavour == "check"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if mode:
        monkeypatch.setenv("BENCH_DEP_MODE", mode)
    if check:
        monkeypatch.setenv("H264MI_CHECK", "1")
    w, h = wh
    data = _streams(w, h)
    caps = [Capture(s) for s, _ in data]
    refs = [r for _, r in data]
    assert all(c.errors == 0 and c.w_mbs == w and c.h_mbs == h and c.npics == NFRAMES for c in caps)
    # the mixes hold what they name
    r0, r1, r2 = _p_records(caps[0]), _p_records(caps[1]), _p_records(caps[2])
    assert (r0["type"] <= MBT_SKIP).all() and (r0["cbits"] == 0).all()
    assert (r1["type"] <= MBT_SKIP).all() and ((r1["type"] == MBT_INTER) & (r1["cbits"] != 0)).any()
    assert (r2["type"] >= MBT_I4x4).any()
    n = NFRAMES
    run = bench.DeviceRun(_lib.mi(), caps, 0, n, pipe)
    try:
        assert run.P == pipe
        assert len(run.launches) == n // pipe
        for i, launch in enumerate(run.launches):
            run.launch(i)
            run.eng.sync()
            for step in launch:
                for s, k in enumerate(step):
                    got = run.eng.read(s, int(run.slot_of[k][s])).tobytes()
                    assert got == refs[s][k], f"stream {s} picture {k}"
            if pipe > 1:
                assert run.eng.last_deps() == 1
        if nmc is not None:
            assert run.eng.last_mc_waves() == nmc
        if check:
            assert run.eng.kernel_name() == "k_wgpp_check"
            assert run.eng.error_bits() == 0
        else:
            assert run.eng.kernel_name() == "k_wgpp"
        assert run.eng.errors() == 0
    finally:
        run.free()
