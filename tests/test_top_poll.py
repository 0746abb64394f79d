"""The row wave's top-halo poll (recon_kernels.hip row_pp): the read of the
row above's mailbox entry c is issued at the top of MB c's iteration, once
more before the vertical pass when it came back stale, and again after it
until the entry's tag is the launch's epoch.  Whatever the timing, H(c) must
take the row above's final rows 12..15 of this launch -- never a stale entry
of the launch before, whose mailbox it reuses under a new epoch -- so every
picture of every launch is compared byte for byte with the oracle's decode
(integer work: no tolerance).

Shapes: one MB column (the c > 0 / hdone branch never runs), one MB per row
wave, three columns, and an odd width at which the two row waves' last MBs
differ.  Each run decodes four streams of one size whose deblocking mix
makes the top edge filtered for all, for none and for some MBs of a row.

Flavours: the plain instances, the dependency checker's (H264MI_CHECK=1) and,
at the two larger sizes, the profiling ones (h264mi_engine_profile), which
nothing else in the suite launches."""
import ctypes as C
import functools

import pytest

import oracle as O
from broadway_amd import _lib, gen
from broadway_amd.engine import Capture

pytestmark = pytest.mark.gpu

SIZES = [(1, 3), (2, 4), (3, 5), (13, 9)]
NFRAMES = 9


def _mixes(w, h):
    """(slices, dbf_idc1_pct, dbf_idc2_pct) of the four streams of a run."""
    return [
        (2, 0, 0),                      # idc 0 only: every MB below row 0 filters its top edge
        # idc 2, one slice per MB row.  The generator moves every slice end
        # by up to 3 MBs, so a few MBs next to the boundaries still have the
        # MB above in their own slice: nearly none does ...
        (h, 0, 100),
        (max(2, h - 1), 50, 50),        # idc 1 / 2 mixed, slice boundaries inside rows: some do
        (w * h, 0, 100),                # ... and with a slice per MB, none at all
    ]


@functools.lru_cache(maxsize=None)
def _streams(w, h, ionly):
    """The run's streams and the oracle's pictures of each (computed once,
    shared by every case of the size; read only)."""
    out = []
    for i, (slices, idc1, idc2) in enumerate(_mixes(w, h)):
        s = gen.generate(2, 90 + i, nframes=NFRAMES, w_mbs=w, h_mbs=h, crop_bottom=0, slices=slices,
                         gop=1 if ionly else 5, dbf_idc1_pct=idc1, dbf_idc2_pct=idc2)
        frames, errs = O.decode(s)[:2]
        assert errs == 0 and len(frames) == NFRAMES
        out.append((s, tuple(frames)))
    return tuple(out)


# (pipe, BENCH_DEP_MODE, environment, I-only, MC waves expected at the last launch)
# Frame-pipelined launches always run single-row workgroups with two MC waves,
# so the workgroup shapes are forced at one picture per launch.
SHAPES = {
    "pipe1": (1, None, {}, False, None),
    "pipe1_mc2": (1, None, {"H264MI_MC_WAVES": "2"}, False, 2),
    "pipe1_mc3": (1, None, {"H264MI_MC_WAVES": "3"}, False, 3),
    "pipe1_ionly_mc6": (1, None, {}, True, 6),
    "pipe1_rpw2": (1, None, {"H264MI_RPW": "2"}, False, None),
    "pipe1_rpw3": (1, None, {"H264MI_RPW": "3"}, False, 3),
    # (profiling: two rows per workgroup run the 3-wave build; the engine still reports 2)
    "pipe1_mc2_rpw2": (1, None, {"H264MI_MC_WAVES": "2", "H264MI_RPW": "2"}, False, 2),
    "pipe3_rows": (3, "rows", {}, False, 2),
    "pipe3_cols": (3, "cols", {}, False, 2),
}


# profiling at the sizes whose five rows leave a partial last group at 2 and 3
# rows per workgroup, and more than one MB per row wave
PROF_SIZES = [(3, 5), (13, 9)]
CASES = [(wh, shape, flavour) for wh in SIZES for shape in sorted(SHAPES) for flavour in ("plain", "check", "prof")
         if flavour != "prof" or wh in PROF_SIZES]


@pytest.mark.parametrize("wh,shape,flavour", CASES, ids=[f"{wh[0]}x{wh[1]}-{shape}-{fl}" for wh, shape, fl in CASES])
def test_top_halo_poll_vs_oracle(wh, shape, flavour, monkeypatch):
    """Nine pictures of four streams (top edge filtered for all / none / some
    MBs of a row), one or three pictures of each per launch, so that several
    launches reuse the mailboxes under new epochs; rows or (row, column)
    dependencies between the pictures of a launch; 2, 3 and 6 MC waves per row
    workgroup, two and three rows per workgroup (the LDS mailboxes); each also
    through the dependency-checker instances (H264MI_CHECK=1) and, switched on
    once the run is set up, the profiling instances, whose row-start stamp of
    row 0 of picture 0 shows that one ran."""
    import bench
    pipe, mode, env, ionly, nmc = SHAPES[shape]
    check, prof = flavour == "check", flavour == "prof"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if mode:
        monkeypatch.setenv("BENCH_DEP_MODE", mode)
    if check:
        monkeypatch.setenv("H264MI_CHECK", "1")
    w, h = wh
    data = _streams(w, h, ionly)
    caps = [Capture(s) for s, _ in data]
    refs = [r for _, r in data]
    assert all(c.errors == 0 and c.w_mbs == w and c.h_mbs == h for c in caps)
    n = min(c.npics for c in caps)
    n -= n % pipe
    assert n == NFRAMES
    run = bench.DeviceRun(_lib.mi(), caps, 0, n, pipe)
    try:
        if prof:
            assert run.eng._L.h264mi_engine_profile(run.eng._h, 1, None, 0) == 0
        assert run.P == pipe
        assert len(run.launches) >= 3
        for i, launch in enumerate(run.launches):
            run.launch(i)
            run.eng.sync()
            for step in launch:
                for s, k in enumerate(step):
                    got = run.eng.read(s, int(run.slot_of[k][s])).tobytes()
                    assert got == refs[s][k], f"stream {s} picture {k}"
            if pipe > 1:
                assert run.eng.last_deps() == (1 if mode == "rows" else 2)
        if nmc is not None:
            assert run.eng.last_mc_waves() == nmc
        if check:
            assert run.eng.kernel_name() == "k_wgpp_check"
            assert run.eng.error_bits() == 0
        elif prof:
            assert run.eng.kernel_name() == ("k_wgpp_prof" if pipe > 1 else "k_wgpp")
            rec = (C.c_uint64 * 16)()
            assert run.eng._L.h264mi_engine_profile(run.eng._h, 1, rec, len(rec)) == 0
            assert rec[0] != 0
        else:
            assert run.eng.kernel_name() == "k_wgpp"
        assert run.eng.errors() == 0
    finally:
        run.free()
