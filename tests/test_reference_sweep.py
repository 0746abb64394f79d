"""Differential sweep: the reference decoder against the CPU oracle over
random knob combinations of the stream generator (tests/_sweep.py).

golden.json pins the oracle to the reference at some forty fixed streams, each
with few knobs on; here every stream draws every knob at once.  The oracle is
the expected value of every generated stream in the GPU tests, so what this
sweep holds, they inherit.  CPU only; needs the reference build
(oracle/_ref/refdec) and is skipped where that is absent.
"""
import os

import pytest

import oracle as O
import _sweep
from _golden import md5s
from broadway_amd import gen

needs_refdec = pytest.mark.skipif(not os.path.exists(O.REFDEC), reason="reference build not present")


def compare(seed, damaged):
    """None if reference and oracle agree on stream `seed`, else one line that
    reproduces the difference.  A stream that cannot be generated or that a
    decoder returns nothing for is a failure like any other."""
    ov, nr = _sweep.draw(seed, damaged)
    where = f"seed {seed}: gen.generate(2, {seed}, **{ov}), no_reorder={nr}"
    try:
        s = gen.generate(2, seed, **ov)
        ref_frames, ref_pics = O.refdec_frames(s, no_reorder=nr, info=True)
        frames, _, _, _, _, pics = O.decode(s, no_reorder=nr, info=True)
    except Exception as ex:
        return f"{where}: {type(ex).__name__}: {ex}"
    if not s or not ref_frames or not frames:
        return f"{where}: empty ({len(s)} stream bytes, {len(ref_frames)} reference pictures, {len(frames)} oracle)"
    a, b = md5s(ref_frames), md5s(frames)
    if a != b:
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        return f"{where}: picture {k} of {len(a)} (oracle {len(b)}) differs"
    if [tuple(p) for p in ref_pics] != pics:
        k = next((i for i, (x, y) in enumerate(zip(ref_pics, pics)) if tuple(x) != y), min(len(ref_pics), len(pics)))
        return f"{where}: (picId, isIdr, nbrOfErrMBs) of picture {k} differs: {ref_pics[k:k + 1]} != {pics[k:k + 1]}"
    return None


def sweep(damaged):
    bad = [m for m in (compare(s, damaged) for s in _sweep.seeds(damaged)) if m]
    n = len(_sweep.seeds(damaged))
    assert not bad, f"{len(bad)} of {n} streams differ:\n" + "\n".join(bad[:10])


@needs_refdec
def test_clean_streams_reference_vs_oracle():
    """400 clean streams: same pictures (MD5), picture ids, IDR flags and a
    zero nbrOfErrMBs from both decoders.  Measured: 0 of 400 differ, with and
    without the concealed-MB chroma QP rule."""
    assert _sweep.N_CLEAN >= 400
    sweep(False)


@needs_refdec
def test_damaged_streams_reference_vs_oracle():
    """800 damaged streams (residuals out of range, lost and truncated slices,
    lost pictures, gaps in frame_num, over the clean knobs): same pictures,
    picture ids, IDR flags and nbrOfErrMBs.

    Every non-zero chroma_qp_offset is in 160 of them: a chroma edge between
    a concealed MB and a decoded one takes both sides' chroma QP through the
    q-side MB's offset, 0 for a concealed MB.  Measured with one
    chroma QP per MB averaged over the edge instead: 153 of 800 differ (53 at
    offset -12, 35 at -5, 28 at 3, 37 at 12, none at 0), in samples only; with
    the rule, 0 of 800.

    The seed base is one at which every stream leaves at least one picture: a
    short stream can lose all of them (seed 200028: three pictures dropped and
    the IDR's only slice failing), and both decoders then return nothing,
    which compare() counts as a failure."""
    assert _sweep.N_DAMAGED >= 800
    per_offset = {o: 0 for o in _sweep.CHROMA_QP_OFFSETS}
    for s in _sweep.seeds(True):
        per_offset[_sweep.draw(s, True)[0]["chroma_qp_offset"]] += 1
    assert all(n >= 100 for o, n in per_offset.items() if o), per_offset
    sweep(True)
