"""The seeded draw of the differential sweep (tests/test_reference_sweep.py:
reference decoder against the CPU oracle; tests/test_gpu_parity.py: a sample
of the same streams, GPU against the oracle).

Stream `seed` is gen.generate(2, seed, **ov) with (ov, no_reorder) =
draw(seed, damaged): every knob below is drawn independently from its list by
a random.Random(seed), so one seed reproduces one stream.  Clean streams take
seeds CLEAN_BASE + i, damaged ones DAMAGED_BASE + i.
"""
import random

CLEAN_BASE, N_CLEAN = 100000, 400
DAMAGED_BASE, N_DAMAGED = 300000, 800

SIZES = [(1, 1), (2, 1), (1, 3), (3, 2), (5, 4), (7, 3), (4, 6), (11, 2), (2, 9)]      # MBs
CHROMA_QP_OFFSETS = [-12, -5, 0, 3, 12]
# knob -> values, drawn in this order after the size-dependent ones
KNOBS = [
    ("qp_delta", [0, 2, 6, 25]),    # 26 would be an out-of-range mb_qp_delta: damage, not a clean stream
    ("dbf_idc1_pct", [0, 30, 100]), ("dbf_idc2_pct", [0, 30, 60]), ("dbf_off", [0, 3, 6]),
    ("num_ref_frames", [1, 2, 4, 16]),
    ("cip", [0, 1]),
    ("coef_pct", [0, 20, 60, 95]), ("level_tail_pct", [0, 5, 30]),
    ("mv_jitter", [0, 4, 40, 400]), ("offpic_pct", [0, 10, 50]),
    ("log2_max_frame_num", [4, 5, 8, 16]),
    ("i4_rem_pct", [0, 50, 100]), ("p8x8_ref0_pct", [0, 50, 100]),
    ("nonref_pct", [0, 30]), ("ref_mod_pct", [0, 50]), ("mmco_pct", [0, 40]), ("lt_idr_pct", [0, 50]),
]
# MB-type mixes (weights; {} = the generator's own): P pictures of 8x8
# partitions only, mostly skipped, intra-heavy; I MBs all I4x4, all I16x16,
# a third I_PCM
P_MIXES = [{}, dict(pm_skip=0, pm_16x16=0, pm_16x8=0, pm_8x16=0, pm_8x8=100, pm_intra=0),
           dict(pm_skip=70, pm_16x16=10, pm_16x8=5, pm_8x16=5, pm_8x8=5, pm_intra=5),
           dict(pm_skip=5, pm_16x16=5, pm_16x8=20, pm_8x16=20, pm_8x8=10, pm_intra=40)]
I_MIXES = [{}, dict(im_i4=100, im_i16=0, im_pcm=0), dict(im_i4=0, im_i16=100, im_pcm=0),
           dict(im_i4=40, im_i16=30, im_pcm=30)]
VUI_KNOBS = [("vui_matrix", [0, 1, 5, 6]), ("vui_full_range", [0, 1])]
DAMAGE_KNOBS = [
    ("err_range_pct", [0, 20]),
    ("drop_slice_pct", [0, 15]), ("trunc_slice_pct", [0, 15]), ("drop_pic_pct", [0, 15]),
    ("gaps_allowed", [0, 1]),
]


def draw(seed, damaged):
    """(generator overrides, no_reorder) of sweep stream `seed`."""
    r = random.Random(seed)
    w, h = r.choice(SIZES)
    ov = dict(w_mbs=w, h_mbs=h, nframes=r.choice([4, 7, 10]), gop=r.choice([1, 3, 5, 20]),
              slices=r.choice([1, 2, 3, w * h]))
    crop = dict(crop_right=r.choice([0, 2, 6]), crop_bottom=r.choice([0, 2, 8]),
                crop_left=r.choice([0, 2]), crop_top=r.choice([0, 2]))
    if crop["crop_left"] + crop["crop_right"] >= 16 * w or crop["crop_top"] + crop["crop_bottom"] >= 16 * h:
        crop = dict.fromkeys(crop, 0)       # the window would be empty
    ov.update(crop)
    ov["qp_min"] = r.choice([0, 10, 26, 40])
    ov["qp_max"] = min(51, ov["qp_min"] + r.choice([0, 5, 11, 51]))
    # a damaged stream takes its offset from its seed: each value in exactly
    # a fifth of them, whatever the other knobs draw
    off = r.choice(CHROMA_QP_OFFSETS)
    ov["chroma_qp_offset"] = CHROMA_QP_OFFSETS[seed % 5] if damaged else off
    ov["poc_type"] = r.choice([0, 2])
    swap = r.choice([0, 1])
    ov["poc_swap"] = swap if ov["poc_type"] == 0 else 0
    for name, values in KNOBS + (DAMAGE_KNOBS if damaged else []):
        ov[name] = r.choice(values)
    no_reorder = bool(r.choice([0, 1]))
    ov.update(r.choice(P_MIXES))
    ov.update(r.choice(I_MIXES))
    for name, values in VUI_KNOBS:
        ov[name] = r.choice(values)
    return ov, no_reorder


def seeds(damaged):
    base, n = (DAMAGED_BASE, N_DAMAGED) if damaged else (CLEAN_BASE, N_CLEAN)
    return range(base, base + n)


def small_sample(damaged, n, max_w=7, max_h=3):
    """The first n sweep seeds whose picture is at most max_w x max_h MBs
    and, of the damaged sweep, whose draw turns some damage on."""
    out = []
    for s in seeds(damaged):
        ov, _ = draw(s, damaged)
        if ov["w_mbs"] > max_w or ov["h_mbs"] > max_h:
            continue
        if damaged and not any(ov[k] for k, _ in DAMAGE_KNOBS[:4]):
            continue
        out.append(s)
        if len(out) == n:
            return out
    raise AssertionError("the sweep holds fewer small streams than asked for")
