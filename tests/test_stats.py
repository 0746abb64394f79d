"""Picture statistics export (stats.hip k_stats): per item -- a
window of a picture, or a box of a box list -- P plane records of L int64 words
(count, sum, sumsq, min, max, sad, ssd, 0, [256 bins]) from one pass over the
source -- h264mi_stats_device_pitch, h264mi_engine_export_stats
(Engine.to_stats) and H264SwDecLastPictureStats (Decoder.stats).

Every comparison is exact equality of integers against tests/_stats.py's numpy
oracle (tests/test_stats_cpu.py ties it to a brute-force loop), and for RGB
against the numpy statistics of the uint8 tensor export of the same window.
Every kernel test fills the output with 0xA5 and puts sentinels before, between
and after the items: the export writes every word of every record and nothing
else."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
import _crop
import _stats as S
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = _crop.cases()
CAP = 32                    # items per kernel launch (H264MI_ROIS_MAX_PER_LAUNCH)
# stats.hip cuts an item's units (two rows of 16 columns) into strips of STATS_STRIP_UNITS = 1024, one workgroup each:
# a whole 256 x 272 picture is 136 row pairs of 16 units, 2176 units, so it spans three strips
STRIP_UNITS = 1024
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128),      # test_warp.py's layouts
        "256x272_packed": (256, 272, 128)}
assert (256 // 16) * (272 // 2) > 2 * STRIP_UNITS
ORDER = [2, 0, 2]           # the picture list of every kernel test
REF_ORDER = [0, 1, 0]       # ... and its reference pictures, from a buffer of their own
SUB = (6, 2, 38, 26)        # a proper sub-window: neighbours just outside it exist and must not be counted
SETS = [("y", 0), ("yuv", 0), ("rgb", 0), ("rgb", 2)]
SENTINEL = 0xA5
FRONT = 64
OUT_PAD = 40                # sentinel bytes between two items


def case_stream(name):
    c = CASES[name]
    s = gen.generate(c["config"], c["seed"], **c["overrides"])
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """As in tests/test_tensor.py: the decoder instances here pool engines."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


def _mi():
    from broadway_amd import _lib
    return _lib.mi()


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 random pictures in the (width, cpitch) layout (read-only)."""
    rng = np.random.default_rng(29)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


_KEEP = {}


@functools.lru_cache(maxsize=None)
def _samples(key, w, h, cp, win, planes, colour):
    return S.plane_samples(_KEEP[key], w, h, cp, win, planes, colour)


def expect(pic, ref, w, h, cp, win, planes, colour, hist):
    """S.expect with the samples computed once per (picture, window, plane set, colour)."""
    for p in (pic, ref):
        if p is not None:
            _KEEP[id(p)] = p
    s = _samples(id(pic), w, h, cp, tuple(win), planes, colour)
    r = _samples(id(ref), w, h, cp, tuple(win), planes, colour) if ref is not None else [None] * len(s)
    return np.stack([S.record(a, b, hist) for a, b in zip(s, r)])


def make_desc(planes, colour=0, hist=False, window=(0, 0, 0, 0), reserved=0, flags=None):
    from broadway_amd import _lib
    d = _lib.StatsDesc()
    d.x, d.y, d.cw, d.ch = window
    d.planes = S.PLANE_IDS[planes] if isinstance(planes, str) else planes
    d.colour, d.reserved = colour, reserved
    d.flags = (1 if hist else 0) if flags is None else flags
    return d


def run_stats(pics, refs, w, h, cp, planes, colour=0, hist=False, window=(0, 0, 0, 0), boxes=None, order=ORDER,
              ref_order=REF_ORDER, in_skew=1, out_skew=0, stride=None, desc=None, null=()):
    """h264mi_stats_device_pitch over pictures `order` of `pics` (the input base
    in_skew bytes into its buffer) against pictures `ref_order` of `refs` (None:
    no reference; base 3 bytes into a buffer of its own); returns rc, the whole
    output buffer (FRONT + out_skew sentinel bytes, then items out_stride apart,
    then 64 sentinel bytes), the first item's offset, out_stride and an item's bytes."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    P, Lw = S.words(planes if isinstance(planes, str) else "y", hist)
    nbytes = P * Lw * 8
    nitems = len(boxes) if boxes is not None else len(order)
    out_stride = nbytes + OUT_PAD if stride is None else stride

    def upload(ps, skew):
        stride_in = ps[0].size + 5                  # (an odd distance: the pictures' alignments differ)
        host = np.zeros(skew + stride_in * len(ps) + 16, dtype=np.uint8)
        for k, p in enumerate(ps):
            host[skew + k * stride_in:skew + k * stride_in + p.size] = p
        return torch.from_numpy(host).to("cuda"), stride_in

    d_in, in_stride = upload(pics, in_skew)
    offs = (C.c_size_t * len(order))(*[k * in_stride for k in order])
    d_ref = roffs = None
    if refs is not None:
        d_ref, ref_stride = upload(refs, 3)
        roffs = (C.c_size_t * len(ref_order))(*[k * ref_stride for k in ref_order])
    first = FRONT + out_skew
    d_out = torch.full((first + max(out_stride, nbytes) * max(nitems, 1) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    if desc is None:
        desc = make_desc(planes, colour, hist, (0, 0, 0, 0) if boxes is not None else window)
    arr = None if boxes is None else (_lib.Roi * max(len(boxes), 1))(*[_lib.Roi(*b) for b in boxes])
    rc = L.h264mi_stats_device_pitch(None if "in" in null else d_in.data_ptr() + in_skew, None if "offs" in null else offs,
                                     None if d_ref is None or "ref" in null else d_ref.data_ptr() + 3,
                                     None if "roffs" in null else roffs, len(order), w, h, cp,
                                     None if "desc" in null else C.byref(desc), arr, len(boxes) if boxes is not None else 0,
                                     None if "out" in null else d_out.data_ptr() + first, out_stride,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), first, out_stride, nbytes


def same(got, want):
    """Exact equality; what differs is printed before the assertion fails."""
    if got.shape == want.shape and np.array_equal(got, want):
        return True
    if got.shape != want.shape:
        print(f"shapes differ: {got.shape} {want.shape}")
    else:
        bad = np.flatnonzero(got != want)
        print(f"{bad.size} of {want.size} words differ, first at {bad[:8].tolist()}: got {got.ravel()[bad[:8]].tolist()} "
              f"want {want.ravel()[bad[:8]].tolist()}")
    return False


def check_items(out, first, stride, nbytes, want):
    """Every item equals `want` (items, P, L) and no byte outside the items changed."""
    assert (out[:first] == SENTINEL).all()
    for r in range(want.shape[0]):
        o = first + r * stride
        got = out[o:o + nbytes].view(np.int64).reshape(want.shape[1:])
        assert same(got.ravel(), want[r].ravel()), r
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), r
    assert (out[first + want.shape[0] * stride:] == SENTINEL).all()


def window_items(pics, refs, w, h, cp, win, planes, colour, hist, order=ORDER, ref_order=REF_ORDER):
    return np.stack([expect(pics[k], refs[ref_order[i]] if refs is not None else None, w, h, cp, win, planes, colour, hist)
                     for i, k in enumerate(order)])


@pytest.mark.gpu
@pytest.mark.parametrize("ref", [False, True], ids=["alone", "ref"])
@pytest.mark.parametrize("hist", [False, True], ids=["moments", "hist"])
@pytest.mark.parametrize("planes,colour", SETS)
def test_device_sweep_vs_oracle(pictures, planes, colour, hist, ref):
    """Every layout, the whole picture and a proper sub-window, the picture list
    [2, 0, 2] against references [0, 1, 0], the input base on an odd byte (the
    v_alignbyte loads) and on a multiple of 16 (16 bytes per lane where the
    rows allow), into a 0xA5-filled buffer with sentinels all round."""
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        pics = pictures[pic]
        refs = pics if ref else None
        for win in ((0, 0, w, h), SUB):
            want = window_items(pics, refs, w, h, cp, win, planes, colour, hist)
            for in_skew in (1, 0):
                rc, out, first, stride, nbytes = run_stats(pics, refs, w, h, cp, planes, colour, hist, win, in_skew=in_skew)
                assert rc == 0, (pic, win, in_skew)
                check_items(out, first, stride, nbytes, want)


def special_pictures(w, h, cp, rng):
    n = w * h + cp * h
    half = rng.integers(0, 256, n, dtype=np.uint8)
    half[w * (h // 2):w * h] = 77                       # the lower half of the luma plane flat: waves of one value
    return {"flat255": np.full(n, 255, np.uint8), "flat0": np.zeros(n, np.uint8), "half_flat": half,
            "random": rng.integers(0, 256, n, dtype=np.uint8)}


@pytest.mark.gpu
@pytest.mark.parametrize("planes,colour", SETS)
def test_special_pictures(planes, colour):
    """Flat 255 and flat 0 (min and max start right, one bin holds everything,
    and every lane of a wave hits it), a picture whose lower half is flat (waves
    that fold their adds next to waves that do not), a picture equal to its
    reference (sad == ssd == 0) and 255 against a reference of 0 -- with the
    histogram, over one strip and over three."""
    rng = np.random.default_rng(31)
    for pic in ("48x32_pitch128", "256x272_packed"):
        w, h, cp = PICS[pic]
        sp = special_pictures(w, h, cp, rng)
        pairs = [("flat255", None), ("flat0", None), ("half_flat", None), ("random", "random"), ("flat255", "flat0"),
                 ("flat0", "flat255"), ("half_flat", "flat255")]
        for a, b in pairs:
            for win in ((0, 0, w, h), SUB):
                want = np.stack([S.expect(sp[a], w, h, cp, win, planes, colour, True, sp[b] if b else None)])
                rc, out, first, stride, nbytes = run_stats([sp[a]], [sp[b]] if b else None, w, h, cp, planes, colour, True, win,
                                                           order=[0], ref_order=[0], in_skew=0 if b else 1)
                assert rc == 0, (pic, a, b, win)
                check_items(out, first, stride, nbytes, want)
                rec = out[first:first + nbytes].view(np.int64).reshape(want.shape[1:])
                if b == a:
                    assert (rec[:, 5:7] == 0).all()
                if a == "flat255" and planes != "rgb":
                    assert (rec[:, 3] == 255).all() and (rec[:, 4] == 255).all() and (rec[:, 8 + 255] == rec[:, 0]).all()
                if (a, b) == ("flat255", "flat0") and planes != "rgb":
                    assert (rec[:, 5] == 255 * rec[:, 0]).all() and (rec[:, 6] == 65025 * rec[:, 0]).all()


def box_list(w, h, rng, n=33):
    """n boxes (k, x, y, cw, ch) over three pictures: a 2 x 2 box, one with x = 2
    mod 4, one touching the right and bottom edges, two overlapping ones, the
    whole picture, then random even boxes."""
    boxes = [(0, 4, 6, 2, 2), (1, 6, 2, 38, 26), (2, w - 22, h - 10, 22, 10), (0, 8, 4, 24, 16), (0, 16, 8, 24, 16),
             (1, 0, 0, w, h)]
    while len(boxes) < n:
        x, y = 2 * int(rng.integers(0, w // 2)), 2 * int(rng.integers(0, h // 2))
        boxes.append((len(boxes) % 3, x, y, 2 * int(rng.integers(1, (w - x) // 2 + 1)), 2 * int(rng.integers(1, (h - y) // 2 + 1))))
    return boxes


@pytest.mark.gpu
@pytest.mark.parametrize("planes,colour,hist,ref", [("y", 0, False, False), ("yuv", 0, True, True), ("rgb", 2, True, True),
                                                    ("rgb", 0, False, False)])
def test_box_list_across_the_launch_boundary(pictures, planes, colour, hist, ref):
    """33 boxes over three pictures: two launches; box k of picture pic against
    the same box of reference picture pic."""
    rng = np.random.default_rng(37)
    for pic in ("256x32_packed", "256x272_packed"):
        w, h, cp = PICS[pic]
        pics = pictures[pic]
        refs = [pics[1], pics[2], pics[0]] if ref else None
        boxes = box_list(w, h, rng)
        assert len(boxes) == CAP + 1
        want = np.stack([expect(pics[k], refs[k] if ref else None, w, h, cp, b, planes, colour, hist) for k, *b in boxes])
        rc, out, first, stride, nbytes = run_stats(pics, refs, w, h, cp, planes, colour, hist, boxes=boxes, order=[0, 1, 2],
                                                   ref_order=[0, 1, 2])
        assert rc == 0, pic
        check_items(out, first, stride, nbytes, want)


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [0, 2])
def test_rgb_statistics_are_those_of_the_tensor_export(pictures, colour):
    """numpy statistics of h264mi_tensor_device_pitch's uint8 planar RGB of the same window of the same pictures."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    st = torch.cuda.current_stream().cuda_stream
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        pics = pictures[pic]
        for win in ((0, 0, w, h), SUB):
            x, y, cw, ch = win
            want = []
            for k, rk in zip(ORDER, REF_ORDER):
                planes = []
                for p in (pics[k], pics[rk]):
                    d_in = torch.from_numpy(np.array(p)).to("cuda")
                    t = _lib.TensorDesc()
                    t.x, t.y, t.cw, t.ch, t.mode, t.dtype = x, y, cw, ch, colour << 8, 0
                    rgb = torch.zeros((3, ch, cw), dtype=torch.uint8, device="cuda")
                    assert L.h264mi_tensor_device_pitch(d_in.data_ptr(), (C.c_size_t * 1)(0), 1, w, h, cp, C.byref(t),
                                                        rgb.data_ptr(), 3 * ch * cw, st) == 0
                    torch.cuda.synchronize()
                    planes.append(rgb.cpu().numpy())
                want.append(np.stack([S.record(planes[0][c], planes[1][c], True) for c in range(3)]))
            rc, out, first, stride, nbytes = run_stats(pics, pics, w, h, cp, "rgb", colour, True, win)
            assert rc == 0
            check_items(out, first, stride, nbytes, np.stack(want))


@pytest.mark.gpu
def test_refusals_launch_nothing(pictures):
    """A bad descriptor, a misaligned d_out, a short out_stride, a bad box and a
    half-named reference each give -1 and leave the output untouched."""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128"]
    good = [(0, 0, 0, w, h), (2, 6, 2, 38, 26)]

    def run(**kw):
        args = dict(planes="rgb", colour=1, hist=True, window=SUB)
        args.update(kw)
        refs = args.pop("refs", pics)
        return run_stats(pics, refs, w, h, cp, args.pop("planes"), **args)

    rc, out, first, stride, nbytes = run()
    assert rc == 0                                      # the arguments below are one step away
    check_items(out, first, stride, nbytes, window_items(pics, pics, w, h, cp, SUB, "rgb", 1, True))
    assert run(stride=nbytes)[0] == 0 and run(boxes=good)[0] == 0       # packed items, and a good list
    assert run(order=[1], ref_order=[1], stride=0)[0] == 0             # one item: any out_stride
    bad = {
        "planes_3": dict(desc=make_desc(3, 0, True, SUB)), "flag_2": dict(desc=make_desc("rgb", 0, window=SUB, flags=3)),
        "reserved": dict(desc=make_desc("rgb", 0, True, SUB, reserved=1)), "colour_4": dict(colour=4),
        "colour_stream": dict(colour=15), "colour_with_y": dict(planes="y", colour=1),
        "window_odd": dict(window=(5, 2, 38, 26)), "window_past_right": dict(window=(12, 2, 38, 26)),
        "window_empty": dict(window=(0, 0, 0, 0)), "out_misaligned": dict(out_skew=4), "stride_misaligned": dict(stride=nbytes + 4),
        "stride_short": dict(stride=nbytes - 8), "stride_zero": dict(stride=0),
        "box_bad_pic": dict(boxes=good + [(3, 0, 0, 2, 2)]), "box_odd": dict(boxes=good + [(0, 1, 0, 2, 2)]),
        "box_past_bottom": dict(boxes=[(0, 0, 8, 16, 26)] + good), "boxes_none": dict(boxes=[]),
        "boxes_with_window": dict(boxes=good, desc=make_desc("rgb", 1, True, SUB)),
        "ref_without_offsets": dict(null=("roffs",)), "offsets_without_ref": dict(null=("ref",)),
        "no_in": dict(null=("in",)), "no_offs": dict(null=("offs",)), "no_desc": dict(null=("desc",)), "no_out": dict(null=("out",)),
    }
    for name, kw in sorted(bad.items()):
        rc, out, *_ = run(**kw)
        assert rc == -1, name
        assert (out == SENTINEL).all(), name             # nothing was launched


@pytest.mark.gpu
def test_engine_to_stats_vs_the_slots_pictures():
    """Statistics of two slots, each against the other, on a caller's stream
    into out=, against the oracle on Engine.read()'s pictures; a decode into
    one of the named slots queued right behind the export does not change the
    result; boxes over the slots; stats_fields' views alias the result; a bad
    slot is a RuntimeError, a wrong out a ValueError."""
    import torch
    from broadway_amd.engine import Capture, Engine, stats_fields
    name = "crop_ltrb_6x4"          # the smallest case: 96 x 64
    cap = Capture(case_stream(name))
    w, h = cap.w_mbs * 16, cap.h_mbs * 16
    assert (w, h) == (96, 64)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    first = slots[:again].index(slots[again])
    other = next(k for k in range(again) if k != first)
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    held = [slots[first], slots[other]]
    pics = [eng.read(0, s).copy() for s in held]
    assert not np.array_equal(pics[0], pics[1])
    cp = w // 2                                         # (read() returns packed I420, whatever the slot's chroma pitch)
    assert pics[0].size == w * h * 3 // 2
    win = (6, 2, 86, 52)
    out = torch.full((2, 3, 264), -1, dtype=torch.int64, device="cuda")
    got = eng.to_stats([0, 0], held, planes="rgb", window=win, hist=True, ref=([0, 0], held[::-1]), colour="bt709", out=out,
                       stream=side)
    eng.decode([0], [cap.pictures[again]])              # overwrites held[0]: it waits for the export
    whole = eng.to_stats([0], [held[1]], planes="yuv")
    boxes = [(1, 6, 2, 38, 26), (0, 0, 0, 96, 64), (1, 94, 62, 2, 2)]
    boxed = eng.to_stats([0, 0], held, rois=boxes, hist=True, ref=([0, 0], [held[1], held[1]]))
    torch.cuda.synchronize()
    assert got is out and eng.errors() == 0
    want = np.stack([S.expect(pics[k], w, h, cp, win, "rgb", 2, True, pics[1 - k]) for k in range(2)])
    assert same(out.cpu().numpy().ravel(), want.ravel())
    assert tuple(whole.shape) == (1, 3, 8) and whole.dtype == torch.int64
    assert same(whole.cpu().numpy().ravel(), S.expect(pics[1], w, h, cp, (0, 0, w, h), "yuv").ravel())
    now = [eng.read(0, held[0]).copy(), pics[1]]        # (held[0] holds the later picture by now)
    assert tuple(boxed.shape) == (3, 1, 264)
    assert same(boxed.cpu().numpy().ravel(), S.expect_items(now, [pics[1], pics[1]], w, h, cp, boxes, "y", 0, True).ravel())
    f = stats_fields(out)
    assert f["ssd"].data_ptr() == out.data_ptr() + 6 * 8 and f["hist"].data_ptr() == out.data_ptr() + 8 * 8
    assert torch.equal(f["hist"].sum(-1), f["count"]) and torch.equal(f["sad"][0], f["sad"][1]) and (f["ssd"] > 0).all()
    with pytest.raises(ValueError):
        eng.to_stats([0, 0], held, out=torch.empty((2, 1, 264), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.to_stats([0, 0], held, out=torch.empty((2, 1, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        eng.to_stats([0, 0], [0, eng.nslots])           # the library refuses the slot
    with pytest.raises(RuntimeError):
        eng.to_stats([0, 0], held, ref=([0, 0], [0, eng.nslots]))
    eng.close()


def run_decoder(stream, opts, on_picture):
    """Decoder(opts) over the stream's NAL units; on_picture(dec, k, buf, w, h)
    runs inside onPictureDecoded.  Returns the number of pictures."""
    dec = Decoder(opts)
    count = [0]

    def cb(buf, w, h, infos):
        on_picture(dec, count[0], buf, w, h)
        count[0] += 1

    dec.onPictureDecoded = cb
    for nal in split_annexb(stream):
        dec.decode(nal)
    dec.close()
    return count[0]


def vui_stream(name):
    """A stream of tests/golden/colour.json: crop_ltrb_6x4's geometry with a VUI (tests/test_colour.py's)."""
    with open(os.path.join(HERE, "golden", "colour.json")) as f:
        g = json.load(f)
    c = g["cases"][name]
    s = gen.generate(g["config"], c["seed"], **dict(g["base_overrides"], **c["overrides"]))
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"crop": True}, {"tensor": {"size": (13, 11)}}, {}], ids=["crop", "tensor", "plain"])
def test_decoder_stats_in_the_callback(opts):
    """Inside onPictureDecoded, in every output mode: the whole delivered
    (crop) window, a window inside it and boxes, moved by the crop offset,
    against the oracle on the reference decoder's pictures; colour="stream"
    takes the set the VUI names (matrix 1, full range: "bt709-full") and
    reports it; consecutive histograms differ exactly where the pictures'
    histograms do."""
    import torch
    stream = vui_stream("m1_full")
    win = (6, 2, 86, 52)
    frames, errs, w, h, _ = O.decode(stream)
    assert errs == 0 and (w, h) == (96, 64)
    boxes = [(0, 0, 86, 52), (46, 20, 40, 32), (2, 2, 2, 2), (10, 4, 38, 26)]
    inner = (4, 2, 80, 48)
    got, colours = [], []

    def on_picture(dec, k, buf, pw, ph):
        got.append(dec.stats())
        got.append(dec.stats(boxes, planes="rgb", hist=True, colour="stream"))
        colours.append(dec.tensor_colour)
        got.append(dec.stats(planes="yuv", hist=True, window=inner))
        got.append(dec.stats(planes="rgb", colour="bt601-full"))

    n = run_decoder(stream, dict(opts), on_picture)
    torch.cuda.synchronize()
    assert n == len(frames) and n >= 3 and len(got) == 4 * n and set(colours) == {"bt709-full"}
    moved = lambda b: (b[0] + win[0], b[1] + win[1], b[2], b[3])            # noqa: E731
    hists = []
    for k in range(n):
        y, b, i, r = (t.cpu().numpy() for t in got[4 * k:4 * k + 4])
        assert y.shape == (1, 1, 8) and b.shape == (4, 3, 264) and i.shape == (1, 3, 264) and r.shape == (1, 3, 8)
        assert y.dtype == np.int64 and got[4 * k].is_cuda
        assert same(y.ravel(), S.expect(frames[k], w, h, w // 2, win, "y").ravel()), k
        want = np.stack([S.expect(frames[k], w, h, w // 2, moved(x), "rgb", 3, True) for x in boxes])
        assert same(b.ravel(), want.ravel()), k
        assert same(i.ravel(), S.expect(frames[k], w, h, w // 2, moved(inner), "yuv", 0, True).ravel()), k
        assert same(r.ravel(), S.expect(frames[k], w, h, w // 2, win, "rgb", 1).ravel()), k
        hists.append((i[0, :, 8:], S.expect(frames[k], w, h, w // 2, moved(inner), "yuv", 0, True)[:, 8:]))
    differ = [not np.array_equal(hists[k][1], hists[k + 1][1]) for k in range(n - 1)]
    assert any(differ)
    assert [not np.array_equal(hists[k][0], hists[k + 1][0]) for k in range(n - 1)] == differ


@pytest.mark.gpu
def test_decoder_stats_return_codes():
    """H264SwDecLastPictureStats: OK before any picture and after the next
    H264SwDecDecode, PARAM_ERR for a window or a box over the crop edge, pic =
    1, a count without boxes and a bad plane set, PIC_RDY on success;
    Decoder.stats raises RuntimeError where the call answers OK."""
    import torch
    from broadway_amd import _lib
    nals = split_annexb(case_stream("crop_ltrb_6x4"))     # two slices a picture: the NAL after a picture's last delivers nothing
    dec = Decoder()
    L = dec._L
    out = torch.full((4 * 3 * 264,), 7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(boxes=None, n=None, **kw):
        desc = make_desc(kw.pop("planes", "yuv"), hist=True, **kw)
        arr = None if boxes is None else (_lib.Roi * max(len(boxes), 1))(*[_lib.Roi(*b) for b in boxes])
        return L.H264SwDecLastPictureStats(dec._inst, C.byref(desc), arr, (len(boxes) if boxes is not None else 0) if n is None else n,
                                           out.data_ptr(), st)

    assert call() == _lib.H264SWDEC_OK                              # before the headers
    assert call(planes=3) == _lib.H264SWDEC_PARAM_ERR               # a bad descriptor even then
    with pytest.raises(RuntimeError):
        dec.stats()
    inside = []

    def cb(buf, w, h, infos):
        inside.append((call(), call(window=(4, 2, 82, 50)), call([(0, 4, 2, 82, 50), (0, 0, 0, 2, 2)]),
                       call(window=(4, 2, 84, 50)), call(window=(4, 2, 82, 52)), call(window=(1, 0, 4, 4)),
                       call([(0, 4, 2, 84, 50)]), call([(1, 0, 0, 2, 2)]), call([]), call(n=1), call(planes=3),
                       call(planes="yuv", colour=15)))

    dec.onPictureDecoded = cb
    delivered_at = []
    for k, nal in enumerate(nals):
        before = len(inside)
        dec.decode(nal)
        if len(inside) > before:
            delivered_at.append(k)
            assert call() == _lib.H264SWDEC_PIC_RDY                 # until the next decode
        elif delivered_at:
            assert call() == _lib.H264SWDEC_OK, k                   # after the next H264SwDecDecode
            with pytest.raises(RuntimeError):
                dec.stats()
    torch.cuda.synchronize()
    assert len(delivered_at) >= 2 and len(delivered_at) < len(nals) - 2
    P, Y = _lib.H264SWDEC_PARAM_ERR, _lib.H264SWDEC_PIC_RDY
    assert set(inside) == {(Y, Y, Y, P, P, P, P, P, P, P, P, P)}
    dec.close()
