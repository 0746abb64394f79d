"""The statistics export without a GPU: the numpy oracle of
tests/_stats.py against a brute-force loop and its own identities, the
descriptor builders' refusals, and the library's entry points."""
import ctypes as C

import numpy as np
import pytest

import _stats as S
from broadway_amd import _lib
from broadway_amd.engine import stats_desc, stats_fields

W, H, CP = 48, 32, 128
WIN = (6, 2, 6, 4)          # the 6 x 4 window of the brute-force check


@pytest.fixture(scope="module")
def pics():
    rng = np.random.default_rng(41)
    out = [rng.integers(0, 256, W * H + CP * H, dtype=np.uint8) for _ in range(2)]
    for p in out:
        p.setflags(write=False)
    return out


def brute(pic, ref, planes, colour):
    """The records of WIN by Python loops over single samples."""
    x, y, cw, ch = WIN
    Y = lambda p, r, c: int(p[r * W + c])                                           # noqa: E731
    U = lambda p, r, c: int(p[W * H + r * CP + c])                                  # noqa: E731
    V = lambda p, r, c: int(p[W * H + CP * (H // 2) + r * CP + c])                  # noqa: E731

    def rgb(p, r, c):
        yy, u, v = Y(p, r, c), U(p, r // 2, c // 2) - 128, V(p, r // 2, c // 2) - 128
        if colour == 0:
            ky, k0, crv, cgu, cgv, cbu = 1192, -1192 * 16, 1634, 400, 832, 2066
        else:
            ky, k0, crv, cgu, cgv, cbu = {2: (1192, 512 - 1192 * 16, 1836, 218, 546, 2163)}[colour]
        a0 = ky * yy + k0
        clamp = lambda t: min(max(t >> 10, 0), 255)                                 # noqa: E731
        return clamp(a0 + crv * v), clamp(a0 - cgu * u - cgv * v), clamp(a0 + cbu * u)

    def samples(p):
        if planes == "rgb":
            px = [rgb(p, r, c) for r in range(y, y + ch) for c in range(x, x + cw)]
            return [[q[k] for q in px] for k in range(3)]
        out = [[Y(p, r, c) for r in range(y, y + ch) for c in range(x, x + cw)]]
        if planes == "yuv":
            half = [(r, c) for r in range(y // 2, (y + ch) // 2) for c in range(x // 2, (x + cw) // 2)]
            out += [[U(p, r, c) for r, c in half], [V(p, r, c) for r, c in half]]
        return out

    recs = []
    for s, r in zip(samples(pic), samples(ref)):
        rec = [len(s), sum(s), sum(v * v for v in s), min(s), max(s), sum(abs(a - b) for a, b in zip(s, r)),
               sum((a - b) ** 2 for a, b in zip(s, r)), 0]
        rec += [sum(1 for v in s if v == b) for b in range(256)]
        recs.append(rec)
    return np.array(recs, dtype=np.int64)


@pytest.mark.parametrize("planes,colour", [("y", 0), ("yuv", 0), ("rgb", 0), ("rgb", 2)])
def test_oracle_against_brute_force(pics, planes, colour):
    got = S.expect(pics[0], W, H, CP, WIN, planes, colour, True, pics[1])
    assert got.shape == S.words(planes, True) and got.dtype == np.int64
    assert np.array_equal(got, brute(pics[0], pics[1], planes, colour))
    # without the histogram: the first 8 words; without a reference: sad = ssd = 0
    assert np.array_equal(S.expect(pics[0], W, H, CP, WIN, planes, colour, False, pics[1]), got[:, :8])
    alone = S.expect(pics[0], W, H, CP, WIN, planes, colour, True)
    assert (alone[:, 5:8] == 0).all() and np.array_equal(np.delete(alone, [5, 6], axis=1), np.delete(got, [5, 6], axis=1))


@pytest.mark.parametrize("planes", sorted(S.PLANES))
def test_oracle_identities(pics, planes):
    """hist.sum() == count, sum v hist[v] == sum, sum v^2 hist[v] == sumsq, min
    and max are the histogram's ends, and ssd == sumsq_a + sumsq_b - 2 sum ab."""
    win = (6, 2, 38, 26)
    a = S.expect(pics[0], W, H, CP, win, planes, 0, True, pics[1])
    b = S.expect(pics[1], W, H, CP, win, planes, 0, True, pics[0])
    v = np.arange(256, dtype=np.int64)
    for p in range(S.PLANES[planes]):
        hist = a[p, 8:]
        assert hist.sum() == a[p, 0] and (v * hist).sum() == a[p, 1] and (v * v * hist).sum() == a[p, 2]
        assert np.flatnonzero(hist)[0] == a[p, 3] and np.flatnonzero(hist)[-1] == a[p, 4]
        sa, sb = S.plane_samples(pics[0], W, H, CP, win, planes)[p], S.plane_samples(pics[1], W, H, CP, win, planes)[p]
        ab = (sa.astype(np.int64) * sb.astype(np.int64)).sum()
        assert a[p, 6] == a[p, 2] + b[p, 2] - 2 * ab
        assert a[p, 5] == b[p, 5] and a[p, 6] == b[p, 6] and a[p, 7] == 0
    count = 38 * 26
    assert a[0, 0] == count and (planes != "yuv" or (a[1, 0] == count // 4 and a[2, 0] == count // 4))


def test_stats_desc_builds_the_descriptor_and_the_array():
    d, arr, P, L = stats_desc("rgb", (6, 2, 38, 26), None, True, "bt709", 3, 48, 32)
    assert (d.x, d.y, d.cw, d.ch, d.planes, d.colour, d.flags, d.reserved) == (6, 2, 38, 26, 2, 2, 1, 0)
    assert arr is None and (P, L) == (3, 264)
    d, arr, P, L = stats_desc("y", None, [(2, 0, 0, 48, 32), (0, 46, 30, 2, 2)], False, None, 3, 48, 32)
    assert (d.x, d.y, d.cw, d.ch, d.planes, d.colour, d.flags) == (0, 0, 0, 0, 0, 0, 0) and (P, L) == (1, 8)
    assert [(b.pic, b.x, b.y, b.cw, b.ch) for b in arr] == [(2, 0, 0, 48, 32), (0, 46, 30, 2, 2)]
    d, arr, P, L = stats_desc("yuv", hist=True)                     # the Decoder's "everything"
    assert (d.cw, d.ch, d.planes, d.flags) == (0, 0, 1, 1) and arr is None and (P, L) == (3, 264)
    assert stats_desc("rgb", colour="stream", stream_ok=True)[0].colour == 15


@pytest.mark.parametrize("kw,why", [
    (dict(window=(1, 2, 38, 26)), "odd x"),
    (dict(window=(6, 2, 37, 26)), "odd cw"),
    (dict(window=(6, 2, 38, 25)), "odd ch"),
    (dict(window=(6, 2, 44, 26)), "past the right edge"),
    (dict(window=(6, 8, 38, 26)), "past the bottom edge"),
    (dict(window=(-2, 2, 38, 26)), "negative x"),
    (dict(window=(0, 0, 0, 0)), "an empty window"),
    (dict(window=(6, 2, 38)), "three numbers"),
    (dict(window=(6.5, 2, 38, 26)), "not integers"),
    (dict(window=(6, 2, 38, 26), rois=[(0, 0, 0, 16, 16)]), "boxes with a window"),
    (dict(rois=[]), "no box"),
    (dict(rois=[(3, 0, 0, 16, 16)]), "picture 3 of 3"),
    (dict(rois=[(0, 0, 0, 16, 16), (-1, 0, 0, 16, 16)]), "picture -1"),
    (dict(rois=[(0, 0, 0, 16, 16), (0, 1, 0, 16, 16)]), "a box with odd x"),
    (dict(rois=[(0, 34, 0, 16, 16)]), "a box past the right edge"),
    (dict(rois=[(0, 0, 16, 16)]), "a box of four numbers"),
    (dict(rois=7), "not a list"),
    (dict(planes="uv"), "unknown planes"),
    (dict(planes=2), "planes by number"),
    (dict(planes="y", colour="bt709"), "colour with Y"),
    (dict(planes="yuv", colour="reference"), "colour with YUV"),
    (dict(planes="rgb", colour="bt2020"), "unknown colour"),
    (dict(planes="rgb", colour="stream"), "stream at the engine"),
])
def test_stats_desc_rejects(kw, why):
    kw = dict(kw)
    kw.setdefault("planes", "rgb" if "colour" in kw else "y")
    with pytest.raises(ValueError):
        stats_desc(npics=3, width=48, height=32, **kw)


def test_engine_to_stats_refuses_before_the_library_is_called():
    """Engine.to_stats on an object that has no library handle: the ValueError comes first."""
    from broadway_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 3, 2
    eng._h = None                                               # (close() and __del__ find nothing to destroy)
    pics = ([0, 0, 0], [0, 1, 2])
    for kw in (dict(window=(0, 0, 50, 32)), dict(window=(0, 0, 48, 32), rois=[(0, 0, 0, 16, 16)]),
               dict(rois=[(3, 0, 0, 16, 16)]), dict(planes="y", colour="bt709"), dict(planes="hsv"),
               dict(ref=([0, 0], [1, 2])), dict(ref=([0, 0, 0], [1, 2])), dict(ref=[0, 1, 2]), dict(ref=5),
               dict(planes="rgb", colour="stream")):
        with pytest.raises(ValueError):
            eng.to_stats(*pics, **kw)
    with pytest.raises(ValueError):
        eng.to_stats([0, 0], [0], planes="y")


def test_stats_fields_are_views():
    import torch
    t = torch.arange(2 * 3 * 264, dtype=torch.int64).reshape(2, 3, 264)
    f = stats_fields(t)
    assert sorted(f) == sorted(S.FIELDS + ("hist",))
    for i, name in enumerate(S.FIELDS):
        assert f[name].shape == (2, 3) and f[name].data_ptr() == t.data_ptr() + 8 * i and torch.equal(f[name], t[..., i])
    assert f["hist"].shape == (2, 3, 256) and f["hist"].data_ptr() == t.data_ptr() + 64
    assert "hist" not in stats_fields(t[..., :8])
    with pytest.raises(ValueError):
        stats_fields(t[..., :9])


def test_library_exports_the_stats_entry_points():
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_stats_device_pitch", 14), ("h264mi_engine_export_stats", 12),
                        ("H264SwDecLastPictureStats", 6), ("h264mi_stats_item_words", 1)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.h264mi_engine_abi() == 6
    # the pure function, for all six (planes, hist) pairs and the refusals
    for planes, P in ((0, 1), (1, 3), (2, 3)):
        for flags, Lw in ((0, 8), (1, 264)):
            d = _lib.StatsDesc(planes=planes, flags=flags)
            assert L.h264mi_stats_item_words(C.byref(d)) == P * Lw
    assert L.h264mi_stats_item_words(C.byref(_lib.StatsDesc(planes=3))) == 0
    assert L.h264mi_stats_item_words(C.byref(_lib.StatsDesc(flags=2))) == 0
    assert L.h264mi_stats_item_words(None) == 0
