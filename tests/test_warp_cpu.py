"""The affine-warped export without a GPU: the properties of the
oracle itself (tests/_warp.py) -- the identity, whole-sample maps, the
half-sample shift, and a derived bound against float bilinear --, the two
coefficient helpers of broadway_amd.engine, the ValueError cases of
Engine.to_tensor(warps=) and Decoder.warps, and the library's symbols."""
import ctypes as C

import numpy as np
import pytest

import _warp as W
from broadway_amd import _lib
from broadway_amd.decoder import warps_args
from broadway_amd.engine import rotated_box_warp, warp_q16, warps_desc

Q = 65536


@pytest.fixture(scope="module")
def planes():
    """(3, 26, 38) random samples, read-only."""
    c = np.random.default_rng(41).integers(0, 256, (3, 26, 38), dtype=np.uint8)
    c.setflags(write=False)
    return c


def test_identity_is_the_unwarped_tensor(planes):
    """The identity at (ch, cw): the samples themselves (fx = fy = 0, no border
    tap has weight) under either border and any pad -- so the elements are
    T.samples + T.convert's."""
    ch, cw = planes.shape[1:]
    for border in (W.CONSTANT, W.REPLICATE):
        assert np.array_equal(W.warp_planes(planes, W.IDENTITY, (ch, cw), border, (114, 7, 250)), planes)
    import _tensor as T
    scale, bias = T.CONSTS["imagenet"]
    assert np.array_equal(W.elements(W.warp_planes(planes, W.IDENTITY, (ch, cw)), "float16", "imagenet"),
                          T.convert(planes, "float16", scale, bias))
    hwc = W.elements(planes, "float16", "imagenet", hwc=True).view(np.float16).reshape(ch, cw, 3)
    assert np.array_equal(hwc.transpose(2, 0, 1).reshape(-1).view(np.uint8), T.convert(planes, "float16", scale, bias))


def test_whole_sample_maps_copy_samples(planes):
    ch, cw = planes.shape[1:]
    pad = (114, 7, 250)
    # a shift by (+3, -2): output (i, j) = sample (i - 2, j + 3), pad where that is outside
    got = W.warp_planes(planes, (Q, 0, 3 * Q, 0, Q, -2 * Q), (ch, cw), W.CONSTANT, pad)
    want = np.empty_like(planes)
    want[:] = np.asarray(pad, dtype=np.uint8).reshape(3, 1, 1)
    want[:, 2:, :cw - 3] = planes[:, :ch - 2, 3:]
    assert np.array_equal(got, want)
    # the same with the edge repeated
    got = W.warp_planes(planes, (Q, 0, 3 * Q, 0, Q, -2 * Q), (ch, cw), W.REPLICATE)
    want = planes[:, np.clip(np.arange(ch) - 2, 0, ch - 1)][:, :, np.clip(np.arange(cw) + 3, 0, cw - 1)]
    assert np.array_equal(got, want)
    # flips (negative coefficients: floor shifts)
    assert np.array_equal(W.warp_planes(planes, (-Q, 0, (cw - 1) * Q, 0, Q, 0), (ch, cw)), planes[:, :, ::-1])
    assert np.array_equal(W.warp_planes(planes, (Q, 0, 0, 0, -Q, (ch - 1) * Q), (ch, cw)), planes[:, ::-1])
    # the four quarter turns: k counter-clockwise turns are np.rot90(k)
    assert np.array_equal(W.warp_planes(planes, W.IDENTITY, (ch, cw)), np.rot90(planes, 0, (1, 2)))
    assert np.array_equal(W.warp_planes(planes, (0, -Q, (cw - 1) * Q, Q, 0, 0), (cw, ch)), np.rot90(planes, 1, (1, 2)))
    assert np.array_equal(W.warp_planes(planes, (-Q, 0, (cw - 1) * Q, 0, -Q, (ch - 1) * Q), (ch, cw)),
                          np.rot90(planes, 2, (1, 2)))
    assert np.array_equal(W.warp_planes(planes, (0, Q, 0, -Q, 0, (ch - 1) * Q), (cw, ch)), np.rot90(planes, 3, (1, 2)))


def test_half_sample_shift_is_the_rounded_mean(planes):
    ch, cw = planes.shape[1:]
    a = planes.astype(np.int64)
    got = W.warp_planes(planes, (Q, 0, Q // 2, 0, Q, 0), (ch, cw - 1))
    assert np.array_equal(got, (a[:, :, :-1] + a[:, :, 1:] + 1) >> 1)
    got = W.warp_planes(planes, (Q, 0, 0, 0, Q, Q // 2), (ch - 1, cw))
    assert np.array_equal(got, (a[:, :-1] + a[:, 1:] + 1) >> 1)


def test_against_float_bilinear(planes):
    """|v - float64 bilinear of the same four taps at the exact position| <=
    1.5: the position is rounded to 1/256 sample per axis (error <= 2^-9), each
    axis' interpolant changes by at most 255 per sample (<= 255 * 2^-9 < 0.5 an
    axis), and the final rounding adds 0.5.  A derived bound, not a measured one."""
    ch, cw = planes.shape[1:]
    rng = np.random.default_rng(43)
    worst = 0.0
    for _ in range(20):
        th = rng.uniform(-np.pi, np.pi)
        sc = rng.uniform(0.4, 2.5)
        m = warp_q16([[sc * np.cos(th), sc * np.sin(th), rng.uniform(-4, cw)],
                      [-sc * np.sin(th), sc * np.cos(th), rng.uniform(-4, ch)]], forward=False)
        oh, ow = 17, 23
        got = W.warp_planes(planes, m, (oh, ow), W.REPLICATE).astype(np.float64)
        i, j = np.mgrid[0:oh, 0:ow]
        x = (m[0] * j + m[1] * i + m[2]) / 65536.0
        y = (m[3] * j + m[4] * i + m[5]) / 65536.0
        # the integer taps (the float position may sit a hair on the other side of a sample), weights from the float position
        x0 = ((m[0] * j + m[1] * i + m[2] + 128) >> 16).astype(np.int64)
        y0 = ((m[3] * j + m[4] * i + m[5] + 128) >> 16).astype(np.int64)
        fx, fy = x - x0, y - y0
        s = lambda dy, dx: planes[:, np.clip(y0 + dy, 0, ch - 1), np.clip(x0 + dx, 0, cw - 1)].astype(np.float64)  # noqa: E731
        want = (1 - fx) * (1 - fy) * s(0, 0) + fx * (1 - fy) * s(0, 1) + (1 - fx) * fy * s(1, 0) + fx * fy * s(1, 1)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"max |integer - float64 bilinear| = {worst:.4f}")
    assert worst <= 1.5


def test_rotated_box_warp_exact_cases():
    # angle 0, the box the window, size (ch, cw): the identity, exactly
    assert rotated_box_warp(19, 13, 38, 26, 0, (26, 38)) == W.IDENTITY
    # power-of-two scales: a 2 : 1 shrink and a 1 : 2 enlargement about the centre
    assert rotated_box_warp(19, 13, 38, 26, 0, (13, 19)) == (2 * Q, 0, Q // 2, 0, 2 * Q, Q // 2)
    assert rotated_box_warp(19, 13, 38, 26, 0, (52, 76)) == (Q // 2, 0, -Q // 4, 0, Q // 2, -Q // 4)
    # 180 degrees: both axes flipped
    assert rotated_box_warp(19, 13, 38, 26, 180, (26, 38)) == (-Q, 0, 37 * Q, 0, -Q, 25 * Q)
    # 90 degrees counter-clockwise of a square box: x = cx - 0.5 + (i + 0.5 - 13), y = cy - 0.5 - (j + 0.5 - 13)
    assert rotated_box_warp(19, 13, 26, 26, 90, (26, 26)) == (0, Q, 6 * Q, -Q, 0, 25 * Q)
    assert rotated_box_warp(19, 13, 26, 26, -270, (26, 26)) == (0, Q, 6 * Q, -Q, 0, 25 * Q)
    assert rotated_box_warp(19, 13, 26, 26, 270, (26, 26)) == (0, -Q, 31 * Q, Q, 0, 0)
    assert all(isinstance(v, int) for v in rotated_box_warp(19.5, 13.25, 30, 20, 30, (112, 112)))


def test_rotated_box_turned_upright_is_the_rotation(planes):
    """A 90-degree box over the whole (square part of the) window copies
    samples: the box's top edge is the window's column that a counter-clockwise
    quarter turn brings to the top."""
    sq = planes[:, :, :26]
    m = rotated_box_warp(13, 13, 26, 26, 90, (26, 26))
    assert np.array_equal(W.warp_planes(sq, m, (26, 26)), np.rot90(sq, 3, (1, 2)))
    m = rotated_box_warp(13, 13, 26, 26, 270, (26, 26))
    assert np.array_equal(W.warp_planes(sq, m, (26, 26)), np.rot90(sq, 1, (1, 2)))


def test_warp_q16_forward_and_inverse_agree():
    # forward: x' = 2 x + 3, y' = 4 y - 8 (dst from src); by hand src = ((x' - 3) / 2, (y' + 8) / 4)
    fwd = [[2.0, 0.0, 3.0], [0.0, 4.0, -8.0]]
    inv = [[0.5, 0.0, -1.5], [0.0, 0.25, 2.0]]
    assert warp_q16(fwd) == warp_q16(inv, forward=False) == (Q // 2, 0, -3 * Q // 2, 0, Q // 4, 2 * Q)
    # a rotation by 90 degrees with a translation, inverted by hand: x' = -y + 5, y' = x + 1  ->  x = y' - 1, y = 5 - x'
    assert warp_q16([[0, -1, 5], [1, 0, 1]]) == warp_q16([[0, 1, -1], [-1, 0, 5]], forward=False) == (0, Q, -Q, -Q, 0, 5 * Q)
    assert warp_q16([[1, 0, 0], [0, 1, 0]]) == W.IDENTITY
    # rounding: floor(v * 65536 + 0.5)
    assert warp_q16([[1, 0, 0.5 / Q], [0, 1, -0.5 / Q]], forward=False) == (Q, 0, 1, 0, Q, 0)


def test_helpers_refuse_what_leaves_int32():
    with pytest.raises(ValueError):
        warp_q16([[32768.0, 0, 0], [0, 1, 0]], forward=False)           # 2^31
    assert warp_q16([[-32768.0, 0, 0], [0, 1, 0]], forward=False)[0] == -2 ** 31
    with pytest.raises(ValueError):
        warp_q16([[1, 0, 0], [0, 1, 40000.0]], forward=False)
    with pytest.raises(ValueError):
        warp_q16([[1e-6, 0, 0], [0, 1, 0]])                             # the inverse's scale is 10^6
    with pytest.raises(ValueError):
        warp_q16([[1, 2, 0], [2, 4, 0]])                                # singular
    with pytest.raises(ValueError):
        warp_q16([[1, 0, float("nan")], [0, 1, 0]], forward=False)
    with pytest.raises(ValueError):
        warp_q16([[1, 0], [0, 1]])
    with pytest.raises(ValueError):
        rotated_box_warp(0, 0, 1e6, 1e6, 45, (1, 1))
    with pytest.raises(ValueError):
        rotated_box_warp(0, 0, 10, 10, 0, (0, 4))


GOOD = [(0, W.IDENTITY), (2, (0, 0, -2 ** 31, 0, 0, 2 ** 31 - 1)), (1, rotated_box_warp(40, 30, 30, 20, 30, (7, 5)))]


def test_warps_desc_builds_the_descriptor_and_the_array():
    import torch
    d, arr, planes, dtype = warps_desc(GOOD, (7, 5), 3, (6, 2, 38, 26), 96, 64, mode="gray", dtype=torch.uint8,
                                       border="replicate", layout="nhwc")
    assert isinstance(d, _lib.TensorWarpDesc) and (d.oh, d.ow, d.filter, d.border, d.layout) == (7, 5, 0, 1, 1)
    assert (d.t.x, d.t.y, d.t.cw, d.t.ch) == (6, 2, 38, 26) and list(d.pad) == [0, 0, 0, 0]
    assert planes == 1 and dtype == torch.uint8 and len(arr) == 3
    assert [(w.pic, tuple(w.m)) for w in arr] == [(k, tuple(m)) for k, m in GOOD]
    d, _, planes, dtype = warps_desc(GOOD, (7, 5), 3, (0, 0, 96, 64), 96, 64, colour="bt709-full", pad=(114, 7, 250))
    assert planes == 3 and dtype == torch.float16 and d.t.mode == 3 << 8 and list(d.pad) == [114, 7, 250, 0]
    assert (d.border, d.layout) == (0, 0)
    d, *_ = warps_desc(GOOD, (7, 5), 3, (0, 0, 96, 64), 96, 64, pad=9)
    assert list(d.pad) == [9, 9, 9, 0]


@pytest.mark.parametrize("warps,size,kw,why", [
    (GOOD, None, {}, "warps without size"),
    ([], (8, 8), {}, "an empty list"),
    ([(3, W.IDENTITY)], (8, 8), {}, "k == npics"),
    ([(-1, W.IDENTITY)], (8, 8), {}, "k == -1"),
    ([(0, W.IDENTITY[:5])], (8, 8), {}, "five coefficients"),
    ([(0, (65536.5, 0, 0, 0, 65536, 0))], (8, 8), {}, "a fraction"),
    ([(0, (2 ** 31, 0, 0, 0, 65536, 0))], (8, 8), {}, "beyond int32"),
    ([(0, (0, 0, 0, 0, 0, -2 ** 31 - 1))], (8, 8), {}, "below int32"),
    ([W.IDENTITY], (8, 8), {}, "no picture index"),
    (GOOD, (0, 8), {}, "size 0"),
    (GOOD, (8, 16385), {}, "size beyond 16384"),
    (GOOD, (8, 8), {"border": "reflect"}, "an unknown border"),
    (GOOD, (8, 8), {"border": "replicate", "pad": 0}, "pad with replicate"),
    (GOOD, (8, 8), {"pad": 256}, "pad beyond a sample"),
    (GOOD, (8, 8), {"pad": (1, 2)}, "two pad samples for three planes"),
    (GOOD, (8, 8), {"layout": "hwc"}, "an unknown layout"),
    (GOOD, (8, 8), {"window": (1, 0, 16, 16)}, "an odd window"),
    (GOOD, (8, 8), {"window": (0, 0, 98, 64)}, "a window wider than the picture"),
    (GOOD, (8, 8), {"window": (0, 2, 96, 64)}, "a window over the bottom edge"),
    (GOOD, (8, 8), {"window": (0, 0, 0, 0)}, "an empty window"),
    (GOOD, (8, 8), {"colour": "stream"}, "an engine knows no stream"),
    (GOOD, (8, 8), {"mode": "gray", "colour": "bt709"}, "a colour set on luma"),
])
def test_warps_desc_rejects(warps, size, kw, why):
    kw = dict(kw)
    window = kw.pop("window", (0, 0, 96, 64))
    with pytest.raises(ValueError):
        warps_desc(warps, size, 3, window, 96, 64, **kw)


def test_engine_to_tensor_refuses_before_the_library_is_called():
    """Engine.to_tensor(warps=) on an object that has no library handle: the
    ValueError comes first."""
    from broadway_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.w_mbs, eng.h_mbs = 6, 4
    eng._h = None                                               # (close() and __del__ find nothing to destroy)
    pics = ([0, 0, 0], [0, 1, 2])
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=GOOD)                                            # no size
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=GOOD, size=(8, 8), rois=[(0, 0, 0, 16, 16)])
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=GOOD, size=(8, 8), fit="letterbox")
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, size=(8, 8), border="replicate")                       # border without warps
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, rois=[(0, 0, 0, 16, 16)], size=(8, 8), border="constant")
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=[], size=(8, 8))
    with pytest.raises(ValueError):
        eng.to_tensor([0, 0], [0, 1], warps=GOOD, size=(8, 8))                      # k = 2 of two pictures
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=GOOD, size=(8, 8), window=(0, 0, 98, 64))
    with pytest.raises(ValueError):
        eng.to_tensor(*pics, warps=GOOD, size=(8, 8), border="wrap")


def test_decoder_warps_argument_validation():
    """Decoder.warps' arguments (decoder.warps_args): matrices of picture 0;
    window None is the delivered window (cw = 0 in the descriptor)."""
    import torch
    d, arr, planes, dtype = warps_args([W.IDENTITY, (0, Q, 0, -Q, 0, 51 * Q)], (5, 7), None, 86, 52, dtype=torch.float32)
    assert [(w.pic, tuple(w.m)) for w in arr] == [(0, W.IDENTITY), (0, (0, Q, 0, -Q, 0, 51 * Q))]
    assert (d.oh, d.ow, planes, dtype) == (5, 7, 3, torch.float32)
    assert (d.t.x, d.t.y, d.t.cw, d.t.ch) == (0, 0, 0, 0)
    d, *_ = warps_args([W.IDENTITY], (4, 4), (2, 2, 84, 50), 86, 52, colour="stream", unspecified="bt709")
    assert d.t.mode == 15 << 8 | 1 << 12 and (d.t.x, d.t.y, d.t.cw, d.t.ch) == (2, 2, 84, 50)
    for mats, size, window in (([], (4, 4), None), ([W.IDENTITY], None, None), ([W.IDENTITY], (0, 4), None), (7, (4, 4), None),
                               ([W.IDENTITY[:4]], (4, 4), None), ([W.IDENTITY], (4, 4), (0, 0, 88, 52)),
                               ([W.IDENTITY], (4, 4), (0, 0, 86, 54)), ([W.IDENTITY], (4, 4), (1, 0, 4, 4))):
        with pytest.raises(ValueError):
            warps_args(mats, size, window, 86, 52)
    with pytest.raises(ValueError):
        warps_args([W.IDENTITY], (4, 4), None, 86, 52, mode="yuv")
    # before the headers (no picture size yet) only the picture-independent rules are checked
    warps_args([W.IDENTITY], (112, 112), (0, 0, 640, 480), 0, 0)
    with pytest.raises(ValueError):
        warps_args([W.IDENTITY], (112, 112), (0, 0, 641, 480), 0, 0)


def test_library_exports_the_warp_entry_points():
    lib = C.CDLL(_lib.LIB_DIR + "/libh264mi.so")
    L = _lib.mi()
    for name, nargs in (("h264mi_tensor_warps_device_pitch", 12), ("h264mi_engine_export_tensor_warps", 10),
                        ("H264SwDecLastPictureTensorWarps", 6)):
        assert hasattr(lib, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    # typedef struct { int pic; int m[6]; } h264mi_warp; and the descriptor of tests/test_warp_desc.py
    assert C.sizeof(_lib.Warp) == 28 and C.sizeof(_lib.TensorWarpDesc) == 72
    assert [f[0] for f in _lib.Warp._fields_] == ["pic", "m"]
    assert [f[0] for f in _lib.TensorWarpDesc._fields_] == ["t", "ow", "oh", "filter", "border", "pad", "layout"]
    assert _lib.WARPS_MAX_PER_LAUNCH == 32 and _lib.WARP_BORDERS == {"constant": 0, "replicate": 1}
