"""The bicubic filter of the resized tensor exports on the GPU (resize.hip,
DESIGN 3.5o; H264MI_RESIZE_BICUBIC): h264mi_tensor_resize_device_pitch, the
table forms (boxes, letterbox, interleaved), Engine.to_tensor(filter=),
Decoder's ``tensor: {"filter": ...}`` and Decoder.rois(filter=).

The oracle (tests/_bicubic.py) restates the arithmetic in Python integers on top
of tests/_tensor.py; the letterbox and the interleaved layout are composed with
tests/_letterbox.py and tests/_layout.py.  Every comparison is exact equality
of bytes, with sentinels around the output."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import _bicubic as B
import _crop
import _layout as LY
import _letterbox as LB
import _tensor as T
from broadway_amd.decoder import Decoder, split_annexb
from test_resize import (CAP, CASES, FRONT, RESIZES, SENTINEL, case_stream, consts_of, make_desc, run_resize, same,
                         sps_window, tensor_bytes)

BICUBIC = B.FILTER


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


# name -> (width, height, chroma pitch)
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128), "32x128": (32, 128, 16)}
# (window, (oh, ow)) by picture, on top of test_resize's RESIZES where the picture holds their windows:
# 16 : 1 on both axes, 64 horizontal taps at the interior columns and two source chunks per tile; a window off the
# 4-column grid; 64 vertical taps over at least four chunks (an accumulator carried over chunks, negative taps)
EXTRA = {"48x32_pitch128": [], "256x32_packed": [((0, 0, 256, 32), (2, 16)), ((130, 0, 126, 32), (5, 9))],
         "32x128": [((0, 0, 32, 128), (8, 7))]}
# on the 0 / 255 pictures: the clamp engages at both ends and t goes negative
CLAMPED = [((6, 2, 38, 26), (52, 76)), ((0, 0, 46, 32), (31, 45))]


def cases_of(pic, kind):
    w, h, _ = PICS[pic]
    fits = lambda c: c[0][0] + c[0][2] <= w and c[0][1] + c[0][3] <= h      # noqa: E731
    if kind == "random":
        return [c for c in RESIZES if fits(c)] + EXTRA[pic]
    return [c for c in CLAMPED if fits(c)] + EXTRA[pic]


@pytest.fixture(scope="module")
def pictures():
    """(name, kind) -> 3 pictures in the (width, cpitch) layout (read-only):
    kind "random" bytes, or a "0/255" pattern."""
    rng = np.random.default_rng(29)
    out = {}
    for name, (w, h, cp) in PICS.items():
        n = w * h + cp * h
        out[name, "random"] = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(3)]
        out[name, "0/255"] = [(rng.integers(0, 2, n, dtype=np.uint8) * 255).astype(np.uint8) for _ in range(3)]
        for kind in ("random", "0/255"):
            for p in out[name, kind]:
                p.setflags(write=False)
    return out


def test_the_clamped_cases_leave_the_byte_range(pictures):
    """The 0 / 255 cases are what they are for: unclamped, the oracle's luma
    leaves 0..255 at both ends (so its intermediate went negative too)."""
    for pic in ("48x32_pitch128", "256x32_packed"):
        w, h, cp = PICS[pic]
        p = pictures[pic, "0/255"][0]
        for (x, y, cw, ch), (oh, ow) in CLAMPED:
            luma = p[:w * h].reshape(h, w)[y:y + ch, x:x + cw]
            raw = B.resize_unclamped(luma, oh, ow)
            assert raw.min() < 0 and raw.max() > 255, (pic, raw.min(), raw.max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_kernel_vs_oracle(pictures, mode, dtype):
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        for kind in ("random", "0/255"):
            p = pictures[pic, kind][0]
            for win, size in cases_of(pic, kind):
                for consts in consts_of(dtype):
                    rc, out, first, stride, nbytes = run_resize([p], [0], w, h, cp, win, size, mode, dtype, consts,
                                                                filt=BICUBIC)
                    assert rc == 0, (pic, kind, win, size, consts)
                    want = B.expect(p, w, h, cp, win, size, mode, dtype, consts)
                    assert same(out[first:first + nbytes], want), (pic, kind, win, size, consts)
                    assert (out[:first] == SENTINEL).all() and (out[first + nbytes:] == SENTINEL).all(), (pic, win, size)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_identity_size_is_the_unresized_export(pictures, pic, dtype):
    """(oh, ow) == (ch, cw): the bytes of h264mi_tensor_device_pitch on the
    same input (the taps are 0, 16384, 0)."""
    import torch
    from broadway_amd import _lib
    L = _mi()
    w, h, cp = PICS[pic]
    p = pictures[pic, "random"][0]
    d_in = torch.from_numpy(np.array(p)).to("cuda")
    offs = (C.c_size_t * 1)(0)
    for win in [(0, 0, w, h), (6, 2, 26, 26), (2, 2, 2, 2)]:
        for mode in sorted(T.MODES):
            rd = make_desc(win, (win[3], win[2]), mode, dtype, "imagenet")
            td = _lib.TensorDesc.from_buffer_copy(rd.t)
            nbytes = T.MODES[mode] * win[2] * win[3] * T.ELEM[dtype]
            plain = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            assert L.h264mi_tensor_device_pitch(d_in.data_ptr(), offs, 1, w, h, cp, C.byref(td), plain.data_ptr(),
                                                nbytes, torch.cuda.current_stream().cuda_stream) == 0
            rc, out, first, _, nb = run_resize([p], [0], w, h, cp, win, (win[3], win[2]), mode, dtype, "imagenet",
                                               filt=BICUBIC)
            assert rc == 0 and nb == nbytes
            assert same(out[first:first + nb], plain.cpu().numpy()), (win, mode)
            assert (out[:first] == SENTINEL).all() and (out[first + nb:] == SENTINEL).all(), (win, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_kernel_batched_padded_strides_write_nothing_else(pictures, mode, dtype):
    """Picture list [2, 0, 2] of three pictures 37 bytes apart; out_stride
    padded by 5 elements, by 48 bytes, and by 48 bytes with d_out one element
    past a 16-byte boundary: every picture is right and no pad byte changes."""
    es = T.ELEM[dtype]
    order = [2, 0, 2]
    win, size = (6, 2, 26, 26), (7, 5)
    for pic in sorted(PICS):
        w, h, cp = PICS[pic]
        pics = pictures[pic, "random"]
        for out_pad, skew in ((5 * es, 0), (48, 0), (48, es)):
            rc, out, first, stride, nbytes = run_resize(pics, order, w, h, cp, win, size, mode, dtype, "imagenet",
                                                        in_pad=37, out_pad=out_pad, skew=skew, filt=BICUBIC)
            assert rc == 0, (pic, out_pad, skew)
            assert (out[:first] == SENTINEL).all(), (pic, out_pad, skew)
            for k, i in enumerate(order):
                o = first + k * stride
                want = B.expect(pics[i], w, h, cp, win, size, mode, dtype, "imagenet")
                assert same(out[o:o + nbytes], want), (pic, out_pad, skew, k)
                assert (out[o + nbytes:o + stride] == SENTINEL).all(), (pic, out_pad, skew, k)
            assert (out[first + len(order) * stride:] == SENTINEL).all(), (pic, out_pad, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_kernel_list_longer_than_one_launch(pictures, dtype):
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128", "random"]
    order = [(5 * k + 1) % 3 for k in range(CAP + 1)]
    win, size = (6, 2, 38, 26), (7, 5)
    rc, out, first, stride, nbytes = run_resize(pics, order, w, h, cp, win, size, "rgb", dtype, "imagenet", in_pad=37,
                                                out_pad=5 * T.ELEM[dtype], filt=BICUBIC)
    assert rc == 0
    for k, i in enumerate(order):
        o = first + k * stride
        assert same(out[o:o + nbytes], B.expect(pics[i], w, h, cp, win, size, "rgb", dtype, "imagenet")), k
        assert (out[o + nbytes:o + stride] == SENTINEL).all(), k
    assert (out[:first] == SENTINEL).all() and (out[first + len(order) * stride:] == SENTINEL).all()


@pytest.mark.gpu
def test_kernel_refusals_leave_the_output_untouched(pictures):
    w, h, cp = PICS["48x32_pitch128"]
    p = pictures["48x32_pitch128", "random"][:1]

    def call(win, size, filt):
        rc, out, first, _, nbytes = run_resize(p, [0], w, h, cp, win, size, "rgb", "float16", filt=filt)
        return rc, bool((out == SENTINEL).all())

    assert call((0, 0, 32, 32), (3, 2), BICUBIC) == (0, False)          # cw == 16 ow is the cap,
    assert call((0, 0, 34, 32), (3, 2), BICUBIC) == (-1, True)          # 16 ow + 2 beyond it
    assert call((0, 0, 34, 32), (3, 2), 0) == (0, False)                # (which the triangle takes)
    assert call((0, 0, 32, 32), (1, 2), BICUBIC) == (-1, True)          # and per axis: 32 rows to 1
    assert call((0, 0, 32, 32), (2, 2), BICUBIC) == (0, False)
    for filt in (1, 3, -1):
        assert call((2, 2, 4, 4), (3, 5), filt) == (-1, True), filt


# ------------------------------------------------------ the table forms ----
def run_table(fn, pics, order, w, h, cp, desc, boxes, nbytes, gap=16, listed=None):
    """`fn`, one of the stateless table-form entry points, over pictures
    `order` of `pics` (boxes: a list of (k, window), or None for the
    descriptor's window of every picture; `listed`: the call takes a list
    argument even then); returns rc, the whole output buffer (FRONT sentinel bytes, the
    results nbytes + gap apart, 64 sentinel bytes), the first one's offset and
    the stride."""
    import torch
    from broadway_amd import _lib
    per = pics[0].size
    d_in = torch.from_numpy(np.concatenate(pics)).to("cuda")
    offs = (C.c_size_t * len(order))(*[k * per for k in order])
    n = len(order) if boxes is None else len(boxes)
    stride = nbytes + gap
    d_out = torch.full((FRONT + stride * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    extra = ((_lib.Roi * n)(*[_lib.Roi(k, *win) for k, win in boxes]), n) if boxes is not None else \
        (None, 0) if listed else ()
    rc = fn(d_in.data_ptr(), offs, len(order), w, h, cp, C.byref(desc), *extra, d_out.data_ptr() + FRONT, stride,
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), FRONT, stride


def check_table(out, first, stride, wants):
    assert (out[:first] == SENTINEL).all()
    for r, want in enumerate(wants):
        o = first + r * stride
        assert same(out[o:o + want.size], want), r
        assert (out[o + want.size:o + stride] == SENTINEL).all(), r
    assert (out[first + len(wants) * stride:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("rgb", "float16"), ("gray", "uint8")])
def test_boxes_of_different_ratios_over_two_pictures(pictures, mode, dtype):
    """h264mi_tensor_rois_device_pitch: box r is the bicubic resized tensor of
    its window -- a 16 : 1 downscale, an upscale, and one of each per axis."""
    w, h, cp = PICS["256x32_packed"]
    pics = pictures["256x32_packed", "random"]
    order = [2, 0]
    boxes = [(0, (0, 0, 144, 32)), (1, (130, 4, 4, 2)), (1, (20, 0, 10, 32))]
    size = (7, 9)
    desc = make_desc((0, 0, 0, 0), size, mode, dtype, "imagenet", filt=BICUBIC)
    nbytes = T.MODES[mode] * size[0] * size[1] * T.ELEM[dtype]
    rc, out, first, stride = run_table(_mi().h264mi_tensor_rois_device_pitch, pics, order, w, h, cp, desc, boxes, nbytes)
    assert rc == 0
    check_table(out, first, stride, [B.expect(pics[order[k]], w, h, cp, win, size, mode, dtype, "imagenet")
                                     for k, win in boxes])
    # one box beyond 16 : 1 refuses the list, which the triangle takes
    bad = boxes[:2] + [(0, (0, 0, 146, 32))]
    rc, out, _, _ = run_table(_mi().h264mi_tensor_rois_device_pitch, pics, order, w, h, cp, desc, bad, nbytes)
    assert rc == -1 and (out == SENTINEL).all()
    desc.filter = 0
    assert run_table(_mi().h264mi_tensor_rois_device_pitch, pics, order, w, h, cp, desc, bad, nbytes)[0] == 0


def fit_desc(window, size, mode, dtype, consts, how, pad):
    from broadway_amd import _lib
    d = _lib.TensorFitDesc()
    d.r = make_desc(window, size, mode, dtype, consts, filt=BICUBIC)
    d.fit = LB.FITS[how]
    d.pad[:] = tuple(pad[:T.MODES[mode]]) + (0,) * (4 - T.MODES[mode])
    return d


def letterbox_expect(pic, w, h, cp, win, size, mode, dtype, consts, how, pad):
    """tests/_letterbox.py's canvas around the bicubic content."""
    place = LB.fit(win[2], win[3], size, how)
    content = B.expect(pic, w, h, cp, win, (place[1], place[0]), mode, dtype, consts)
    return LB.compose(content, size, place, T.MODES[mode], dtype, consts, pad), place


@pytest.mark.gpu
@pytest.mark.parametrize("mode,dtype", [("rgb", "float16"), ("gray", "float32")])
def test_letterbox_with_a_pad_colour(pictures, mode, dtype):
    """h264mi_tensor_fit_device_pitch: the bars are the pad element, the
    content the bicubic bytes at the content size."""
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128", "0/255"]
    order = [1, 2]
    win, size, pad = (6, 2, 38, 26), (40, 37), (114, 7, 250)
    desc = fit_desc(win, size, mode, dtype, "imagenet", "letterbox", pad)
    nbytes = T.MODES[mode] * size[0] * size[1] * T.ELEM[dtype]
    rc, out, first, stride = run_table(_mi().h264mi_tensor_fit_device_pitch, pics, order, w, h, cp, desc, None, nbytes)
    assert rc == 0
    wants = [letterbox_expect(pics[k], w, h, cp, win, size, mode, dtype, "imagenet", "letterbox", pad) for k in order]
    rw, rh, px, py = wants[0][1]
    assert (rw, rh) == (37, 25) and py > 0                       # bars above and below
    check_table(out, first, stride, [wt for wt, _ in wants])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_layout_nhwc(pictures, dtype):
    """h264mi_tensor_layout_device_pitch, interleaved: a stretched window, and
    letterboxed boxes -- the planar bytes' elements, transposed."""
    from broadway_amd import _lib
    w, h, cp = PICS["48x32_pitch128"]
    pics = pictures["48x32_pitch128", "random"]
    order = [0, 2]
    size = (21, 19)
    nbytes = 3 * size[0] * size[1] * T.ELEM[dtype]
    L = _mi()
    win = (6, 2, 38, 26)
    d = _lib.TensorLayoutDesc()
    d.f.r = make_desc(win, size, "rgb", dtype, "imagenet", filt=BICUBIC)
    d.layout = 1
    rc, out, first, stride = run_table(L.h264mi_tensor_layout_device_pitch, pics, order, w, h, cp, d, None, nbytes,
                                       listed=True)
    assert rc == 0
    check_table(out, first, stride,
                [LY.interleave(B.expect(pics[k], w, h, cp, win, size, "rgb", dtype, "imagenet"), 3, size[0], size[1],
                               dtype) for k in order])
    # boxes, letterboxed
    pad = (114, 7, 250)
    boxes = [(1, (0, 0, 46, 32)), (0, (10, 4, 8, 26))]
    d.f = fit_desc((0, 0, 0, 0), size, "rgb", dtype, "imagenet", "letterbox", pad)
    rc, out, first, stride = run_table(L.h264mi_tensor_layout_device_pitch, pics, order, w, h, cp, d, boxes, nbytes)
    assert rc == 0
    check_table(out, first, stride,
                [LY.interleave(letterbox_expect(pics[order[k]], w, h, cp, bw, size, "rgb", dtype, "imagenet", "letterbox",
                                                pad)[0], 3, size[0], size[1], dtype) for k, bw in boxes])


# ------------------------------------------------- engine and decoder ----
def frame_expect(frame, w, h, win, size, mode, dtype, consts):
    x, y, cw, ch = win
    scale, bias = T.CONSTS[consts]
    c = T.samples(_crop.crop_i420(frame, w, h, x, y, cw, ch), cw, ch, mode)
    return T.convert(B.resize_planes(c, size[0], size[1]), dtype, scale, bias)


@pytest.mark.gpu
def test_engine_to_tensor_bicubic_vs_reference_decoder():
    """Every picture exported behind its launch on a side stream, as in
    tests/test_resize.py, through Engine.to_tensor(size=, filter="bicubic")."""
    import torch
    from broadway_amd.engine import Capture, Engine
    name = "crop_ltrb_6x4"
    win = sps_window(CASES[name])
    size = (13, 11)
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and len(frames) == cap.npics and (w, h) == (cap.w_mbs * 16, cap.h_mbs * 16)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    side = torch.cuda.Stream()
    kinds = [("rgb", torch.float16, "imagenet"), ("rgb", torch.uint8, "unit"), ("gray", torch.bfloat16, "unit"),
             ("rgb", torch.float32, "unit"), ("gray", torch.float32, "imagenet")]
    got = []
    for k, pic in enumerate(cap.pictures):
        eng.decode([0], [pic])
        mode, dtype, consts = kinds[k % len(kinds)]
        scale, bias = T.CONSTS[consts]
        got.append(eng.to_tensor([0], [pic.cur_slot], window=win, mode=mode, dtype=dtype, scale=scale, bias=bias,
                                 stream=side, size=size, filter="bicubic"))
    torch.cuda.synchronize()
    assert eng.errors() == 0
    for k, t in enumerate(got):
        mode, dtype, consts = kinds[k % len(kinds)]
        assert tuple(t.shape) == (1, T.MODES[mode]) + size and t.dtype == dtype and t.is_cuda
        assert same(tensor_bytes(t), frame_expect(frames[k], w, h, win, size, mode, str(dtype).split(".")[1], consts)), k
    # the other forms take the keyword too: boxes, a letterbox, channels-last
    slot = cap.pictures[-1].cur_slot
    boxes = [(0, 6, 2, 86, 52), (0, 10, 4, 8, 26)]
    t = eng.to_tensor([0], [slot], rois=boxes, size=size, dtype=torch.uint8, filter="bicubic")
    u = eng.to_tensor([0], [slot], window=win, size=(16, 16), dtype=torch.uint8, fit="letterbox", pad=9, filter="bicubic")
    v = eng.to_tensor([0], [slot], window=win, size=size, dtype=torch.uint8, layout="nhwc", filter="bicubic")
    torch.cuda.synchronize()
    for r, b in enumerate(boxes):
        assert same(tensor_bytes(t[r]), frame_expect(frames[-1], w, h, b[1:], size, "rgb", "uint8", "unit")), r
    place = LB.fit(win[2], win[3], (16, 16), "letterbox")
    content = frame_expect(frames[-1], w, h, win, (place[1], place[0]), "rgb", "uint8", "unit")
    assert same(tensor_bytes(u), LB.compose(content, (16, 16), place, 3, "uint8", "unit", (9, 9, 9)))
    assert same(tensor_bytes(v.permute(0, 2, 3, 1)),
                LY.interleave(frame_expect(frames[-1], w, h, win, size, "rgb", "uint8", "unit"), 3, size[0], size[1], "uint8"))
    with pytest.raises(RuntimeError):
        eng.to_tensor([0], [slot], window=(0, 0, w, 4), size=(1, 5), filter="bicubic")      # 96 to 5: beyond 16 : 1
    assert tuple(eng.to_tensor([0], [slot], window=(0, 0, w, 4), size=(1, 5)).shape) == (1, 3, 1, 5)


def decode_js(nals, opts, on_picture=None):
    got, dims = [], []
    dec = Decoder(opts)

    def cb(buf, w, h, infos):
        got.append(buf)
        dims.append((w, h))
        if on_picture:
            on_picture(dec)

    dec.onPictureDecoded = cb
    for nal in nals:
        dec.decode(nal)
    dec.close()
    return got, dims


@pytest.mark.gpu
def test_decoder_tensor_filter_option_and_rois_vs_reference():
    """Decoder({"tensor": {"size": (26, 43), "filter": "bicubic"}}) and, inside
    the callback, Decoder.rois(..., filter="bicubic") with boxes in the
    delivered (crop) window's coordinates."""
    import torch
    c = CASES["crop_ltrb_6x4"]
    win = sps_window(c)
    assert win == (6, 2, 86, 52)
    size = (26, 43)
    frames, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    nals = split_annexb(case_stream("crop_ltrb_6x4"))
    boxes = [(0, 0, 20, 12), (82, 48, 4, 4), (0, 0, 86, 52)]
    bsize = (5, 9)
    rois = []
    got, dims = decode_js(nals, {"tensor": {"dtype": torch.float16, "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD,
                                            "size": size, "filter": "bicubic"}},
                          lambda dec: rois.append(dec.rois(boxes, bsize, dtype=torch.uint8, filter="bicubic")))
    gray, gdims = decode_js(nals, {"tensor": {"dtype": torch.uint8, "mode": "gray", "size": size, "filter": "bicubic"}})
    torch.cuda.synchronize()
    assert len(got) == len(gray) == len(rois) == len(frames) and set(dims) == set(gdims) == {(size[1], size[0])}
    for k, (t, g) in enumerate(zip(got, gray)):
        assert t.dtype == torch.float16 and tuple(t.shape) == (3,) + size and t.is_cuda
        assert g.dtype == torch.uint8 and tuple(g.shape) == (1,) + size and g.is_cuda
        assert same(tensor_bytes(t), frame_expect(frames[k], w, h, win, size, "rgb", "float16", "imagenet")), k
        assert same(tensor_bytes(g), frame_expect(frames[k], w, h, win, size, "gray", "uint8", "unit")), k
        assert tuple(rois[k].shape) == (3, 3) + bsize
        for r, (x, y, cw, ch) in enumerate(boxes):
            at = (x + win[0], y + win[1], cw, ch)
            assert same(tensor_bytes(rois[k][r]), frame_expect(frames[k], w, h, at, bsize, "rgb", "uint8", "unit")), (k, r)
