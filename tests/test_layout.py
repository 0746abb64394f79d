"""Channels-last (interleaved) layout of the RGB tensor exports:
h264mi_tensor_layout_device_pitch, h264mi_engine_export_tensor_layout
(Engine.to_tensor(layout="nhwc")), H264SwDecNextPictureTensorLayout (the
Decoder's ``tensor`` option) and H264SwDecLastPictureTensorRoisLayout
(Decoder.rois(layout=)).

Every comparison is exact equality of bytes.  The oracle is the planar one --
tests/_tensor.py, _resize.py, _colour.py and _letterbox.py give a picture's
(planes, rows, cols) elements -- with the elements transposed to (rows, cols,
planes) by tests/_layout.py.  Every kernel case has sentinel bytes in front of
and behind each picture's elements and checks them afterwards."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import _colour as K
import _crop
import _layout as Y
import _letterbox as LB
import _resize as R
import _tensor as T
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CASES = _crop.cases()
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}       # tests/test_rois.py's layouts
ORDER = [2, 0, 2]           # the picture list of every kernel test
BOXES = [(0, (6, 2, 38, 26)), (1, (2, 2, 2, 2)), (2, (44, 30, 4, 2)), (1, (0, 0, 46, 32))]    # tests/test_rois.py's
PAD = (114, 7, 250)         # a different sample per plane
# tests/test_letterbox.py's GEOMETRIES rows 1, 2 and 7: an all-bar tile, content narrower than a tile, bars above and
# below the content inside one tile -- (layout, window, canvas (oh, ow), fit, (rw, rh, px, py))
GEOMETRIES = [
    ("48x32_pitch128", (6, 2, 38, 26), (40, 70), "letterbox", (58, 40, 6, 0)),
    ("48x32_pitch128", (2, 2, 2, 2), (40, 70), "letterbox", (40, 40, 15, 0)),
    ("48x32_pitch128", (4, 4, 12, 6), (9, 6), "letterbox", (6, 3, 0, 3)),
]
SENTINEL = 0xA5
FRONT = 64
GAP = 16                    # sentinel bytes between two pictures (a multiple of 16: the wide stores stay possible)
PLANAR, INTERLEAVED = 0, 1


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
    """name -> 3 random pictures in the (width, cpitch) layout (read-only), on
    the host and on the device; tests/test_rois.py's."""
    import torch
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        pics = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in pics:
            p.setflags(write=False)
        out[name] = (pics, torch.from_numpy(np.concatenate(pics)).to("cuda"))
    return out


def make_desc(layout, mode, dtype, consts="unit", colour=0, window=(0, 0, 0, 0), size=None, how="stretch", pad=(0, 0, 0)):
    """An h264mi_tensor_layout_desc: no size is the unresized export."""
    from broadway_amd import _lib
    d = _lib.TensorLayoutDesc()
    t = d.f.r.t
    t.x, t.y, t.cw, t.ch = window
    t.mode = {"rgb": 0, "gray": 1}[mode] | colour << 8
    t.dtype = T.DTYPES.index(dtype)
    scale, bias = T.CONSTS[consts]
    t.scale[:] = scale
    t.bias[:] = bias
    if size is not None:
        d.f.r.oh, d.f.r.ow = size
    d.f.fit = LB.FITS[how]
    d.f.pad[:] = tuple(pad) + (0,) * (4 - len(pad))
    d.layout = layout
    return d


def make_rois(boxes):
    from broadway_amd import _lib
    return (_lib.Roi * len(boxes))(*[_lib.Roi(k, *win) for k, win in boxes])


def run_layout(pics_dev, layout_name, order, desc, boxes, nbytes, skew=0, gap=GAP, call=None):
    """h264mi_tensor_layout_device_pitch (or `call`, an existing entry point
    given as (function, descriptor, takes boxes)) over the pictures `order`;
    returns rc, the whole output buffer (FRONT + skew sentinel bytes, then the
    pictures or boxes nbytes + gap apart, then 64 sentinel bytes), the first
    one's offset and the stride."""
    import torch
    w, h, cp = PICS[layout_name]
    L = _mi()
    per = w * h + cp * h
    offs = (C.c_size_t * len(order))(*[k * per for k in order])
    n = len(boxes) if boxes is not None else len(order)
    first, stride = FRONT + skew, nbytes + gap
    d_out = torch.full((first + stride * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    head = (pics_dev.data_ptr(), offs, len(order), w, h, cp)
    if call is None:
        rc = L.h264mi_tensor_layout_device_pitch(*head, C.byref(desc), make_rois(boxes) if boxes is not None else None,
                                                 n if boxes is not None else 0, d_out.data_ptr() + first, stride, st)
    else:
        fn, old, listed = call
        extra = (make_rois(boxes), n) if listed else ()
        rc = fn(*head, C.byref(old), *extra, d_out.data_ptr() + first, stride, st)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), first, stride


def same(got, want):
    """Exact equality; what differs is printed before the assertion fails."""
    if got.shape == want.shape and np.array_equal(got, want):
        return True
    if got.shape != want.shape:
        print(f"shapes differ: {got.shape} {want.shape}")
    else:
        bad = np.flatnonzero(got != want)
        print(f"{bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()} "
              f"want {want[bad[:8]].tolist()}")
    return False


def check(out, first, stride, wants):
    """Picture or box r equals wants[r] and no byte outside them changed."""
    assert (out[:first] == SENTINEL).all()
    for r, want in enumerate(wants):
        o = first + r * stride
        assert same(out[o:o + want.size], want), r
        assert (out[o + want.size:o + stride] == SENTINEL).all(), r
    assert (out[first + len(wants) * stride:] == SENTINEL).all()


def planar_expect(pic, w, h, cp, win, mode, dtype, consts, colour=0, size=None):
    """The planar oracle's bytes of one window, resized to `size` if given."""
    if colour:
        return K.expect(pic, w, h, cp, tuple(win), colour, dtype, consts, size=size)
    if size is None:
        return T.expect(pic, w, h, cp, win, mode, dtype, consts)
    return R.expect(pic, w, h, cp, win, size, mode, dtype, consts)


def hwc_expect(pic, w, h, cp, win, dtype, consts, colour=0, size=None):
    rows, cols = size if size is not None else (win[3], win[2])
    return Y.interleave(planar_expect(pic, w, h, cp, win, "rgb", dtype, consts, colour, size), 3, rows, cols, dtype)


def consts_of(dtype):
    """Per-plane constants that differ, so that a plane mix-up shows; uint8 ignores them."""
    return "unit" if dtype == "uint8" else "imagenet"


# ---------------------------------------------------------------- k_tensor ---
@pytest.mark.gpu
@pytest.mark.parametrize("colour", [0, 2])
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_plain_interleaved_vs_oracle(pictures, dtype, colour):
    """The unresized export, interleaved: the whole 48-column window (rows of
    3 * 48 elements: the 16-byte path for every type) on both layouts, and a
    window with x = 2 mod 4 whose last group is 2 columns wide."""
    es, consts = T.ELEM[dtype], consts_of(dtype)
    for name in sorted(PICS):
        w, h, cp = PICS[name]
        pics, dev = pictures[name]
        for win in ((0, 0, 48, 32), (2, 2, 6, 4)):
            nbytes = 3 * win[2] * win[3] * es
            desc = make_desc(INTERLEAVED, "rgb", dtype, consts, colour, win)
            rc, out, first, stride = run_layout(dev, name, ORDER, desc, None, nbytes)
            assert rc == 0, (name, win)
            check(out, first, stride, [hwc_expect(pics[k], w, h, cp, win, dtype, consts, colour) for k in ORDER])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_plain_interleaved_off_the_16_byte_grid(pictures, dtype):
    """The 48-column window with d_out skewed by one element, and with an
    out_stride that is no multiple of 16: both take the element path, and both
    give the same bytes."""
    es, consts, name, win = T.ELEM[dtype], consts_of(dtype), "48x32_pitch128", (0, 0, 48, 32)
    w, h, cp = PICS[name]
    pics, dev = pictures[name]
    nbytes = 3 * win[2] * win[3] * es
    wants = [hwc_expect(pics[k], w, h, cp, win, dtype, consts, 2) for k in ORDER]
    desc = make_desc(INTERLEAVED, "rgb", dtype, consts, 2, win)
    for skew, gap in ((es, GAP), (0, GAP + es)):
        assert (FRONT + skew) % 16 or (nbytes + gap) % 16
        rc, out, first, stride = run_layout(dev, name, ORDER, desc, None, nbytes, skew=skew, gap=gap)
        assert rc == 0, (skew, gap)
        check(out, first, stride, wants)
    # (a d_out that is no multiple of the element size is refused, as by the planar call)
    if es > 1:
        rc, out, *_ = run_layout(dev, name, ORDER, desc, None, nbytes, skew=1)
        assert rc == -1 and (out == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_plain_interleaved_33_pictures_take_a_second_launch(pictures, dtype):
    es, consts, name, win = T.ELEM[dtype], consts_of(dtype), "48x32_pitch128", (0, 0, 4, 2)
    w, h, cp = PICS[name]
    pics, dev = pictures[name]
    order = [k % 3 for k in range(33)]
    desc = make_desc(INTERLEAVED, "rgb", dtype, consts, 0, win)
    rc, out, first, stride = run_layout(dev, name, order, desc, None, 3 * 4 * 2 * es)
    assert rc == 0
    check(out, first, stride, [hwc_expect(pics[k], w, h, cp, win, dtype, consts) for k in order])


# --------------------------------------------------------- k_tensor_resize ---
RESIZED = [
    ("48x32_pitch128", (6, 2, 38, 26), (40, 70)),       # three tile columns, the last 6 wide, and a tile row of 8
    ("256x32_packed", (0, 0, 256, 32), (3, 8)),         # 64 taps
    ("48x32_pitch128", (2, 2, 2, 2), (7, 5)),           # an upscale of a 2 x 2 window
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_resized_interleaved_vs_oracle(pictures, dtype):
    es, consts = T.ELEM[dtype], consts_of(dtype)
    for name, win, size in RESIZED:
        w, h, cp = PICS[name]
        pics, dev = pictures[name]
        for colour in (0, 3):
            desc = make_desc(INTERLEAVED, "rgb", dtype, consts, colour, win, size)
            rc, out, first, stride = run_layout(dev, name, ORDER, desc, None, 3 * size[0] * size[1] * es)
            assert rc == 0, (name, win, size)
            check(out, first, stride, [hwc_expect(pics[k], w, h, cp, win, dtype, consts, colour, size) for k in ORDER])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_rois_interleaved_33_boxes_take_a_second_launch(pictures, dtype):
    es, consts, name, size = T.ELEM[dtype], consts_of(dtype), "48x32_pitch128", (7, 5)
    w, h, cp = PICS[name]
    pics, dev = pictures[name]
    boxes = (BOXES * 9)[:33]
    desc = make_desc(INTERLEAVED, "rgb", dtype, consts, 0, size=size)
    rc, out, first, stride = run_layout(dev, name, ORDER, desc, boxes, 3 * size[0] * size[1] * es)
    assert rc == 0
    check(out, first, stride, [hwc_expect(pics[ORDER[k]], w, h, cp, win, dtype, consts, 0, size) for k, win in boxes])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_letterbox_interleaved_vs_oracle(pictures, dtype):
    """An all-bar tile, content narrower than a tile, bars above and below
    inside one tile; a different pad sample per plane; as one window per
    picture and as a list of boxes."""
    es, consts = T.ELEM[dtype], consts_of(dtype)
    for name, win, size, how, place in GEOMETRIES:
        assert LB.fit(win[2], win[3], size, how) == place
        w, h, cp = PICS[name]
        pics, dev = pictures[name]
        nbytes = 3 * size[0] * size[1] * es
        wants = [Y.interleave(LB.expect(pics[k], w, h, cp, win, size, "rgb", dtype, consts, how, PAD), 3, size[0],
                              size[1], dtype) for k in ORDER]
        desc = make_desc(INTERLEAVED, "rgb", dtype, consts, 0, win, size, how, PAD)
        rc, out, first, stride = run_layout(dev, name, ORDER, desc, None, nbytes)
        assert rc == 0, (win, size)
        check(out, first, stride, wants)
        desc = make_desc(INTERLEAVED, "rgb", dtype, consts, 0, size=size, how=how, pad=PAD)
        rc, out, first, stride = run_layout(dev, name, ORDER, desc, [(k, win) for k in range(3)], nbytes)
        assert rc == 0, (win, size)
        check(out, first, stride, wants)


# ------------------------------------------------- PLANAR and GRAY: the old bytes ---
def old_calls(mode, dtype, consts, colour, win, size, how, pad):
    """(name, new descriptor fields, existing call) of the four exports on one
    window / list: the existing entry point with its own descriptor."""
    from broadway_amd import _lib
    L = _mi()
    full = make_desc(PLANAR, mode, dtype, consts, colour, win, size, how, pad)
    lst = make_desc(PLANAR, mode, dtype, consts, colour, (0, 0, 0, 0), size, how, pad)
    stretch = make_desc(PLANAR, mode, dtype, consts, colour, win, size)
    stretch_lst = make_desc(PLANAR, mode, dtype, consts, colour, (0, 0, 0, 0), size)
    plain = make_desc(PLANAR, mode, dtype, consts, colour, win)
    r, rl = _lib.TensorResizeDesc(), _lib.TensorResizeDesc()
    C.memmove(C.byref(r), C.byref(stretch.f.r), C.sizeof(r))
    C.memmove(C.byref(rl), C.byref(stretch_lst.f.r), C.sizeof(rl))
    return [
        ("plain", plain, False, (win[3], win[2]), (L.h264mi_tensor_device_pitch, plain.f.r.t, False)),
        ("resized", stretch, False, size, (L.h264mi_tensor_resize_device_pitch, r, False)),
        ("rois", stretch_lst, True, size, (L.h264mi_tensor_rois_device_pitch, rl, True)),
        ("fit", full, False, size, (L.h264mi_tensor_fit_device_pitch, full.f, False)),
        ("rois_fit", lst, True, size, (L.h264mi_tensor_rois_fit_device_pitch, lst.f, True)),
    ]


@pytest.mark.gpu
def test_planar_through_the_new_call_is_the_existing_call(pictures):
    """PLANAR: byte for byte what h264mi_tensor_device_pitch, _resize_, _rois_,
    _fit_ and _rois_fit_device_pitch give, sentinels included."""
    name, win, size, dtype = "48x32_pitch128", (6, 2, 38, 26), (40, 70), "float16"
    pics, dev = pictures[name]
    for what, desc, listed, (rows, cols), call in old_calls("rgb", dtype, "imagenet", 2, win, size, "letterbox", PAD):
        boxes = BOXES if listed else None
        nbytes = 3 * rows * cols * 2
        rc, got, first, stride = run_layout(dev, name, ORDER, desc, boxes, nbytes)
        rc_old, want, *_ = run_layout(dev, name, ORDER, None, boxes, nbytes, call=call)
        assert rc == 0 and rc_old == 0, what
        assert (want != SENTINEL).sum() > nbytes // 2 and same(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_gray_is_the_existing_bytes_in_both_layouts(pictures, layout):
    name, win, size, dtype = "48x32_pitch128", (6, 2, 38, 26), (40, 70), "bfloat16"
    pics, dev = pictures[name]
    for what, desc, listed, (rows, cols), call in old_calls("gray", dtype, "imagenet", 0, win, size, "topleft", (9, 0, 0)):
        desc.layout = layout
        boxes = BOXES if listed else None
        nbytes = rows * cols * 2
        rc, got, first, stride = run_layout(dev, name, ORDER, desc, boxes, nbytes)
        rc_old, want, *_ = run_layout(dev, name, ORDER, None, boxes, nbytes, call=call)
        assert rc == 0 and rc_old == 0, what
        assert (want != SENTINEL).sum() > nbytes // 2 and same(got, want), what


@pytest.mark.gpu
def test_bad_descriptors_launch_nothing(pictures):
    name, win = "48x32_pitch128", (0, 0, 48, 32)
    pics, dev = pictures[name]
    bad = [make_desc(2, "rgb", "uint8", window=win), make_desc(-1, "rgb", "uint8", window=win),
           make_desc(INTERLEAVED, "rgb", "uint8", window=win, how="letterbox"),
           make_desc(INTERLEAVED, "rgb", "uint8", window=win, pad=(1, 0, 0)),
           make_desc(INTERLEAVED, "rgb", "uint8", window=win, size=(0, 8)),
           make_desc(INTERLEAVED, "rgb", "uint8", colour=15, window=win),
           make_desc(INTERLEAVED, "rgb", "uint8", window=(0, 0, 50, 32))]
    for k, desc in enumerate(bad):
        rc, out, *_ = run_layout(dev, name, ORDER, desc, None, 3 * 48 * 32)
        assert rc == -1 and (out == SENTINEL).all(), k
    # boxes need a size and a reserved window
    for k, desc in enumerate([make_desc(INTERLEAVED, "rgb", "uint8"),
                              make_desc(INTERLEAVED, "rgb", "uint8", window=win, size=(7, 5))]):
        rc, out, *_ = run_layout(dev, name, ORDER, desc, BOXES, 3 * 7 * 5)
        assert rc == -1 and (out == SENTINEL).all(), k


# ------------------------------------------------------- through the layers ---
def sps_window(case):
    p = case["cropParams"]
    return (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])


def hwc_bytes(t):
    """The bytes of the contiguous HWC view of an "nhwc" result."""
    import torch
    v = t.permute(0, 2, 3, 1) if t.dim() == 4 else t.permute(1, 2, 0)
    assert v.is_contiguous()
    return v.view(torch.uint8).cpu().numpy().reshape(-1)


@pytest.mark.gpu
def test_engine_to_tensor_nhwc_in_every_form():
    """Engine.to_tensor(layout="nhwc") for window, size, rois and fit: the
    usual shape with channels-last strides, torch.equal with the "nchw"
    result, and the HWC view's bytes equal the oracle's on the reference
    decoder's pictures; out= is filled in place."""
    import torch
    from broadway_amd.engine import Capture, Engine, empty_layout
    name = "crop_ltrb_6x4"          # the smallest case: 96 x 64
    frames, errs, w, h, _ = O.decode(case_stream(name))
    cap = Capture(case_stream(name))
    assert errs == 0 and (w, h) == (96, 64)
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    held = list(range(min(again, 2)))
    ss, sl = [0] * len(held), [slots[k] for k in held]
    win, size = sps_window(CASES[name]), (20, 50)
    rois = [(len(held) - 1, 6, 2, 86, 52), (0, 0, 0, 96, 64), (0, 2, 2, 2, 2), (0, 10, 20, 26, 38)]
    kw = dict(dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD, colour="bt709-full")
    forms = {
        "window": (dict(window=win), lambda k: K.frame_expect(frames[k], w, h, win, 3, "float16", "imagenet")),
        "size": (dict(window=win, size=size),
                 lambda k: K.frame_expect(frames[k], w, h, win, 3, "float16", "imagenet", size=size)),
        "fit": (dict(window=win, size=size, fit="letterbox", pad=PAD),
                lambda k: LB.frame_expect(frames[k], w, h, win, size, "rgb", "float16", "imagenet", "letterbox", PAD, 3)),
    }
    for what, (args, want) in forms.items():
        a = eng.to_tensor(ss, sl, layout="nhwc", **args, **kw)
        b = eng.to_tensor(ss, sl, **args, **kw)
        torch.cuda.synchronize()
        n, p, rows, cols = a.shape
        assert (n, p) == (len(held), 3) and a.shape == b.shape and b.is_contiguous(), what
        assert a.stride() == (rows * cols * 3, 1, cols * 3, 3) and a.is_contiguous(memory_format=torch.channels_last), what
        assert torch.equal(a, b), what
        for r, k in enumerate(held):
            assert same(hwc_bytes(a[r]), Y.interleave(want(k), 3, rows, cols, "float16")), (what, r)
    for fit in (None, "topleft"):
        args = dict(rois=rois, size=size) if fit is None else dict(rois=rois, size=size, fit=fit, pad=PAD)
        out = empty_layout((len(rois), 3) + size, torch.float16, torch.device("cuda", eng.device), "nhwc")
        a = eng.to_tensor(ss, sl, layout="nhwc", out=out, **args, **kw)
        b = eng.to_tensor(ss, sl, **args, **kw)
        torch.cuda.synchronize()
        assert a is out and a.stride() == (size[0] * size[1] * 3, 1, size[1] * 3, 3) and torch.equal(a, b), fit
        for r, (k, x, y, cw, ch) in enumerate(rois):
            want = LB.frame_expect(frames[held[k]], w, h, (x, y, cw, ch), size, "rgb", "float16", "imagenet",
                                   fit or "stretch", PAD, 3)
            assert same(hwc_bytes(a[r]), Y.interleave(want, 3, size[0], size[1], "float16")), (fit, r)
    # gray: one plane has one order -- the same bytes, whichever layout is named
    g = eng.to_tensor(ss, sl, window=win, mode="gray", dtype=torch.uint8, layout="nhwc")
    assert torch.equal(g, eng.to_tensor(ss, sl, window=win, mode="gray", dtype=torch.uint8))
    # out= in the other layout: refused before the library is called
    with pytest.raises(ValueError):
        eng.to_tensor(ss, sl, window=win, layout="nhwc", out=torch.empty((len(held), 3, win[3], win[2]),
                                                                        dtype=torch.float16, device="cuda"), **kw)
    with pytest.raises(ValueError):
        eng.to_tensor(ss, sl, window=win, out=empty_layout((len(held), 3, win[3], win[2]), torch.float16,
                                                           torch.device("cuda", eng.device), "nhwc"), **kw)
    assert eng.errors() == 0


@pytest.mark.gpu
def test_decoder_option_and_rois_nhwc():
    """Decoder({"tensor": {"layout": "nhwc", ...}}) and Decoder.rois(layout=
    "nhwc") over the SPS crop window, against the oracle at the crop-offset
    coordinates, with the colour taken from the stream."""
    import torch
    name = "crop_ltrb_6x4"
    win = sps_window(CASES[name])
    assert win == (6, 2, 86, 52)
    frames, _, w, h, _ = O.decode(case_stream(name))
    boxes = [(0, 0, 20, 12), (82, 48, 4, 4), (0, 0, 86, 52)]
    size = (24, 24)
    got = []

    def cb(buf, pw, ph, infos):
        got.append((buf, dec.rois(boxes, size, dtype=torch.float32, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD,
                                  fit="letterbox", pad=PAD, layout="nhwc"), dec.tensor_colour))

    dec = Decoder({"tensor": {"layout": "nhwc", "dtype": torch.bfloat16, "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD,
                              "colour": "stream"}})
    dec.onPictureDecoded = cb
    for nal in split_annexb(case_stream(name)):
        dec.decode(nal)
    dec.close()
    torch.cuda.synchronize()
    assert len(got) == len(frames)
    for k, (whole, t, colour) in enumerate(got):
        assert colour == "reference"                                # (the stream names no matrix: BT.601 limited)
        assert tuple(whole.shape) == (3, 52, 86) and whole.stride() == (1, 86 * 3, 3), k
        want = T.convert(T.samples(_crop.crop_i420(frames[k], w, h, *win), 86, 52, "rgb"), "bfloat16",
                         *T.CONSTS["imagenet"])
        assert same(hwc_bytes(whole), Y.interleave(want, 3, 52, 86, "bfloat16")), k
        assert tuple(t.shape) == (3, 3) + size and t.stride() == (size[0] * size[1] * 3, 1, size[1] * 3, 3), k
        for r, (x, y, cw, ch) in enumerate(boxes):
            at = (x + win[0], y + win[1], cw, ch)
            want = LB.frame_expect(frames[k], w, h, at, size, "rgb", "float32", "imagenet", "letterbox", PAD)
            assert same(hwc_bytes(t[r]), Y.interleave(want, 3, size[0], size[1], "float32")), (k, r)
