"""Strided destinations of the pixel exports:
h264mi_tensor_dest_device_pitch and h264mi_tensor_warps_dest_device_pitch on
the three kernels, Engine.to_tensor(out=view, clip=T) and the Decoder's
``tensor: {"clip": T, "step": s}`` option.

Every comparison is exact equality of bytes.  The expected bytes are those of
the existing planar and interleaved oracles (tests/_tensor.py, _resize.py,
_bicubic.py, _letterbox.py, _warp.py, _layout.py), scattered through the
descriptor by tests/_dest.py into a buffer of sentinel bytes; every kernel case
compares the whole buffer, so every byte the descriptor does not address --
row padding, the gaps between planes, frames and clips, front and tail -- must
still be the sentinel."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import oracle as O
import _bicubic as B
import _colour as K
import _crop
import _dest as D
import _layout as Y
import _letterbox as LB
import _resize as R
import _tensor as T
import _warp as W
import test_layout as TL
from _dest import Dest
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

CASES = _crop.cases()
PICS = TL.PICS              # tests/test_rois.py's layouts: 48x32_pitch128, 256x32_packed
SENTINEL = D.SENTINEL
assert SENTINEL == TL.SENTINEL
FRONT = 64
TAIL = 64
PAD = TL.PAD
PLANAR, INTERLEAVED = 0, 1
TRIANGLE, BICUBIC = 0, B.FILTER
ORDER3 = [2, 0, 2]
ORDER6 = [2, 0, 2, 1, 0, 1]
ORDER8 = [2, 0, 2, 1, 0, 1, 2, 0]


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
    """tests/test_rois.py's random pictures: name -> (3 pictures on the host,
    read-only, and the same on the device)."""
    import torch
    rng = np.random.default_rng(23)
    out = {}
    for name, (w, h, cp) in PICS.items():
        pics = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in pics:
            p.setflags(write=False)
        out[name] = (pics, torch.from_numpy(np.concatenate(pics)).to("cuda"))
    return out


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


def run(dev, name, order, nitems, shape, dest, out_stride, call, skew=0):
    """One export of `nitems` items of shape = (es, planes, rows, cols,
    interleaved) over the pictures `order` into a sentinel buffer: FRONT + skew
    bytes, then what the descriptor addresses, then TAIL bytes.  `call(head,
    c_dest, d_out, out_stride, stream)` makes the library call.  Returns rc, the
    whole buffer, the items' base and the buffer's size."""
    import torch
    w, h, cp = PICS[name]
    per = w * h + cp * h
    offs = (C.c_size_t * len(order))(*[k * per for k in order])
    base = FRONT + skew
    total = base + D.extent(dest, nitems, out_stride, *shape) + TAIL
    d_out = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    rc = call((dev.data_ptr(), offs, len(order), w, h, cp), D.c_dest(dest), d_out.data_ptr() + base, out_stride, st)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), base, total


def layout_call(desc, boxes=None):
    """h264mi_tensor_dest_device_pitch under `desc`, over `boxes` if given."""
    def call(head, dest, d_out, out_stride, st):
        rois = TL.make_rois(boxes) if boxes is not None else None
        return _mi().h264mi_tensor_dest_device_pitch(*head, C.byref(desc), rois, len(boxes) if boxes is not None else 0,
                                                     dest, d_out, out_stride, st)
    return call


def existing_layout_call(desc, boxes=None):
    """h264mi_tensor_layout_device_pitch: the call without a destination."""
    def call(head, dest, d_out, out_stride, st):
        assert dest is None
        rois = TL.make_rois(boxes) if boxes is not None else None
        return _mi().h264mi_tensor_layout_device_pitch(*head, C.byref(desc), rois, len(boxes) if boxes is not None else 0,
                                                       d_out, out_stride, st)
    return call


def check(rc, out, base, total, items, dest, out_stride, shape, what):
    assert rc == 0, what
    assert same(out, D.scatter(total, base, items, dest, out_stride, *shape)), what


# ---------------------------------------------------------------- k_tensor ---
def tensor_dests(es, planes, rows, cols, interleaved):
    """name -> (pictures, Dest, out_stride, d_out's skew) of the five
    destinations of the unresized export."""
    packed = cols * es * (planes if interleaved else 1)
    item = rows * packed * (1 if interleaved else planes)
    wide = packed + 16
    odd = packed + es
    return {
        # what the call without a descriptor does, spelt out; the items 16 bytes apart
        "contiguous": (ORDER3, Dest(packed, 0 if interleaved else rows * packed, 0, 1), item + 16),
        # a row and a plane each padded by 16 bytes: the 16-byte stores stay possible
        "padded_16": (ORDER3, Dest(wide, 0 if interleaved else rows * wide + 16, 0, 1),
                      (rows * wide if interleaved else planes * (rows * wide + 16)) + 16),
        # a row padded by one element: rows off the 16-byte grid, the element path
        "padded_element": (ORDER3, Dest(odd, 0, 0, 1), (rows * odd if interleaved else planes * rows * odd)),
        # (N, C, T, H, W), T = 3, contiguous; interleaved: (N, T, H, W, C), channels_last_3d's memory
        "ncthw": (ORDER6, Dest(0, 0 if interleaved else 3 * rows * packed, rows * packed, 3),
                  3 * item),
        # a 2 x 4 grid of tiles in one canvas (C, 2 rows, 4 cols) / (2 rows, 4 cols, C): a clip is a row of tiles
        "tiles_2x4": (ORDER8, Dest(4 * packed, 0 if interleaved else 2 * rows * 4 * packed, packed, 4), rows * 4 * packed),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("mode,dtype", [("rgb", "uint8"), ("rgb", "float16"), ("rgb", "float32"), ("gray", "uint8")])
def test_unresized_into_five_destinations(pictures, mode, dtype, layout):
    """k_tensor: the whole 48 x 32 window (the 16-byte stores can run) and
    (6, 2, 38, 26) (cw = 2 mod 4: the element path, a last group 2 columns wide)
    into the five destinations, on both picture layouts."""
    es, planes, consts = T.ELEM[dtype], T.MODES[mode], TL.consts_of(dtype)
    for name in sorted(PICS):
        w, h, cp = PICS[name]
        pics, dev = pictures[name]
        for win in ((0, 0, 48, 32), (6, 2, 38, 26)):
            rows, cols = win[3], win[2]
            shape = (es, planes, rows, cols, layout == INTERLEAVED)
            desc = TL.make_desc(layout, mode, dtype, consts, 0, win)
            want = {}
            for k in range(3):
                p = T.expect(pics[k], w, h, cp, win, mode, dtype, consts)
                want[k] = Y.interleave(p, planes, rows, cols, dtype) if layout == INTERLEAVED and planes == 3 else p
            for what, (order, dest, out_stride) in tensor_dests(*shape).items():
                rc, out, base, total = run(dev, name, order, len(order), shape, dest, out_stride, layout_call(desc))
                check(rc, out, base, total, [want[k] for k in order], dest, out_stride, shape, (name, win, what))
                if what == "contiguous":
                    # the same bytes, sentinels included, as the call that takes no descriptor
                    rc0, out0, *_ = run(dev, name, order, len(order), shape, None, out_stride, existing_layout_call(desc))
                    assert rc0 == 0 and same(out, out0), (name, win)


@pytest.mark.gpu
def test_unresized_null_and_all_zero_are_the_existing_call(pictures):
    """dest NULL and the all-zero descriptor with clip 1: the packed items of
    h264mi_tensor_layout_device_pitch, byte for byte, with d_out off the
    16-byte grid too."""
    name, win, dtype = "48x32_pitch128", (0, 0, 48, 32), "float16"
    pics, dev = pictures[name]
    shape = (2, 3, 32, 48, False)
    desc = TL.make_desc(PLANAR, "rgb", dtype, "imagenet", 2, win)
    for skew in (0, 2):
        stride = 3 * 32 * 48 * 2 + 32
        rc0, out0, *_ = run(dev, name, ORDER3, 3, shape, None, stride, existing_layout_call(desc), skew)
        for dest in (None, Dest()):
            rc, out, *_ = run(dev, name, ORDER3, 3, shape, dest, stride, layout_call(desc), skew)
            assert rc == 0 and rc0 == 0 and (out0 != SENTINEL).sum() > stride and same(out, out0), (skew, dest)


@pytest.mark.gpu
def test_bad_destinations_launch_nothing(pictures):
    """dest_ok's refusals at the entry point: -1 and not a byte written."""
    name, win = "48x32_pitch128", (0, 0, 48, 32)
    pics, dev = pictures[name]
    shape = (2, 3, 32, 48, False)
    desc = TL.make_desc(PLANAR, "rgb", "float16", "unit", 0, win)
    item = 3 * 32 * 96
    bad = [(Dest(94, 0, 0, 1), item), (Dest(97, 0, 0, 1), item), (Dest(0, 32 * 96 - 2, 0, 1), item),
           (Dest(0, 0, 0, 2), item), (Dest(0, 0, item, 1), item), (Dest(0, 0, item - 2, 3), 3 * item),
           (Dest(0, 0, 0, 0), item), (Dest(0, 0, 0, 1), item - 2), (Dest(-96, 0, 0, 1), item)]
    import torch
    for k, (dest, out_stride) in enumerate(bad):
        d_out = torch.full((FRONT + 4 * item,), SENTINEL, dtype=torch.uint8, device="cuda")
        w, h, cp = PICS[name]
        offs = (C.c_size_t * 3)(*[i * (w * h + cp * h) for i in ORDER3])
        rc = _mi().h264mi_tensor_dest_device_pitch(dev.data_ptr(), offs, 3, w, h, cp, C.byref(desc), None, 0, D.c_dest(dest),
                                                   d_out.data_ptr() + FRONT, out_stride, None)
        torch.cuda.synchronize()
        assert rc == -1 and bool((d_out == SENTINEL).all()), k
    # interleaved has no plane stride; reserved is 0
    from broadway_amd import _lib
    hwc = TL.make_desc(INTERLEAVED, "rgb", "float16", "unit", 0, win)
    for k, (d, t) in enumerate([(hwc, _lib.TensorDest(0, item, 0, 1, 0)), (desc, _lib.TensorDest(0, 0, 0, 1, 1))]):
        d_out = torch.full((FRONT + 4 * item,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = _mi().h264mi_tensor_dest_device_pitch(dev.data_ptr(), offs, 3, w, h, cp, C.byref(d), None, 0, C.byref(t),
                                                   d_out.data_ptr() + FRONT, item, None)
        torch.cuda.synchronize()
        assert rc == -1 and bool((d_out == SENTINEL).all()), k


# --------------------------------------------------------- k_tensor_resize ---
def resized_expect(pic, w, h, cp, win, size, how, filt, colour, dtype, consts, interleaved, pad=PAD):
    """The existing oracles' bytes of one resized item: stretched (how None) or
    fitted into the canvas `size`, triangle or bicubic, planar or interleaved."""
    if how is None:
        if filt == BICUBIC:
            p = B.expect(pic, w, h, cp, win, size, "rgb", dtype, consts)
        else:
            p = TL.planar_expect(pic, w, h, cp, win, "rgb", dtype, consts, colour, size)
    elif filt == BICUBIC:
        place = LB.fit(win[2], win[3], size, how)
        p = LB.compose(B.expect(pic, w, h, cp, win, (place[1], place[0]), "rgb", dtype, consts), size, place, 3, dtype,
                       consts, pad)
    else:
        p = LB.expect(pic, w, h, cp, win, size, "rgb", dtype, consts, how, pad, colour)
    return Y.interleave(p, 3, size[0], size[1], dtype) if interleaved else p


def clip_dest(es, planes, rows, cols, interleaved, T_, row_pad):
    """(N, C, T, H, W) -- interleaved: (N, T, H, W, C) -- with every row
    padded by row_pad bytes: (Dest, out_stride)."""
    row = cols * es * (planes if interleaved else 1) + row_pad
    frame = rows * row
    if interleaved:
        return Dest(row, 0, frame, T_), T_ * frame
    return Dest(row, T_ * frame, frame, T_), planes * T_ * frame


def resize_desc(layout, dtype, consts, colour, win, size, how, filt, pad=(0, 0, 0)):
    d = TL.make_desc(layout, "rgb", dtype, consts, colour, win, size, how or "stretch", pad if how else (0, 0, 0))
    d.f.r.filter = filt
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("filt,colour", [(TRIANGLE, 2), (BICUBIC, 0)])
def test_fitted_geometries_as_33_boxes_in_clips_of_3(pictures, filt, colour, layout):
    """k_tensor_resize's table form: tests/test_layout.py's GEOMETRIES (an
    all-bar tile -- the early exit's stores --, content narrower than a tile,
    bars inside one tile), each as 33 boxes in clips of T = 3 with rows padded
    by 16 bytes: the 32-item launch split falls inside clip 10."""
    dtype, consts, es = "float16", "imagenet", 2
    il = layout == INTERLEAVED
    for name, win, size, how, place in TL.GEOMETRIES:
        assert LB.fit(win[2], win[3], size, how) == place
        w, h, cp = PICS[name]
        pics, dev = pictures[name]
        boxes = [(k % 3, win) for k in range(33)]
        shape = (es, 3, size[0], size[1], il)
        dest, out_stride = clip_dest(*shape, 3, 16)
        want = {k: resized_expect(pics[ORDER3[k]], w, h, cp, win, size, how, filt, colour, dtype, consts, il) for k in range(3)}
        desc = resize_desc(layout, dtype, consts, colour, (0, 0, 0, 0), size, how, filt, PAD)
        rc, out, base, total = run(dev, name, ORDER3, 33, shape, dest, out_stride, layout_call(desc, boxes))
        check(rc, out, base, total, [want[k] for k, _ in boxes], dest, out_stride, shape, (win, size))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("filt,colour", [(TRIANGLE, 3), (BICUBIC, 0)])
def test_stretched_boxes_and_windows_in_clips_of_3(pictures, filt, colour, layout):
    """tests/test_layout.py's BOXES repeated to 33, stretched into 7 x 5 (the
    list form without a fit; interleaved: the table form), and six pictures'
    windows stretched into 40 x 70 (one table row per picture), in clips
    of T = 3 with rows padded by one element."""
    dtype, consts, es, name = "float16", "imagenet", 2, "48x32_pitch128"
    il = layout == INTERLEAVED
    w, h, cp = PICS[name]
    pics, dev = pictures[name]
    boxes, size = (TL.BOXES * 9)[:33], (7, 5)
    shape = (es, 3, size[0], size[1], il)
    dest, out_stride = clip_dest(*shape, 3, es)
    want = [resized_expect(pics[ORDER3[k]], w, h, cp, win, size, None, filt, colour, dtype, consts, il) for k, win in boxes]
    desc = resize_desc(layout, dtype, consts, colour, (0, 0, 0, 0), size, None, filt)
    rc, out, base, total = run(dev, name, ORDER3, 33, shape, dest, out_stride, layout_call(desc, boxes))
    check(rc, out, base, total, want, dest, out_stride, shape, "boxes")
    win, size = (6, 2, 38, 26), (40, 70)
    shape = (es, 3, size[0], size[1], il)
    dest, out_stride = clip_dest(*shape, 3, es)
    one = {k: resized_expect(pics[k], w, h, cp, win, size, None, filt, colour, dtype, consts, il) for k in range(3)}
    desc = resize_desc(layout, dtype, consts, colour, win, size, None, filt)
    rc, out, base, total = run(dev, name, ORDER6, 6, shape, dest, out_stride, layout_call(desc))
    check(rc, out, base, total, [one[k] for k in ORDER6], dest, out_stride, shape, "windows")


# ----------------------------------------------------------- k_tensor_warp ---
def turn_q16(deg, cw, ch, ow, oh):
    """The inverse map of a turn by deg about the window's centre, Q16."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    sx, sy = cw / ow, ch / oh
    m = (c * sx, -s * sy, cw / 2 - c * sx * ow / 2 + s * sy * oh / 2, s * sx, c * sy, ch / 2 - s * sx * ow / 2 - c * sy * oh / 2)
    return tuple(int(round(v * 65536)) for v in m)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("border", [W.CONSTANT, W.REPLICATE])
def test_33_warps_in_clips_of_3(pictures, border, layout):
    """k_tensor_warp: the identity, a 30-degree turn and a warp wholly outside
    the window (CONSTANT: the pad tile's early exit), 33 of them into 9 x 6 in
    clips of T = 3 with rows padded by 16 bytes."""
    import test_warp as TW
    dtype, consts, es, name, win, size = "float16", "imagenet", 2, "48x32_pitch128", (6, 2, 38, 26), (6, 9)
    il = layout == INTERLEAVED
    w, h, cp = PICS[name]
    pics, dev = pictures[name]
    mats = [W.IDENTITY, turn_q16(30, win[2], win[3], size[1], size[0]), (65536, 0, 1000 << 16, 0, 65536, 1000 << 16)]
    warps = [(k % 3, mats[(k // 3) % 3]) for k in range(33)]
    pad = PAD if border == W.CONSTANT else (0, 0, 0)
    shape = (es, 3, size[0], size[1], il)
    dest, out_stride = clip_dest(*shape, 3, 16)
    want = {}
    for k, m in warps:
        if (k, m) not in want:
            want[k, m] = W.expect(pics[ORDER3[k]], w, h, cp, win, m, size, "rgb", dtype, consts, 0, border, pad, hwc=il)
    desc = TW.make_desc(size, "rgb", dtype, win, consts, 0, border, pad, layout)

    def call(head, c_dest, d_out, stride, st):
        return _mi().h264mi_tensor_warps_dest_device_pitch(*head, C.byref(desc), TW.make_warps(warps), len(warps), c_dest,
                                                           d_out, stride, st)
    rc, out, base, total = run(dev, name, ORDER3, 33, shape, dest, out_stride, call)
    check(rc, out, base, total, [want[k, m] for k, m in warps], dest, out_stride, shape, border)
    # NULL: the existing call's bytes
    def old(head, c_dest, d_out, stride, st):
        return _mi().h264mi_tensor_warps_device_pitch(*head, C.byref(desc), TW.make_warps(warps), len(warps), d_out, stride, st)
    item = 3 * size[0] * size[1] * es
    rc0, out0, *_ = run(dev, name, ORDER3, 33, shape, None, item + 16, old)
    rc1, out1, base, total = run(dev, name, ORDER3, 33, shape, None, item + 16, call)
    assert rc0 == 0 and rc1 == 0 and same(out1, out0)
    assert same(out1, D.scatter(total, base, [want[k, m] for k, m in warps], None, item + 16, *shape))


# ------------------------------------------------------- through the layers ---
def engine_with_two_pictures():
    """tests/test_layout.py's engine: the smallest case (96 x 64) with its
    first pictures decoded; (engine, streams, slots) of two held slots."""
    from broadway_amd.engine import Capture, Engine
    name = "crop_ltrb_6x4"
    cap = Capture(case_stream(name))
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    slots = [p.cur_slot for p in cap.pictures]
    again = next(k for k in range(1, cap.npics) if slots[k] in slots[:k])
    assert again >= 2
    for k in range(again):
        eng.decode([0], [cap.pictures[k]])
    return eng, slots[:2]


FILL = 7.0      # what the surrounding tensors hold before an export


@pytest.mark.gpu
def test_engine_out_views():
    """Engine.to_tensor(out=view): a channel slice of a wider tensor, a 2 x 4
    tile grid of a canvas (a 5-D view, clip=4) and a permuted clip, each
    torch.equal to the contiguous result with the surrounding elements
    untouched -- for the window, size, fit, rois and warps forms."""
    import torch
    eng, held = engine_with_two_pictures()
    win, size = (6, 2, 86, 52), (20, 50)
    kw = dict(dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD, colour="bt709-full")
    rois = [(1, 6, 2, 86, 52), (0, 0, 0, 96, 64), (0, 2, 2, 2, 2)]
    warps = [(0, W.IDENTITY), (1, turn_q16(30, 86, 52, 50, 20)), (1, W.IDENTITY)]
    forms = {"window": (3, dict(window=win)), "size": (3, dict(window=win, size=size)),
             "fit": (3, dict(window=win, size=size, fit="letterbox", pad=PAD)), "rois": (3, dict(rois=rois, size=size)),
             "warps": (3, dict(warps=warps, window=win, size=size, border="replicate"))}
    for layout in ("nchw", "nhwc"):
        for what, (n, args) in forms.items():
            ss, sl = [0] * n, [held[k % 2] for k in range(n)]
            want = eng.to_tensor(ss, sl, **args, **kw)
            _, p, rows, cols = want.shape
            if layout == "nhwc":
                # (interleaved elements have no plane stride to slice by: the left columns of a wider NHWC tensor)
                x = torch.full((n, rows, cols + 2, 3), FILL, dtype=torch.float16, device="cuda")
                view = x.permute(0, 3, 1, 2)[:, :, :, :cols]
                got = eng.to_tensor(ss, sl, out=view, layout=layout, **args, **kw)
                torch.cuda.synchronize()
                assert got.data_ptr() == x.data_ptr() and torch.equal(got, want), (layout, what)
                assert bool((x[:, :, cols:] == FILL).all()), (layout, what)
                continue
            # channels 1..3 of a five-channel tensor
            x = torch.full((n, 5, rows, cols), FILL, dtype=torch.float16, device="cuda")
            got = eng.to_tensor(ss, sl, out=x[:, 1:4], **args, **kw)
            torch.cuda.synchronize()
            assert got.data_ptr() == x[:, 1:4].data_ptr() and torch.equal(got, want), (layout, what)
            assert bool((x[:, 0] == FILL).all()) and bool((x[:, 4] == FILL).all()), (layout, what)
            # T pictures into clip.permute(1, 0, 2, 3): the item stride below the plane stride
            clip = torch.full((3, n + 1, rows, cols), FILL, dtype=torch.float16, device="cuda")
            got = eng.to_tensor(ss, sl, out=clip[:, :n].permute(1, 0, 2, 3), **args, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got, want) and torch.equal(clip[:, :n], want.permute(1, 0, 2, 3)), what
            assert bool((clip[:, n] == FILL).all()), what
    # eight tiles of a canvas that is one row and two columns larger than the grid
    ss, sl = [0] * 8, [held[k % 2] for k in range(8)]
    tile = (16, 24)
    want = eng.to_tensor(ss, sl, window=win, size=tile, **kw)
    canvas = torch.full((3, 2 * tile[0] + 1, 4 * tile[1] + 2), FILL, dtype=torch.float16, device="cuda")
    grid = canvas[:, :2 * tile[0], :4 * tile[1]].unflatten(2, (4, tile[1])).unflatten(1, (2, tile[0]))   # (3, 2, th, 4, tw)
    view = grid.permute(1, 0, 3, 2, 4)                                                                   # (2, 3, 4, th, tw)
    got = eng.to_tensor(ss, sl, window=win, size=tile, clip=4, out=view, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == canvas.data_ptr()
    for k in range(8):
        r, c = divmod(k, 4)
        assert torch.equal(canvas[:, r * tile[0]:(r + 1) * tile[0], c * tile[1]:(c + 1) * tile[1]], want[k]), k
    assert bool((canvas[:, 2 * tile[0]:] == FILL).all()) and bool((canvas[:, :, 4 * tile[1]:] == FILL).all())
    assert eng.errors() == 0


@pytest.mark.gpu
def test_engine_clips():
    """to_tensor(clip=T) for window, rois= and warps=: (n // T, planes, T,
    rows, cols), contiguous, equal to the 4-D result viewed (B, T, C, h, w) and
    permuted; with layout="nhwc" the same values with channels_last_3d's
    strides; out= a 5-D tensor is filled in place."""
    import torch
    eng, held = engine_with_two_pictures()
    win, size, T_ = (6, 2, 86, 52), (20, 50), 3
    kw = dict(dtype=torch.float16, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD)
    n = 6
    ss, sl = [0] * n, [held[k % 2] for k in (0, 1, 1, 0, 0, 1)]
    rois = [(k % n, 2 * k, 2 * k, 40 + 2 * k, 30) for k in range(6)]
    warps = [(k % n, turn_q16(10 * k, 86, 52, 50, 20)) for k in range(6)]
    forms = {"window": dict(window=win), "rois": dict(rois=rois, size=size),
             "warps": dict(warps=warps, window=win, size=size)}
    for what, args in forms.items():
        flat = eng.to_tensor(ss, sl, **args, **kw)
        _, p, rows, cols = flat.shape
        want = flat.view(n // T_, T_, p, rows, cols).permute(0, 2, 1, 3, 4)
        got = eng.to_tensor(ss, sl, clip=T_, **args, **kw)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (n // T_, p, T_, rows, cols) and got.is_contiguous() and torch.equal(got, want), what
        last = eng.to_tensor(ss, sl, clip=T_, layout="nhwc", **args, **kw)
        torch.cuda.synchronize()
        like = torch.empty(got.shape, dtype=got.dtype, device="cuda").contiguous(memory_format=torch.channels_last_3d)
        assert last.stride() == like.stride() and last.is_contiguous(memory_format=torch.channels_last_3d), what
        assert torch.equal(last, want), what
        out = torch.full((n // T_ + 1, p, T_, rows, cols), FILL, dtype=torch.float16, device="cuda")
        assert eng.to_tensor(ss, sl, clip=T_, out=out[:n // T_], **args, **kw).data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert torch.equal(out[:n // T_], want) and bool((out[n // T_] == FILL).all()), what
    with pytest.raises(ValueError):
        eng.to_tensor(ss, sl, window=win, clip=4, **kw)         # 6 items are no multiple of 4
    with pytest.raises(ValueError):
        eng.to_tensor(ss, sl, window=win, clip=0, **kw)
    assert eng.errors() == 0


@pytest.mark.gpu
def test_engine_refuses_views_it_cannot_express():
    """A column stride of 2, an expanded dimension and a dtype mismatch: each
    a ValueError before the library is called (nothing is written)."""
    import torch
    eng, held = engine_with_two_pictures()
    win = (6, 2, 86, 52)
    ss, sl = [0, 0], held
    wide = torch.full((2, 3, 52, 172), FILL, dtype=torch.float16, device="cuda")
    one = torch.full((1, 3, 52, 86), FILL, dtype=torch.float16, device="cuda")
    other = torch.full((2, 3, 52, 86), FILL, dtype=torch.float32, device="cuda")[:, :, :, :]
    for what, bad in (("column stride", wide[:, :, :, ::2]), ("item stride", one.expand(2, 3, 52, 86)), ("float32", other)):
        with pytest.raises(ValueError, match=what):
            eng.to_tensor(ss, sl, window=win, dtype=torch.float16, out=bad)
    torch.cuda.synchronize()
    assert bool((wide == FILL).all()) and bool((one == FILL).all()) and bool((other == FILL).all())


def decode_tensors(nals, options, on_clip=None):
    """The (tensor, width, height) of every onPictureDecoded under `options`,
    the clips of onClipDecoded, and the decoder's clip_fill at the end."""
    pics, clips = [], []
    dec = Decoder(options)
    dec.onPictureDecoded = lambda buf, w, h, infos: pics.append((buf, w, h))
    dec.onClipDecoded = lambda clip, w, h: clips.append((clip, w, h))
    for nal in nals:
        dec.decode(nal)
    fill = dec.clip_fill
    dec.close()
    return pics, clips, fill


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_decoder_clips(layout):
    """Decoder({"tensor": {"clip": 3, "step": s}}), s = 1 and 2, on a stream of
    tests/_crop.py's cases cut to a picture count that leaves a remainder: every
    clip equals torch.stack of the matching pictures of a plain ``tensor`` run
    along dimension 1, the per-picture views alias their clip, and clip_fill at
    the end is the remainder."""
    import torch
    nals = split_annexb(case_stream("cfg1_plumbing_640x368"))[:-2]
    opts = {"dtype": torch.float16, "mean": T.IMAGENET_MEAN, "std": T.IMAGENET_STD, "size": (24, 40), "fit": "letterbox",
            "pad": PAD, "layout": layout}
    plain, none, fill = decode_tensors(nals, {"tensor": opts})
    P, T_ = len(plain), 3
    assert P >= 2 * T_ + 1 and not none and fill == 0
    for step in (1, 2):
        pics, clips, fill = decode_tensors(nals, {"tensor": dict(opts, clip=T_, step=step)})
        torch.cuda.synchronize()
        kept = list(range(0, P, step))
        assert len(pics) == len(kept) and len(clips) == len(kept) // T_ and fill == len(kept) % T_, step
        assert step == 2 or fill, "the cut leaves an incomplete clip"
        for c, (clip, w, h) in enumerate(clips):
            assert (w, h) == (40, 24) and tuple(clip.shape) == (3, T_, 24, 40), (step, c)
            if layout == "nchw":
                assert clip.is_contiguous(), (step, c)
            else:
                assert clip.permute(1, 2, 3, 0).is_contiguous(), (step, c)
            want = torch.stack([plain[kept[c * T_ + t]][0] for t in range(T_)], dim=1)
            assert torch.equal(clip, want), (step, c)
            for t in range(T_):
                view = pics[c * T_ + t][0]
                assert view.data_ptr() == clip[:, t].data_ptr() and view.stride() == clip[:, t].stride(), (step, c, t)
        for k in range(len(clips) * T_, len(kept)):           # the incomplete clip's pictures were still delivered
            assert torch.equal(pics[k][0], plain[kept[k]][0]), (step, k)
