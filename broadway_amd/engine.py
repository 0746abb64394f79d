"""Batched multi-stream reconstruction on one MI355X (the throughput path).

``Capture`` runs the product host parser over a whole stream and keeps each
picture's MB-record batch (include/h264mi_records.h).  ``Engine`` owns the
HBM frame slots of S streams and reconstructs one picture of each stream per
launch pair (k_prep: deblocking records + residuals; k_wgpp: MC, intra and the
deblocking row chain).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

MBREC_BYTES = 96
PICDESC_BYTES = 32


def tensor_affine(mean: Sequence[float], std: Sequence[float]) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """(scale, bias) of ``(c / 255 - mean) / std`` for 8-bit samples c: mean
    and std are per-plane triples in 0..1 units; scale = 1 / (255 * std) and
    bias = -mean / std, computed in float64 and rounded once to fp32 (the
    values the kernel's fused multiply-add takes)."""
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std are triples")
    scale = tuple(float(np.float32(1.0 / (255.0 * s))) for s in std)
    bias = tuple(float(np.float32(-m / s)) for m, s in zip(mean, std))
    return scale, bias


def tensor_colour_bits(colour, unspecified=None, mode="rgb", stream_ok=False):
    """Bits 8..13 of a tensor descriptor's mode for the colour set ``colour``
    (a key of ``_lib.TENSOR_COLOURS``; None is "reference").  "stream" -- the
    set the delivered picture's VUI names, ``unspecified`` ("bt601", the
    default, "bt709" or "size") where it names none -- belongs to the Decoder
    (``stream_ok``); a colour goes with ``mode="rgb"`` only.  ValueError
    otherwise."""
    if colour is None and unspecified is None:
        return 0
    if mode != "rgb":
        raise ValueError(f"colour / unspecified: mode {mode!r} has no colour set (only 'rgb')")
    colour = "reference" if colour is None else colour
    if not isinstance(colour, str) or colour not in _lib.TENSOR_COLOURS:
        raise ValueError(f"colour {colour!r}: one of {sorted(_lib.TENSOR_COLOURS)}")
    if colour != "stream":
        if unspecified is not None:
            raise ValueError("unspecified: goes with colour='stream'")
        return _lib.TENSOR_COLOURS[colour] << _lib.TENSOR_COLOUR_SHIFT
    if not stream_ok:
        raise ValueError("colour 'stream': the Decoder's tensor option only (an engine knows no stream)")
    unspecified = "bt601" if unspecified is None else unspecified
    if not isinstance(unspecified, str) or unspecified not in _lib.TENSOR_UNSPECIFIED:
        raise ValueError(f"unspecified {unspecified!r}: one of {sorted(_lib.TENSOR_UNSPECIFIED)}")
    return (_lib.TENSOR_COLOUR_STREAM << _lib.TENSOR_COLOUR_SHIFT |
            _lib.TENSOR_UNSPECIFIED[unspecified] << _lib.TENSOR_UNSPEC_SHIFT)


def _resize_size(size):
    """(oh, ow) of a resized export's ``size``, each 1..16384."""
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size {size!r}: (oh, ow)") from None
    if not (1 <= oh <= _lib.RESIZE_MAX_DIM and 1 <= ow <= _lib.RESIZE_MAX_DIM):
        raise ValueError(f"size {size!r}: oh and ow are 1..{_lib.RESIZE_MAX_DIM}")
    return oh, ow


def resize_filter(filter, size=True, what="filter") -> int:
    """The ``h264mi_tensor_resize_desc.filter`` of ``filter``: None or
    "triangle" (the antialiased triangle, torch's ``bilinear, antialias=True``)
    or "bicubic" (Keys, a = -0.5, antialiased: PIL's BICUBIC, torch's ``bicubic,
    antialias=True``).  A filter goes with a ``size`` (``size``
    None or False: ValueError unless ``filter`` is None); ValueError for
    anything else."""
    if filter is None:
        return _lib.RESIZE_TRIANGLE
    if not isinstance(filter, str) or filter not in _lib.RESIZE_FILTERS:
        raise ValueError(f"{what} {filter!r}: one of {sorted(_lib.RESIZE_FILTERS)}")
    if size is None or size is False:
        raise ValueError(f"{what}: goes with size=(oh, ow)")
    return _lib.RESIZE_FILTERS[filter]


def _no_filter(filter, what):
    """The exports that have one filter only: ValueError for a ``filter``."""
    if filter is not None:
        raise ValueError(f"filter: {what} (only size=, rois= and fit= of to_tensor take one)")


def _field_resized(resized, built, size):
    """A field descriptor triple ``built`` with its descriptor wrapped into the
    resize descriptor ``resized`` (``f``, then ow, oh and the filter) of
    ``size`` = (oh, ow); ``size`` None: ``built`` as it is."""
    if size is None:
        return built
    oh, ow = _resize_size(size)
    f, n, dtype = built
    d = resized()
    d.f, d.ow, d.oh, d.filter = f, ow, oh, _lib.RESIZE_TRIANGLE
    return d, n, dtype


def tensor_layout(layout) -> int:
    """The ``h264mi_tensor_layout_desc.layout`` of ``layout``: "nchw" (planar,
    the default everywhere) or "nhwc" (interleaved: torch's channels_last).
    ValueError for anything else."""
    if not isinstance(layout, str) or layout not in _lib.TENSOR_LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {sorted(_lib.TENSOR_LAYOUTS)}")
    return _lib.TENSOR_LAYOUTS[layout]


def layout_desc(desc, layout):
    """The ``_lib.TensorLayoutDesc`` of a pixel export's descriptor -- a
    ``_lib.TensorDesc`` (no size: the unresized export), ``TensorResizeDesc``
    (a stretch) or ``TensorFitDesc`` -- under ``layout`` (``tensor_layout``)."""
    d = _lib.TensorLayoutDesc()
    d.layout = tensor_layout(layout)
    if isinstance(desc, _lib.TensorFitDesc):
        d.f = desc
    elif isinstance(desc, _lib.TensorResizeDesc):
        d.f.r = desc
    elif isinstance(desc, _lib.TensorDesc):
        d.f.r.t = desc
    else:
        raise ValueError(f"layout_desc: {type(desc).__name__} is no pixel export's descriptor")
    return d


def empty_layout(shape, dtype, device, layout="nchw"):
    """A new tensor of the logical ``shape`` = (n, planes, rows, cols), or
    (planes, rows, cols), in the memory order of ``layout``: "nhwc" is
    ``torch.empty((n, rows, cols, planes)).permute(0, 3, 1, 2)`` -- the usual
    shape with channels-last strides."""
    import torch
    if not tensor_layout(layout):
        return torch.empty(shape, dtype=dtype, device=device)
    if len(shape) == 3:
        return torch.empty((shape[1], shape[2], shape[0]), dtype=dtype, device=device).permute(2, 0, 1)
    return torch.empty((shape[0], shape[2], shape[3], shape[1]), dtype=dtype, device=device).permute(0, 3, 1, 2)


def check_out(out, shape, dtype, device, layout="nchw"):
    """``out=`` of an export against the result's logical ``shape`` = (n,
    planes, rows, cols), dtype, device and ``layout``: "nchw" asks for a
    contiguous tensor, "nhwc" for one whose ``permute(0, 2, 3, 1)`` is
    contiguous.  ValueError otherwise, before the library is called."""
    dense = out.permute(0, 2, 3, 1) if tensor_layout(layout) and out.dim() == 4 else out
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not dense.is_contiguous():
        raise ValueError(f"out: a {dtype} tensor of shape {tuple(shape)} on {device}, {layout!r}-contiguous "
                         f"(got {out.dtype} {tuple(out.shape)} with strides {tuple(out.stride())} on {out.device})")


def empty_clip(shape, dtype, device, layout="nchw"):
    """A new tensor of the logical ``shape`` = (b, planes, t, rows, cols) for
    ``to_tensor(clip=t)``: contiguous NCTHW, or with "nhwc"
    ``torch.empty((b, t, rows, cols, planes)).permute(0, 4, 1, 2, 3)`` -- the
    strides of ``torch.channels_last_3d``."""
    import torch
    if not tensor_layout(layout):
        return torch.empty(shape, dtype=dtype, device=device)
    b, p, t, rows, cols = shape
    return torch.empty((b, t, rows, cols, p), dtype=dtype, device=device).permute(0, 4, 1, 2, 3)


def dest_of_view(out, shape, dtype, device, layout="nchw"):
    """(``_lib.TensorDest``, out_stride in bytes) of ``out=``, any view of the
    result's logical ``shape`` -- (n, planes, rows, cols), or (b, planes, t,
    rows, cols) of ``clip=t`` -- whose strides the exports can write through
    (h264mi_tensor_dest): the column stride is 1 ("nhwc": the
    plane stride 1 and the column stride ``planes``), every other stride is
    free as long as no two elements share an address -- a slice of a wider
    tensor, a tile of a canvas, a permuted clip.  ValueError, naming the
    stride, for anything else, before the library is called.  A dimension of
    one element has no stride to speak of."""
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError(f"out: a {dtype} view of shape {tuple(shape)} on {device} "
                         f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    es = out.element_size()
    st = tuple(out.stride())
    if len(shape) == 5:
        (n, planes, clip, rows, cols), (s_n, s_p, s_t, s_r, s_c) = shape, st
    else:
        (n, planes, rows, cols), (s_n, s_p, s_r, s_c), clip, s_t = shape, st, 1, 0
    nhwc = tensor_layout(layout) != 0 and planes > 1
    names = {"column": s_c, "row": s_r, "plane": s_p, "frame": s_t, "item": s_n}
    if nhwc and (s_p != 1 or (cols > 1 and s_c != planes)):
        raise ValueError(f"out: layout 'nhwc' writes the planes of a column side by side: plane stride 1 and column "
                         f"stride {planes} (got plane stride {s_p}, column stride {s_c})")
    if not nhwc and cols > 1 and s_c != 1:
        raise ValueError(f"out: column stride {s_c}: the elements of a row are written side by side (stride 1)")
    packed = cols * (planes if nhwc else 1)
    # the levels above a row's elements that hold more than one element, by stride
    levels = [(s_r, rows, "row")] + ([] if nhwc else [(s_p, planes, "plane")]) + [(s_t, clip, "frame"), (s_n, n, "item")]
    span = packed
    for stride, count, name in sorted((l for l in levels if l[1] > 1), key=lambda l: l[0]):
        if stride < span:
            raise ValueError(f"out: {name} stride {stride} (dimension of {count}): below the {span} elements it has to "
                             f"step over -- elements would share an address (strides {names})")
        span += (count - 1) * stride
    d = _lib.TensorDest()
    d.row = s_r * es if rows > 1 else 0
    d.plane = s_p * es if planes > 1 and not nhwc else 0
    d.frame = s_t * es if clip > 1 else 0
    d.clip = clip
    return d, (s_n * es if n > 1 else 0)


def tensor_desc(window, mode="rgb", dtype=None, scale=None, bias=None, mean=None, std=None, size=None, colour=None,
                unspecified=None, stream_ok=False, layout=None, filter=None):
    """(``_lib.TensorDesc``, planes, torch dtype) of a tensor export
    (Engine.to_tensor, Decoder's ``tensor`` option); window = (x, y, cw, ch),
    or None for the decoder's SPS crop window (cw = 0 in the descriptor).
    With ``size`` = (oh, ow), each 1..16384, the descriptor is a
    ``_lib.TensorResizeDesc`` of the resized export (its ``t`` is the one
    above).  ``colour``: the colour set of the R, G, B samples
    (``tensor_colour_bits``; None: the reference's BT.601 limited range).
    ``layout`` "nchw" or "nhwc" (not None): the descriptor is the
    ``_lib.TensorLayoutDesc`` (``layout_desc``) of the one above.  ``filter``
    (with ``size`` only): "triangle", the default, or "bicubic"
    (``resize_filter``; a window at most 16 times the output on each axis)."""
    import torch
    if layout is not None:
        tensor_layout(layout)
        d, planes, dtype = tensor_desc(window, mode, dtype, scale, bias, mean, std, size, colour, unspecified, stream_ok,
                                       filter=filter)
        return layout_desc(d, layout), planes, dtype
    filt = resize_filter(filter, size)
    if size is not None:
        oh, ow = _resize_size(size)
        t, planes, dtype = tensor_desc(window, mode, dtype, scale, bias, mean, std, None, colour, unspecified, stream_ok)
        d = _lib.TensorResizeDesc()
        d.t, d.ow, d.oh, d.filter = t, ow, oh, filt
        return d, planes, dtype
    dtype = torch.float16 if dtype is None else dtype
    dts = {torch.uint8: _lib.TENSOR_U8, torch.float16: _lib.TENSOR_F16, torch.bfloat16: _lib.TENSOR_BF16,
           torch.float32: _lib.TENSOR_F32}
    modes = {"rgb": (_lib.TENSOR_RGB, 3), "gray": (_lib.TENSOR_GRAY, 1)}
    if dtype not in dts:
        raise ValueError(f"dtype {dtype}: one of torch.uint8, float16, bfloat16, float32")
    if mode not in modes:
        raise ValueError(f"mode {mode!r}: 'rgb' or 'gray'")
    colour_bits = tensor_colour_bits(colour, unspecified, mode, stream_ok)
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is not None:
        if scale is not None or bias is not None:
            raise ValueError("mean / std or scale / bias, not both")
        scale, bias = tensor_affine(mean, std)

    def triple(v, default):
        if v is None:
            return (default,) * 3
        v = tuple(float(f) for f in v) if hasattr(v, "__len__") else (float(v),) * 3
        if len(v) != 3:
            raise ValueError("scale and bias are scalars or triples")
        return v

    d = _lib.TensorDesc()
    d.x, d.y, d.cw, d.ch = (int(v) for v in window) if window is not None else (0, 0, 0, 0)
    d.mode, planes = modes[mode]
    d.mode |= colour_bits
    d.dtype = dts[dtype]
    d.scale[:] = triple(scale, 1.0 / 255.0)
    d.bias[:] = triple(bias, 0.0)
    return d, planes, dtype


def letterbox_fit(cw: int, ch: int, size, fit: str = "letterbox"):
    """``(rw, rh, px, py)``: the content size and position of a cw x ch window
    fitted into the canvas ``size`` = (oh, ow) with its aspect ratio kept --
    ``h264mi_letterbox_fit``'s arithmetic (include/h264mi.h) in Python
    integers.  The major axis fills the canvas, the minor axis is the nearest
    integer (halves up) but at least ceil(n / 32) and 1; "letterbox" centres
    the content (floored), "topleft" puts it at (0, 0), "stretch" is (ow, oh,
    0, 0)."""
    oh, ow = _resize_size(size)
    if fit not in _lib.TENSOR_FIT:
        raise ValueError(f"fit {fit!r}: one of {sorted(_lib.TENSOR_FIT)}")
    try:
        given, (cw, ch) = (cw, ch), (int(cw), int(ch))
        if (cw, ch) != given or not (1 <= cw <= _lib.RESIZE_MAX_DIM and 1 <= ch <= _lib.RESIZE_MAX_DIM):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"window size {(cw, ch)!r}: integers 1..{_lib.RESIZE_MAX_DIM}") from None
    rw, rh = ow, oh
    if fit != "stretch":
        if cw * oh >= ch * ow:
            rh = max((2 * ch * ow + cw) // (2 * cw), (ch + 31) // 32, 1)
        else:
            rw = max((2 * cw * oh + ch) // (2 * ch), (cw + 31) // 32, 1)
    if fit == "letterbox":
        return rw, rh, (ow - rw) // 2, (oh - rh) // 2
    return rw, rh, 0, 0


def unletterbox(boxes, window, size, fit: str = "letterbox"):
    """A detector's corner boxes ``(k, x0, y0, x1, y1)`` (floats) in the
    coordinates of a canvas ``size`` = (oh, ow) that holds ``window`` = (x, y,
    cw, ch) fitted by ``fit``, back in picture coordinates: minus the content's
    position, times cw / rw and ch / rh, plus the window's origin.  The result
    is in ``snap_rois``' format (it clips, so a box that reaches into the bars
    needs nothing more)."""
    x, y, cw, ch = window
    rw, rh, px, py = letterbox_fit(cw, ch, size, fit)
    sx, sy = cw / rw, ch / rh
    return [(k, x + (x0 - px) * sx, y + (y0 - py) * sy, x + (x1 - px) * sx, y + (y1 - py) * sy)
            for k, x0, y0, x1, y1 in boxes]


def fit_desc(desc, planes, fit="letterbox", pad=114, layout=None):
    """The ``_lib.TensorFitDesc`` of the resize descriptor ``desc`` letterboxed
    (Engine.to_tensor(fit=), the Decoder's ``tensor`` option, Decoder.rois):
    ``fit`` "letterbox", "topleft" or "stretch"; ``pad`` one uint8 sample for
    every plane or one per plane, in the tensor's own domain (R, G, B or
    luma).  With ``layout`` (not None): its ``_lib.TensorLayoutDesc``.
    ValueError for anything else."""
    if layout is not None:
        tensor_layout(layout)
        return layout_desc(fit_desc(desc, planes, fit, pad), layout)
    if fit not in _lib.TENSOR_FIT:
        raise ValueError(f"fit {fit!r}: one of {sorted(_lib.TENSOR_FIT)}")
    try:
        given = tuple(pad) if hasattr(pad, "__len__") else (pad,) * planes
        samples = tuple(int(v) for v in given)
        if len(samples) != planes or samples != given or any(isinstance(v, bool) for v in given) or \
                not all(0 <= v <= 255 for v in samples):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"pad {pad!r}: an integer 0..255, or {planes} of them (one per plane)") from None
    d = _lib.TensorFitDesc()
    d.r, d.fit = desc, _lib.TENSOR_FIT[fit]
    d.pad[:] = samples + (0,) * (4 - planes)
    return d


def snap_rois(boxes, width: int, height: int):
    """Corner boxes ``(k, x0, y0, x1, y1)`` (floats or ints, as detectors emit
    them; k indexes a picture list) as the ``(k, x, y, cw, ch)`` boxes of
    ``Engine.to_tensor(rois=)`` on pictures of width x height: each box is
    rounded outward to even coordinates and clipped to the picture, and a box
    that is empty after clipping is dropped.  Returns ``(rois, kept)``, kept[i]
    being the index in ``boxes`` of rois[i]."""
    import math
    width, height = int(width) & ~1, int(height) & ~1
    rois, kept = [], []
    for i, (k, x0, y0, x1, y1) in enumerate(boxes):
        x0, y0 = max(2 * math.floor(x0 / 2), 0), max(2 * math.floor(y0 / 2), 0)
        x1, y1 = min(2 * math.ceil(x1 / 2), width), min(2 * math.ceil(y1 / 2), height)
        if x1 > x0 and y1 > y0:
            rois.append((int(k), x0, y0, x1 - x0, y1 - y0))
            kept.append(i)
    return rois, kept


def rois_desc(rois, size, npics, width, height, mode="rgb", dtype=None, scale=None, bias=None, mean=None, std=None,
              colour=None, unspecified=None, stream_ok=False, fit=None, pad=None, layout=None, filter=None):
    """(``_lib.TensorResizeDesc`` with a zero window, ``_lib.Roi`` array, planes,
    torch dtype) of a region-of-interest export (Engine.to_tensor(rois=),
    Decoder.rois): ``rois`` = [(k, x, y, cw, ch), ...] over ``npics`` pictures
    of width x height, every box to ``size`` = (oh, ow).  The rules of
    include/h264mi.h: a non-empty list, k in [0, npics), every box even,
    inside the picture, at most 16384 a side and 32 source samples per output
    and axis.  With ``fit`` (or ``pad``) the descriptor is the
    ``_lib.TensorFitDesc`` of the letterboxed export (``fit_desc``): every box
    gets its own fit into ``size``, and the 32 samples per output are judged
    against its content size.  With ``layout`` (not None) the descriptor is
    the ``_lib.TensorLayoutDesc`` of that one.  ``filter`` "triangle" (default)
    or "bicubic": the 32 samples per output are 16 under "bicubic".  ValueError
    otherwise."""
    if layout is not None:
        tensor_layout(layout)
        desc, arr, planes, dtype = rois_desc(rois, size, npics, width, height, mode, dtype, scale, bias, mean, std,
                                             colour, unspecified, stream_ok, fit, pad, filter=filter)
        return layout_desc(desc, layout), arr, planes, dtype
    if size is None:
        raise ValueError("rois: goes with size=(oh, ow)")
    desc, planes, dtype = tensor_desc((0, 0, 0, 0), mode, dtype, scale, bias, mean, std, size, colour, unspecified,
                                      stream_ok, filter=filter)
    oh, ow, ratio = desc.oh, desc.ow, _lib.RESIZE_MAX_RATIO[desc.filter]
    if fit is not None or pad is not None:
        fit = "letterbox" if fit is None else fit
        desc = fit_desc(desc, planes, fit, 114 if pad is None else pad)
    try:
        given = [tuple(b) for b in rois]
        boxes = [tuple(int(v) for v in b) for b in given]
        if any(len(b) != 5 for b in boxes) or boxes != given:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"rois {rois!r}: a list of (k, x, y, cw, ch) integers") from None
    if not boxes:
        raise ValueError("rois: an empty list")
    for k, x, y, cw, ch in boxes:
        if not 0 <= k < npics:
            raise ValueError(f"rois: box {(k, x, y, cw, ch)}: picture {k} of {npics}")
        if (x | y | cw | ch) & 1 or x < 0 or y < 0 or cw < 2 or ch < 2 or cw > width - x or ch > height - y:
            raise ValueError(f"rois: box {(k, x, y, cw, ch)}: even and inside {width} x {height}")
        if cw > _lib.RESIZE_MAX_DIM or ch > _lib.RESIZE_MAX_DIM:
            raise ValueError(f"rois: box {(k, x, y, cw, ch)}: at most {_lib.RESIZE_MAX_DIM} a side")
        rw, rh = (ow, oh) if fit is None else letterbox_fit(cw, ch, (oh, ow), fit)[:2]
        if cw > ratio * rw or ch > ratio * rh or rw > ow or rh > oh:
            raise ValueError(f"rois: box {(k, x, y, cw, ch)}: at most {ratio} times the size {(rh, rw)} on each axis")
    arr = (_lib.Roi * len(boxes))(*[_lib.Roi(*b) for b in boxes])
    return desc, arr, planes, dtype


def _q16(v, what):
    """floor(v * 65536 + 0.5) of a coefficient; ValueError where it leaves int32."""
    import math
    v = float(v)
    q = math.floor(v * 65536.0 + 0.5) if math.isfinite(v) else None
    if q is None or not -2 ** 31 <= q < 2 ** 31:
        raise ValueError(f"{what}: coefficient {v!r} does not fit Q16 in int32")
    return int(q)


def warp_q16(M, forward=True):
    """The six Q16 coefficients ``(m0, ..., m5)`` of ``Engine.to_tensor(warps=)``
    from a float 2x3 matrix in cv2's convention (integer coordinates are
    sample centres, of the window and of the output alike).  ``forward``
    (cv2.warpAffine's default): ``M`` maps a window position to an output
    position and is inverted here; ``forward=False``: ``M`` maps an output
    position to a window position already (cv2's WARP_INVERSE_MAP), which is
    what the export takes.  Each coefficient is ``floor(v * 65536 + 0.5)``;
    ValueError for a singular forward matrix, a bad shape, or a coefficient
    outside int32."""
    try:
        (a, b, c), (d, e, f) = [[float(v) for v in row] for row in M]
    except (TypeError, ValueError):
        raise ValueError(f"warp_q16: {M!r}: a 2x3 matrix") from None
    if forward:
        det = a * e - b * d
        if det == 0.0 or det != det:
            raise ValueError(f"warp_q16: {M!r} is singular")
        a, b, c, d, e, f = e / det, -b / det, (b * f - c * e) / det, -d / det, a / det, (c * d - a * f) / det
    return tuple(_q16(v, "warp_q16") for v in (a, b, c, d, e, f))


def rotated_box_warp(cx, cy, bw, bh, angle_deg, size):
    """The six Q16 coefficients that turn a rotated box upright: the box of
    bw x bh centred at (cx, cy), rotated counter-clockwise (as seen, y down) by
    ``angle_deg`` about its centre, in continuous coordinates of the window
    (sample k covers [k, k + 1)), sampled to ``size`` = (oh, ow).  Output (i,
    j) samples ``(cx, cy) + R(angle) ((j + 0.5) bw / ow - bw / 2, (i + 0.5) bh
    / oh - bh / 2) - (0.5, 0.5)`` with R = [[cos, sin], [-sin, cos]].  Angle 0
    with the box equal to the window and ``size == (ch, cw)`` is the identity,
    and quarter turns use exact cosines.  ValueError as for ``warp_q16``."""
    import math
    oh, ow = _resize_size(size)
    cx, cy, bw, bh, angle = (float(v) for v in (cx, cy, bw, bh, angle_deg))
    quarter = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    c, s = quarter.get(angle % 360.0) or (math.cos(math.radians(angle)), math.sin(math.radians(angle)))
    sx, sy = bw / ow, bh / oh
    u0, v0 = 0.5 * sx - 0.5 * bw, 0.5 * sy - 0.5 * bh
    M = ((c * sx, s * sy, cx - 0.5 + c * u0 + s * v0), (-s * sx, c * sy, cy - 0.5 - s * u0 + c * v0))
    return tuple(_q16(v, "rotated_box_warp") for row in M for v in row)


def warps_desc(warps, size, npics, window, width, height, mode="rgb", dtype=None, scale=None, bias=None, mean=None,
               std=None, colour=None, unspecified=None, stream_ok=False, border=None, pad=None, layout=None):
    """(``_lib.TensorWarpDesc``, ``_lib.Warp`` array, planes, torch dtype) of an
    affine-warped export (Engine.to_tensor(warps=), Decoder.warps): ``warps`` =
    [(k, (m0, ..., m5)), ...] over ``npics`` pictures of width x height (0: not
    known yet, so the window is not judged against it), every warp to ``size``
    = (oh, ow) from ``window`` = (x, y, cw, ch), the window the taps are
    confined to (None: cw = 0, the Decoder's crop window).  The coefficients
    are Q16 integers (``warp_q16``, ``rotated_box_warp``), any int32.
    ``border`` "constant" (the default: a tap outside the window is the sample
    ``pad``, default 0; one value or one per plane) or "replicate" (the
    window's edge; no ``pad``).  ``layout`` "nchw" (default) or "nhwc".
    ValueError for anything the library would refuse."""
    if size is None:
        raise ValueError("warps: goes with size=(oh, ow)")
    t, planes, dtype = tensor_desc(window, mode, dtype, scale, bias, mean, std, None, colour, unspecified, stream_ok)
    oh, ow = _resize_size(size)
    border = "constant" if border is None else border
    if not isinstance(border, str) or border not in _lib.WARP_BORDERS:
        raise ValueError(f"border {border!r}: one of {sorted(_lib.WARP_BORDERS)}")
    if border == "replicate" and pad is not None:
        raise ValueError("pad: goes with border='constant' (replicate repeats the window's edge)")
    d = _lib.TensorWarpDesc()
    d.t, d.ow, d.oh, d.filter, d.border = t, ow, oh, _lib.WARP_BILINEAR, _lib.WARP_BORDERS[border]
    d.pad[:] = fit_desc(_lib.TensorResizeDesc(), planes, "stretch", 0 if pad is None else pad).pad[:]
    d.layout = tensor_layout("nchw" if layout is None else layout)
    if window is not None:
        x, y, cw, ch = (t.x, t.y, t.cw, t.ch)
        if (x | y | cw | ch) & 1 or x < 0 or y < 0 or cw < 2 or ch < 2 or cw > _lib.RESIZE_MAX_DIM or \
                ch > _lib.RESIZE_MAX_DIM or (width and (cw > width - x or ch > height - y)):
            raise ValueError(f"warps: window {(x, y, cw, ch)}: even, at most {_lib.RESIZE_MAX_DIM} a side and inside "
                             f"{width} x {height}")
    try:
        given = [(k, tuple(m)) for k, m in warps]
        mats = [(int(k), tuple(int(v) for v in m)) for k, m in given]
        if any(len(m) != 6 for _, m in mats) or mats != given or \
                any(isinstance(v, bool) for k, m in given for v in (k,) + m):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"warps {warps!r}: a list of (k, (m0, m1, m2, m3, m4, m5)) integers") from None
    if not mats:
        raise ValueError("warps: an empty list")
    for k, m in mats:
        if not 0 <= k < npics:
            raise ValueError(f"warps: {(k, m)}: picture {k} of {npics}")
        if not all(-2 ** 31 <= v < 2 ** 31 for v in m):
            raise ValueError(f"warps: {(k, m)}: the coefficients are int32 (Q16)")
    arr = (_lib.Warp * len(mats))(*[_lib.Warp(k, (C.c_int * 6)(*m)) for k, m in mats])
    return d, arr, planes, dtype


def stats_desc(planes="y", window=None, rois=None, hist=False, colour=None, npics=1, width=None, height=None,
               stream_ok=False):
    """(``_lib.StatsDesc``, ``_lib.Roi`` array or None, P, L) of a statistics
    export (Engine.to_stats, Decoder.stats): ``planes`` "y", "yuv" or "rgb";
    ``window`` = (x, y, cw, ch) or ``rois`` = [(k, x, y, cw, ch), ...] over
    ``npics`` pictures of width x height (None: sizes are not judged here) --
    never both; ``window`` None without boxes leaves the descriptor's window
    zero (the Decoder: the whole delivered picture).  ``hist``: the 256 bins
    behind the 8 words.  ``colour``: a key of ``_lib.TENSOR_COLOURS``, with
    "rgb" only; "stream" belongs to the Decoder (``stream_ok``).  P plane
    records of L int64 words per item.  The rules of include/h264mi.h: every
    window even and inside the picture, a non-empty box list, k in [0, npics).
    ValueError otherwise."""
    if not isinstance(planes, str) or planes not in _lib.STATS_PLANES:
        raise ValueError(f"planes {planes!r}: one of {sorted(_lib.STATS_PLANES)}")
    d = _lib.StatsDesc()
    d.planes = _lib.STATS_PLANES[planes]
    d.flags = _lib.STATS_HIST if hist else 0
    if colour is not None:
        if planes != "rgb":
            raise ValueError(f"colour: planes {planes!r} has no colour set (only 'rgb')")
        if not isinstance(colour, str) or colour not in _lib.TENSOR_COLOURS:
            raise ValueError(f"colour {colour!r}: one of {sorted(_lib.TENSOR_COLOURS)}")
        if colour == "stream" and not stream_ok:
            raise ValueError("colour 'stream': Decoder.stats only (an engine knows no stream)")
        d.colour = _lib.TENSOR_COLOURS[colour]

    def box(b, what):
        x, y, cw, ch = b
        if (x | y | cw | ch) & 1 or x < 0 or y < 0 or cw < 2 or ch < 2 or \
                (width is not None and cw > width - x) or (height is not None and ch > height - y):
            raise ValueError(f"{what} {tuple(b)}: even and inside {width} x {height}")

    arr = None
    if rois is not None:
        if window is not None:
            raise ValueError("rois: goes without a window (every box is its own)")
        try:
            given = [tuple(b) for b in rois]
            boxes = [tuple(int(v) for v in b) for b in given]
            if any(len(b) != 5 for b in boxes) or boxes != given:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"rois {rois!r}: a list of (k, x, y, cw, ch) integers") from None
        if not boxes:
            raise ValueError("rois: an empty list")
        for b in boxes:
            if not 0 <= b[0] < npics:
                raise ValueError(f"rois: box {b}: picture {b[0]} of {npics}")
            box(b[1:], "rois: box")
        arr = (_lib.Roi * len(boxes))(*[_lib.Roi(*b) for b in boxes])
    elif window is not None:
        try:
            given = tuple(window)
            win = tuple(int(v) for v in given)
            if len(win) != 4 or win != given:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"window {window!r}: (x, y, cw, ch) integers") from None
        box(win, "window")
        d.x, d.y, d.cw, d.ch = win
    return d, arr, 1 if planes == "y" else 3, _lib.STATS_WORDS + (_lib.STATS_BINS if hist else 0)


def stats_fields(t):
    """Named views of a statistics tensor ``t`` of shape (..., L), L = 8 or 264,
    without a copy: ``count, sum, sumsq, min, max, sad, ssd`` of shape (...),
    and ``hist`` of shape (..., 256) where L holds it."""
    if t.shape[-1] not in (_lib.STATS_WORDS, _lib.STATS_WORDS + _lib.STATS_BINS):
        raise ValueError(f"stats_fields: a last dimension of {_lib.STATS_WORDS} or {_lib.STATS_WORDS + _lib.STATS_BINS} words")
    out = {name: t[..., i] for i, name in enumerate(_lib.STATS_FIELDS)}
    if t.shape[-1] > _lib.STATS_WORDS:
        out["hist"] = t[..., _lib.STATS_WORDS:]
    return out


def _field_channels(channels, table, max_ch):
    """The ids of ``channels`` (a name or names of ``table``, 1..max_ch of them)."""
    if isinstance(channels, str):
        channels = (channels,)
    channels = tuple(channels)
    if not 1 <= len(channels) <= max_ch:
        raise ValueError(f"channels: 1..{max_ch} names")
    bad = [c for c in channels if c not in table]
    if bad:
        raise ValueError(f"channels {bad}: each one of {sorted(table)}")
    return [table[c] for c in channels]


def _field_desc(d, n, per, window, dtype, scale, bias, blocks=False, uv=False):
    """What the four field descriptors (mbinfo, residual, accmv, accres) share,
    filled into ``d``: the window -- d's first four ints, in 4x4 blocks
    (``blocks``) or luma samples, all even for ``uv`` --, the element type, and
    scale and bias expanded to ``n`` values, one per ``per`` ("channel" or
    "plane").  Returns (d, n, torch dtype)."""
    import torch
    dtype = torch.int16 if dtype is None else dtype
    dts = {torch.int16: _lib.TENSOR_I16, torch.float16: _lib.TENSOR_F16, torch.bfloat16: _lib.TENSOR_BF16,
           torch.float32: _lib.TENSOR_F32}
    if dtype not in dts:
        raise ValueError(f"dtype {dtype}: one of torch.int16, float16, bfloat16, float32")

    def expand(v, default, what):
        if v is None:
            return (default,) * n
        v = tuple(float(f) for f in v) if hasattr(v, "__len__") else (float(v),) * n
        if len(v) != n:
            raise ValueError(f"{what}: a scalar or one value per {per}")
        return v

    if window is not None:
        x, y, w, h = ("bx", "by", "bw", "bh") if blocks else ("x", "y", "cw", "ch")
        try:
            vx, vy, vw, vh = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError(f"window {window!r}: ({x}, {y}, {w}, {h})") from None
        for name, v in ((x, vx), (y, vy), (w, vw), (h, vh)):
            setattr(d, name, v)
        vx, vy, vw, vh = (getattr(d, name) for name in (x, y, w, h))       # (as the C ints hold them)
        if vx < 0 or vy < 0 or vw < 1 or vh < 1:
            raise ValueError(f"window {tuple(window)}: {x}, {y} >= 0 and {w}, {h} >= 1 "
                             f"({'4x4 blocks' if blocks else 'luma samples'})")
        if uv and (vx | vy | vw | vh) & 1:
            raise ValueError(f"window {tuple(window)}: x, y, cw and ch are even for planes 'uv'")
    d.dtype = dts[dtype]
    d.scale[:n] = expand(scale, 1.0, "scale")
    d.bias[:n] = expand(bias, 0.0, "bias")
    return d, n, dtype


def mbinfo_desc(channels, window=None, dtype=None, scale=None, bias=None):
    """(``_lib.MbInfoDesc``, number of channels, torch dtype) of an export of
    motion vectors and MB side information (Engine.to_mbinfo, Decoder's
    ``mbinfo`` option): ``channels`` names the planes, in order, repeats
    allowed (1..16 of "mvx", "mvy", "ref_idx", "ref_slot", "mb_type", "qp",
    "intra_mode", "coded", "slice"; include/h264mi.h defines them); window =
    (bx, by, bw, bh) in 4x4 blocks, or None for the blocks covering the
    decoder's SPS crop window (bw = 0 in the descriptor).  ``dtype``:
    torch.int16 (the default; the integer itself) or float16 / bfloat16 /
    float32, ``fma(v, scale[c], bias[c])`` of channel position c; scale and
    bias are scalars or one value per channel, default 1 and 0."""
    ids = _field_channels(channels, _lib.MBINFO_CHANNELS, _lib.MBINFO_MAX_CH)
    d = _lib.MbInfoDesc()
    d.nch, d.ch[:len(ids)] = len(ids), ids
    return _field_desc(d, len(ids), "channel", window, dtype, scale, bias, blocks=True)


def residual_desc(planes="y", window=None, dtype=None, scale=None, bias=None):
    """(``_lib.ResidualDesc``, number of planes, torch dtype) of an export of
    the decoded residual (Engine.to_residual, Decoder's ``residual`` option;
    include/h264mi.h defines the field): ``planes`` is "y" (one plane), "uv"
    (Cb and Cr at half resolution) or "yuv" (three planes at luma resolution,
    chroma by nearest neighbour); window = (x, y, cw, ch) in luma samples of
    the MB-aligned picture, all even for "uv", or None for the decoder's SPS
    crop window (cw = ch = 0 in the descriptor).  ``dtype``: torch.int16 (the
    default; the integer itself) or float16 / bfloat16 / float32, ``fma(v,
    scale[c], bias[c])`` of plane position c; scale and bias are scalars or
    one value per plane, default 1 and 0."""
    if planes not in _lib.RESID_PLANES:
        raise ValueError(f"planes {planes!r}: one of {sorted(_lib.RESID_PLANES)}")
    d = _lib.ResidualDesc()
    d.planes = _lib.RESID_PLANES[planes]
    return _field_desc(d, {"y": 1, "uv": 2, "yuv": 3}[planes], "plane", window, dtype, scale, bias, uv=planes == "uv")


def accmv_desc(channels=("adx", "ady"), window=None, dtype=None, scale=None, bias=None, size=None):
    """(``_lib.AccMvDesc``, number of channels, torch dtype) of an export of
    the accumulated motion (Engine.to_accmv, Decoder's ``accmv`` option;
    include/h264mi.h defines the field): ``channels`` names the planes, in
    order, repeats allowed (1..8 of "adx", "ady", "jx", "jy", "anchored");
    window = (x, y, cw, ch) in luma samples of the MB-aligned picture, or None
    for the decoder's SPS crop window (cw = ch = 0 in the descriptor).
    ``dtype``: torch.int16 (the default; the integer itself) or float16 /
    bfloat16 / float32, ``fma(v, scale[c], bias[c])`` of channel position c;
    scale and bias are scalars or one value per channel, default 1 and 0.
    With ``size`` = (oh, ow), each 1..16384, the descriptor is a
    ``_lib.AccMvResizeDesc`` of the resized export (its ``f`` is the one
    above): the window's integer field filtered to oh x ow per channel
    (DESIGN 3.5i), int16 rounded to the nearest integer, halves up."""
    ids = _field_channels(channels, _lib.ACCMV_CHANNELS, _lib.ACCMV_MAX_CH)
    d = _lib.AccMvDesc()
    d.nch, d.id[:len(ids)] = len(ids), ids
    return _field_resized(_lib.AccMvResizeDesc, _field_desc(d, len(ids), "channel", window, dtype, scale, bias), size)


def accres_desc(planes="y", window=None, dtype=None, scale=None, bias=None, colour=None, unanchored="key", size=None):
    """(``_lib.AccResDesc``, number of planes, torch dtype) of an export of the
    accumulated residual (Engine.to_accres; include/h264mi.h defines the
    field): every sample of the picture minus its
    origin in the key picture of its GOP.  ``planes`` is "y" (one plane), "uv"
    (Cb and Cr at half resolution), "yuv" (three planes at luma resolution,
    chroma by nearest neighbour) or "rgb" (three planes at luma resolution,
    the difference of the two pixels converted under ``colour``: a name of
    ``_lib.TENSOR_COLOURS`` but "stream", None is "reference"; "rgb" only).
    ``unanchored``: "key" -- a sample whose chain back started at an intra MB is
    set against the key picture where that chain started -- or "zero": such a
    sample is 0.  window, dtype, scale and bias as for ``residual_desc``;
    ``size`` as for ``accmv_desc`` (a ``_lib.AccResResizeDesc``; "uv": its
    half-resolution grid is what is resized)."""
    if not isinstance(planes, str) or planes not in _lib.ACCRES_PLANES:
        raise ValueError(f"planes {planes!r}: one of {sorted(_lib.ACCRES_PLANES)}")
    if not isinstance(unanchored, str) or unanchored not in _lib.ACCRES_UNANCHORED:
        raise ValueError(f"unanchored {unanchored!r}: one of {sorted(_lib.ACCRES_UNANCHORED)}")
    if colour is not None and planes != "rgb":
        raise ValueError(f"colour: planes {planes!r} have no colour set (only 'rgb')")
    colour = "reference" if colour is None else colour
    if not isinstance(colour, str) or colour not in _lib.TENSOR_COLOURS or colour == "stream":
        raise ValueError(f"colour {colour!r}: one of {sorted(set(_lib.TENSOR_COLOURS) - {'stream'})}")
    d = _lib.AccResDesc()
    d.planes = _lib.ACCRES_PLANES[planes]
    d.colour, d.unanchored = _lib.TENSOR_COLOURS[colour], _lib.ACCRES_UNANCHORED[unanchored]
    return _field_resized(_lib.AccResResizeDesc,
                          _field_desc(d, {"y": 1, "uv": 2, "yuv": 3, "rgb": 3}[planes], "plane", window, dtype, scale,
                                      bias, uv=planes == "uv"), size)


@dataclass
class CapturedPicture:
    rec: int            # host address of w*h MbRec
    coef: int           # host address of ncoef coefficient blocks
    ncoef: int
    cur_slot: int
    alg_ref_bytes: int
    n_inter: int
    n_intra: int
    n_coded: int
    ref_line_bytes: int = 0     # distinct 128-B reference lines the MC windows touch, x 128


class Capture:
    def __init__(self, stream: bytes, no_reorder: bool = False):
        self._L = _lib.mi()
        self._buf = C.create_string_buffer(stream, len(stream))
        self._h = self._L.h264mi_capture_stream(C.cast(self._buf, C.c_void_p), len(stream), int(no_reorder))
        if not self._h:
            raise RuntimeError("capture failed")
        w, h, ns, npics, err = (C.c_int() for _ in range(5))
        self._L.h264mi_capture_info(self._h, C.byref(w), C.byref(h), C.byref(ns), C.byref(npics), C.byref(err))
        self.w_mbs, self.h_mbs, self.nslots = w.value, h.value, ns.value
        self.npics, self.errors = npics.value, err.value
        self.pictures: List[CapturedPicture] = [self._picture(i) for i in range(self.npics)]

    def _picture(self, i: int) -> CapturedPicture:
        rec, coef = C.c_void_p(), C.c_void_p()
        nc, slot = C.c_uint32(), C.c_int()
        alg = C.c_uint64()
        self._L.h264mi_capture_picture(self._h, i, C.byref(rec), C.byref(coef), C.byref(nc), C.byref(slot),
                                       C.byref(alg))
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._L.h264mi_capture_stats(self._h, i, C.byref(a), C.byref(b), C.byref(c))
        lb = C.c_uint64()
        self._L.h264mi_capture_ref_lines(self._h, i, C.byref(lb))
        return CapturedPicture(rec.value or 0, coef.value or 0, nc.value, slot.value, alg.value,
                               a.value, b.value, c.value, lb.value)

    def records_bytes(self, i: int) -> bytes:
        p = self.pictures[i]
        return C.string_at(p.rec, self.w_mbs * self.h_mbs * MBREC_BYTES)

    def coef_bytes(self, i: int) -> bytes:
        p = self.pictures[i]
        return C.string_at(p.coef, p.ncoef * 32) if p.ncoef else b""

    def close(self):
        if self._h:
            self._L.h264mi_capture_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, w_mbs: int, h_mbs: int, nstreams: int, nslots: int, device: int = 0):
        self._L = _lib.mi()
        self.w_mbs, self.h_mbs, self.nstreams, self.nslots = w_mbs, h_mbs, nstreams, nslots
        self._h = self._L.h264mi_engine_create(device, w_mbs, h_mbs, nstreams, nslots)
        if not self._h:
            raise RuntimeError("h264mi_engine_create failed (no HIP device?)")
        self.frame_bytes = self._L.h264mi_engine_frame_bytes(self._h)       # packed I420 (read's output)
        if hasattr(self._L, "h264mi_engine_slot_bytes"):
            self.slot_bytes = self._L.h264mi_engine_slot_bytes(self._h)     # device slot stride
            self.chroma_pitch = self._L.h264mi_engine_chroma_pitch(self._h) # H264MI_CPITCH
        else:                                                               # an older tree's A/B build: packed slots
            self.slot_bytes, self.chroma_pitch = self.frame_bytes, w_mbs * 8

    def decode(self, streams: Sequence[int], pics: Sequence[CapturedPicture]) -> None:
        n = len(pics)
        st = (C.c_int * n)(*streams)
        sl = (C.c_int * n)(*[p.cur_slot for p in pics])
        recs = (C.c_void_p * n)(*[p.rec for p in pics])
        coefs = (C.c_void_p * n)(*[p.coef for p in pics])
        nc = (C.c_uint32 * n)(*[p.ncoef for p in pics])
        if self._L.h264mi_engine_decode(self._h, n, st, sl, recs, coefs, nc) != 0:
            raise RuntimeError("h264mi_engine_decode failed")

    def decode_device(self, npics: int, d_recs: int, d_coef: int, d_pics: int) -> None:
        if self._L.h264mi_engine_decode_device(self._h, npics, d_recs, d_coef, d_pics) != 0:
            raise RuntimeError("h264mi_engine_decode_device failed")

    def decode_device_next(self, npics: int, d_recs: int, d_coef: int, d_pics: int,
                           n_recs: int, n_coef: int, n_pics: int) -> None:
        """decode_device, naming the next batch: its k_prep runs in this
        launch's tail."""
        if self._L.h264mi_engine_decode_device_next(self._h, npics, d_recs, d_coef, d_pics,
                                                    n_recs, n_coef, n_pics) != 0:
            raise RuntimeError("h264mi_engine_decode_device_next failed")

    def hint_deps(self, mode: int) -> None:
        """Dependency mode of the next frame-pipelined launch: 1 whole MB
        rows, 2 (MB row, MB column) cells, 0 the engine's default."""
        if not hasattr(self._L, "h264mi_engine_hint_deps"):     # an older tree's A/B build
            return
        if self._L.h264mi_engine_hint_deps(self._h, int(mode)) != 0:
            raise RuntimeError("h264mi_engine_hint_deps failed")

    def last_deps(self) -> int:
        if not hasattr(self._L, "h264mi_engine_last_deps"):
            return -1
        return int(self._L.h264mi_engine_last_deps(self._h))

    def last_mc_waves(self) -> int:
        """MC waves per row workgroup of the last launch (-1: an older build)."""
        if not hasattr(self._L, "h264mi_engine_last_mc_waves"):
            return -1
        return int(self._L.h264mi_engine_last_mc_waves(self._h))

    def hint_intra(self, intra_heavy: bool) -> None:
        """Shape hint for the next device-resident launch: does some picture
        have more than half its MBs intra (include/h264mi.h)."""
        if self._L.h264mi_engine_hint_intra(self._h, int(bool(intra_heavy))) != 0:
            raise RuntimeError("h264mi_engine_hint_intra failed")

    def set_steps(self, steps: int) -> None:
        """Pictures per stream per launch for decode_device_steps (1..2)."""
        if self._L.h264mi_engine_set_steps(self._h, steps) != 0:
            raise RuntimeError("h264mi_engine_set_steps failed")

    def decode_device_steps(self, S: int, P: int, d_recs: int, d_coef: int, d_pics: int,
                            n_recs: int = 0, n_coef: int = 0, n_pics: int = 0) -> None:
        """P consecutive pictures of each of S streams in one launch
        (descriptors step-major, rec_base relative to d_recs); the next
        batch's k_prep in this launch's tail when n_recs is given."""
        if self._L.h264mi_engine_decode_device_steps(self._h, S, P, d_recs, d_coef, d_pics,
                                                     n_recs or None, n_coef or None, n_pics or None) != 0:
            raise RuntimeError("h264mi_engine_decode_device_steps failed")

    def decode_device_steps_next(self, S: int, P: int, d_recs: int, d_coef: int, d_pics: int,
                                 n_recs: int, n_coef: int, n_pics: int, next_P: int) -> bool:
        """decode_device_steps with the next batch's step count when it
        differs (its k_prep over S * next_P pictures in this launch's tail).
        False: the library predates it (nothing launched)."""
        if not hasattr(self._L, "h264mi_engine_decode_device_steps_next"):
            return False
        if self._L.h264mi_engine_decode_device_steps_next(self._h, S, P, d_recs, d_coef, d_pics,
                                                          n_recs, n_coef, n_pics, next_P) != 0:
            raise RuntimeError("h264mi_engine_decode_device_steps_next failed")
        return True

    def read(self, stream: int, slot: int) -> np.ndarray:
        out = np.empty(self.frame_bytes, dtype=np.uint8)
        if self._L.h264mi_engine_read(self._h, stream, slot, out.ctypes.data) != 0:
            raise RuntimeError("h264mi_engine_read failed")
        return out

    def read_rgba(self, stream: int, slot: int) -> np.ndarray:
        """The slot converted to RGBA on the GPU (Decoder.js `rgb: true`)."""
        out = np.empty(self.frame_bytes // 3 * 8, dtype=np.uint8)       # w*h*1.5 -> w*h*4
        if self._L.h264mi_engine_read_rgba(self._h, stream, slot, out.ctypes.data) != 0:
            raise RuntimeError("h264mi_engine_read_rgba failed")
        return out

    def read_crop(self, stream: int, slot: int, x: int, y: int, cw: int, ch: int, rgba: bool = False) -> np.ndarray:
        """The window (x, y, cw, ch; luma pixels, all even) of the slot,
        cropped on the GPU: packed I420 (cw*ch*3/2 bytes, the layout of the
        reference testbench's CropPicture) or RGBA (cw*ch*4 bytes)."""
        out = np.empty(cw * ch * 4 if rgba else cw * ch * 3 // 2, dtype=np.uint8)
        if self._L.h264mi_engine_read_crop(self._h, stream, slot, x, y, cw, ch, int(bool(rgba)),
                                           out.ctypes.data) != 0:
            raise RuntimeError("h264mi_engine_read_crop failed")
        return out

    @staticmethod
    def _pictures(streams: Sequence[int], slots: Sequence[int]):
        """(n, streams, slots) of an export's pictures, the two as C int arrays."""
        n = len(streams)
        if n < 1 or len(slots) != n:
            raise ValueError("streams and slots name the same, non-zero number of pictures")
        return n, (C.c_int * n)(*streams), (C.c_int * n)(*slots)

    def _out(self, shape, dtype, out, stream, layout="nchw"):
        """(out, HIP stream handle) of an export: ``out``, checked, or a new
        ``torch.empty`` (``layout`` "nhwc": ``empty_layout`` / ``check_out``);
        ``stream`` or torch's current stream of the device."""
        import torch
        dev = torch.device("cuda", self.device)
        if layout != "nchw":
            if out is None:
                with torch.cuda.device(self.device):
                    out = empty_layout(shape, dtype, dev, layout)
            else:
                check_out(out, shape, dtype, dev, layout)
        elif out is None:
            with torch.cuda.device(self.device):
                out = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out: a contiguous {dtype} tensor of shape {shape} on {dev} "
                             f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
        cur = torch.cuda.current_stream(dev)
        st = stream if stream is not None else cur
        if st != cur:
            out.record_stream(st)       # (the caching allocator: the block is in use on `stream` too)
        return out, st.cuda_stream

    def _out_dest(self, shape, dtype, out, stream, layout="nchw", clip=None):
        """``_out`` for the pixel exports: (out, HIP stream handle, None) where
        the existing calls serve -- no ``out``, or one that is dense in
        ``layout`` -- and otherwise (out, handle, (``_lib.TensorDest``,
        out_stride)) of ``dest_of_view``.  ``clip`` = T: the ``shape[0]`` items
        as ``(shape[0] // T, planes, T, rows, cols)``, a new ``empty_clip`` or
        ``out``, always through a destination."""
        import torch
        dev = torch.device("cuda", self.device)
        if clip is None:
            dense = out is None or (tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.device == dev and
                                    (out.permute(0, 2, 3, 1) if layout != "nchw" else out).is_contiguous())
            if dense:
                return self._out(shape, dtype, out, stream, layout) + (None,)
        else:
            n, planes, rows, cols = shape
            if not isinstance(clip, int) or isinstance(clip, bool) or clip < 1 or n % clip:
                raise ValueError(f"clip {clip!r}: a positive integer that divides the {n} items")
            shape = (n // clip, planes, clip, rows, cols)
            if out is None:
                with torch.cuda.device(self.device):
                    out = empty_clip(shape, dtype, dev, layout)
        dest = dest_of_view(out, shape, dtype, dev, layout)
        cur = torch.cuda.current_stream(dev)
        st = stream if stream is not None else cur
        if st != cur:
            out.record_stream(st)
        return out, st.cuda_stream, dest

    def _export_dest(self, n, c_streams, c_slots, desc, boxes, layout, out, st, dest):
        """``out`` filled through h264mi_engine_export_tensor_dest: ``desc`` any
        pixel export's descriptor, ``boxes`` a ``_lib.Roi`` array or None,
        ``dest`` from ``_out_dest``."""
        ld = desc if isinstance(desc, _lib.TensorLayoutDesc) else layout_desc(desc, layout)
        d, out_stride = dest
        if not hasattr(self._L, "h264mi_engine_export_tensor_dest") or \
                self._L.h264mi_engine_export_tensor_dest(self._h, n, c_streams, c_slots, C.byref(ld), boxes,
                                                         len(boxes) if boxes is not None else 0, C.byref(d),
                                                         out.data_ptr(), out_stride, st) != 0:
            raise RuntimeError("h264mi_engine_export_tensor_dest failed (stream, slot, window or size out of range?)")
        return out

    def _export_field(self, entry, needs, streams, slots, window, build, out, stream, blocks=False, uv=False):
        """A field export (to_mbinfo, to_residual, to_accmv, to_accres) through
        the library's ``entry``, which needs the retention ``needs``:
        ``build(window)`` is the field's ``*_desc`` call; window None: the whole
        MB-aligned picture in 4x4 blocks (``blocks``) or luma samples; ``uv``:
        the planes are at half resolution."""
        n, c_streams, c_slots = self._pictures(streams, slots)
        unit = 4 if blocks else 16
        if window is None:
            window = (0, 0, self.w_mbs * unit, self.h_mbs * unit)
        desc, planes, dtype = build(window)
        if hasattr(desc, "oh"):                 # a resize descriptor
            rows, cols = desc.oh, desc.ow
        else:
            rows, cols = (desc.bh, desc.bw) if blocks else (desc.ch >> uv, desc.cw >> uv)
        out, st = self._out((n, planes, rows, cols), dtype, out, stream)
        if not hasattr(self._L, entry) or \
                getattr(self._L, entry)(self._h, n, c_streams, c_slots, C.byref(desc), out.data_ptr(),
                                        planes * rows * cols * out.element_size(), st) != 0:
            raise RuntimeError(f"{entry} failed ({needs} off, or stream, slot or window out of range?)")
        return out

    def to_tensor(self, streams: Sequence[int], slots: Sequence[int], window=None, mode: str = "rgb", dtype=None,
                  scale=None, bias=None, mean=None, std=None, out=None, stream=None, size=None, colour=None,
                  rois=None, fit=None, pad=None, layout="nchw", warps=None, border=None, filter=None, clip=None):
        """The slots (streams[k], slots[k]) as one ``(n, planes, ch, cw)``
        torch tensor on ``cuda:{self.device}``, built on the GPU and never
        copied to the host: planes R, G, B (``mode="rgb"``, the values of
        read_rgba) or luma (``"gray"``) of ``window`` = (x, y, cw, ch), all
        even (None: the whole picture), as ``dtype`` (torch.uint8, float16 --
        the default --, bfloat16 or float32).  Float elements are
        ``fma(c, scale[p], bias[p])`` in fp32, rounded once more to the 16-bit
        types; scale and bias are scalars or per-plane triples (default
        1 / 255 and 0), or come from ``mean`` / ``std`` (``tensor_affine``);
        uint8 ignores them.  ``size`` = (oh, ow): the window's 8-bit samples
        resized on the GPU before that conversion (antialiased triangle
        filter in integer arithmetic; a window at most 32 times
        the output on each axis) -- the result is ``(n, planes, oh, ow)``.
        ``filter`` (with ``size``; every form below but ``warps``):
        "triangle", that default, or "bicubic" -- the antialiased bicubic
        filter (Keys, a = -0.5) of PIL's BICUBIC and torch's ``bicubic,
        antialias=True``, what CLIP / SigLIP / DINOv2-style encoders and the
        timm ViT transforms resize with, in integer arithmetic and
        reproducible to the byte; a window at most 16 times the
        output on each axis.
        ``colour`` (``mode="rgb"`` only): the colour set of the R, G, B
        samples -- None / "reference" (BT.601 limited range, the values of
        read_rgba), "bt601-full", "bt709" or "bt709-full" (DESIGN 3.5f); the
        resize works on the samples of that set.

        ``rois`` = [(k, x, y, cw, ch), ...] (with ``size``, without
        ``window``): a list of boxes instead of one window, box r the window
        (x, y, cw, ch) of picture k of the list (streams[k], slots[k]), every
        one resized to ``size`` -- the result is ``(len(rois), planes, oh,
        ow)``, box r holding the bytes ``window=(x, y, cw, ch), size=size``
        gives for that picture, from one kernel launch per 32 boxes and one
        ordering of the streams for the whole list.  Each box is
        even, inside the picture and at most 32 times ``size`` on each axis
        (``snap_rois`` makes such boxes from a detector's corners); a bad box,
        an empty list or a k out of range is a ValueError.

        ``fit`` = "letterbox", "topleft" or "stretch" (with ``size``, with or
        without ``rois``): ``size`` is a canvas, and the window -- or every box
        on its own -- is scaled with its aspect ratio kept
        (``letterbox_fit``), centred ("letterbox") or at the top left, the rest
        of the canvas being the element of the sample ``pad`` (default 114;
        one value, or one per plane) under the same scale and bias, all in
        the one launch.  "stretch" gives the bytes of ``size``
        alone.  ``engine.unletterbox`` maps a detector's boxes back.

        ``layout`` = "nhwc" (every form above): the same values
        stored channels-last by the export's own kernel -- the result has the
        usual shape ``(n, planes, rows, cols)`` with the strides of
        ``torch.channels_last`` (``empty_layout``), so model code is unchanged
        and ``t.permute(0, 2, 3, 1)`` is the contiguous HWC view; ``out`` then
        is such a tensor (``check_out``).  "nchw", the default, is everything
        above, untouched.  With ``mode="gray"`` the two are the same bytes.

        ``warps`` = [(k, (m0, ..., m5)), ...] (with ``size``; not with ``rois``
        or ``fit``): affine warps instead of upright boxes --
        rotated boxes turned upright, crops aligned to landmarks.  Warp r makes
        ``size`` outputs from ``window`` of picture k: the six Q16 integers map
        output (row i, column j) to the window position ``(m0 j + m1 i + m2,
        m3 j + m4 i + m5) / 65536`` (the inverse map; ``warp_q16`` and
        ``rotated_box_warp`` make them), sampled bilinearly in integers from
        the converted samples, reproducible to the byte.  ``border``
        "constant" (default): a tap outside ``window`` is the sample ``pad``
        (default 0); "replicate": the window's edge sample.  Nothing outside
        ``window`` is read.  The result is ``(len(warps), planes, oh, ow)``,
        from one launch per 32 warps.  Not antialiased: shrink by more than
        about 2 : 1 with ``size`` / ``rois`` instead.

        The export is ordered on ``stream`` (a torch.cuda.Stream; default:
        torch's current stream of the device): it starts after the work queued
        there and after every launch queued on the engine, later work on
        ``stream`` sees the tensor, and a later launch that overwrites a slot
        waits for it.  The host is never synchronised.  ``out``: a tensor of
        the result's shape, dtype and device to fill instead of a new
        ``torch.empty`` -- contiguous, or any view whose strides the exports
        can write through (``dest_of_view``; every form above): a
        channel slice ``x[:, 1:4]`` of a wider tensor, a tile of a canvas, a
        permuted clip, rows with a pitch.  Only the view's elements are
        written.  A view with a column stride other than 1 ("nhwc": a plane
        stride other than 1), an expanded dimension or overlapping elements is
        a ValueError that names the stride.

        ``clip`` = T (every form above; the number of items a multiple of T):
        the items as video clips, ``(n // T, planes, T, rows, cols)`` --
        contiguous NCTHW, what video models take, written in place by the same
        kernels instead of ``permute(...).contiguous()`` over the result; with
        ``layout="nhwc"`` the same shape with the strides of
        ``torch.channels_last_3d``.  Item k is frame ``k % T`` of clip ``k //
        T``; with ``rois`` or ``warps`` a clip is a tube, one tracked box over T
        pictures.  ``out`` then is a 5-D view under the same rules.

        The result is an ordinary torch tensor, so DLPack
        consumers (``torch.utils.dlpack`` / ``__dlpack__``) need nothing further."""
        n, c_streams, c_slots = self._pictures(streams, slots)
        nhwc = tensor_layout(layout) != 0
        if warps is None and border is not None:
            raise ValueError("border: goes with warps")
        if warps is not None:
            _no_filter(filter, "warps are sampled bilinearly")
            if rois is not None or fit is not None:
                raise ValueError("warps: not combinable with rois or fit")
            if window is None:
                window = (0, 0, self.w_mbs * 16, self.h_mbs * 16)
            desc, mats, planes, dtype = warps_desc(warps, size, n, window, self.w_mbs * 16, self.h_mbs * 16, mode, dtype,
                                                   scale, bias, mean, std, colour, border=border, pad=pad, layout=layout)
            out, st, dest = self._out_dest((len(mats), planes, desc.oh, desc.ow), dtype, out, stream, layout, clip)
            if dest is not None:
                if not hasattr(self._L, "h264mi_engine_export_tensor_warps_dest") or \
                        self._L.h264mi_engine_export_tensor_warps_dest(self._h, n, c_streams, c_slots, C.byref(desc), mats,
                                                                       len(mats), C.byref(dest[0]), out.data_ptr(), dest[1],
                                                                       st) != 0:
                    raise RuntimeError("h264mi_engine_export_tensor_warps_dest failed (stream or slot out of range?)")
                return out
            if not hasattr(self._L, "h264mi_engine_export_tensor_warps") or \
                    self._L.h264mi_engine_export_tensor_warps(self._h, n, c_streams, c_slots, C.byref(desc), mats, len(mats),
                                                              out.data_ptr(), planes * desc.oh * desc.ow * out.element_size(),
                                                              st) != 0:
                raise RuntimeError("h264mi_engine_export_tensor_warps failed (stream or slot out of range?)")
            return out
        fitted = fit is not None or pad is not None
        if fitted and size is None:
            raise ValueError("fit and pad go with size=(oh, ow), the canvas")
        if rois is not None:
            if window is not None:
                raise ValueError("rois: not combinable with window (each box is one)")
            desc, boxes, planes, dtype = rois_desc(rois, size, n, self.w_mbs * 16, self.h_mbs * 16, mode, dtype, scale,
                                                   bias, mean, std, colour, fit=fit, pad=pad, filter=filter)
            name = "h264mi_engine_export_tensor_rois_fit" if fitted else "h264mi_engine_export_tensor_rois"
            oh, ow = (desc.r.oh, desc.r.ow) if fitted else (desc.oh, desc.ow)
            out, st, dest = self._out_dest((len(boxes), planes, oh, ow), dtype, out, stream, layout, clip)
            if dest is not None:
                return self._export_dest(n, c_streams, c_slots, desc, boxes, layout, out, st, dest)
            if nhwc:
                return self._export_layout(n, c_streams, c_slots, desc, boxes, (len(boxes), planes, oh, ow), dtype, out,
                                           stream, layout)
            if not hasattr(self._L, name) or \
                    getattr(self._L, name)(self._h, n, c_streams, c_slots, C.byref(desc), boxes, len(boxes),
                                           out.data_ptr(), planes * oh * ow * out.element_size(), st) != 0:
                raise RuntimeError(f"{name} failed (stream or slot out of range?)")
            return out
        if window is None:
            window = (0, 0, self.w_mbs * 16, self.h_mbs * 16)
        desc, planes, dtype = tensor_desc(window, mode, dtype, scale, bias, mean, std, size, colour, filter=filter)
        if fitted:
            fd = fit_desc(desc, planes, "letterbox" if fit is None else fit, 114 if pad is None else pad)
            out, st, dest = self._out_dest((n, planes, desc.oh, desc.ow), dtype, out, stream, layout, clip)
            if dest is not None:
                return self._export_dest(n, c_streams, c_slots, fd, None, layout, out, st, dest)
            if nhwc:
                return self._export_layout(n, c_streams, c_slots, fd, None, (n, planes, desc.oh, desc.ow), dtype, out,
                                           stream, layout)
            if not hasattr(self._L, "h264mi_engine_export_tensor_fit") or \
                    self._L.h264mi_engine_export_tensor_fit(self._h, n, c_streams, c_slots, C.byref(fd), out.data_ptr(),
                                                            planes * desc.oh * desc.ow * out.element_size(), st) != 0:
                raise RuntimeError("h264mi_engine_export_tensor_fit failed (stream, slot, window or size out of range?)")
            return out
        shape = (n, planes, desc.ch, desc.cw) if size is None else (n, planes, desc.oh, desc.ow)
        if out is None and min(shape) < 1:
            raise ValueError(f"window {tuple(window)}")
        out, st, dest = self._out_dest(shape, dtype, out, stream, layout, clip)
        if dest is not None:
            return self._export_dest(n, c_streams, c_slots, desc, None, layout, out, st, dest)
        if nhwc:
            return self._export_layout(n, c_streams, c_slots, desc, None, shape, dtype, out, stream, layout)
        export = self._L.h264mi_engine_export_tensor if size is None else self._L.h264mi_engine_export_tensor_resized
        if export(self._h, n, c_streams, c_slots, C.byref(desc), out.data_ptr(),
                  planes * shape[2] * shape[3] * out.element_size(), st) != 0:
            raise RuntimeError(f"{export.__name__} failed (stream, slot, window or size out of range?)")
        return out

    def _export_layout(self, n, c_streams, c_slots, desc, boxes, shape, dtype, out, stream, layout):
        """to_tensor's export of ``desc`` (any pixel export's descriptor; with
        ``boxes``, a ``_lib.Roi`` array, the list form) under ``layout`` through
        h264mi_engine_export_tensor_layout."""
        out, st = self._out(shape, dtype, out, stream, layout)
        ld = layout_desc(desc, layout)
        if not hasattr(self._L, "h264mi_engine_export_tensor_layout") or \
                self._L.h264mi_engine_export_tensor_layout(self._h, n, c_streams, c_slots, C.byref(ld), boxes,
                                                           len(boxes) if boxes is not None else 0, out.data_ptr(),
                                                           shape[1] * shape[2] * shape[3] * out.element_size(), st) != 0:
            raise RuntimeError("h264mi_engine_export_tensor_layout failed (stream, slot, window or size out of range?)")
        return out

    def to_stats(self, streams: Sequence[int], slots: Sequence[int], planes="y", window=None, rois=None, hist=False,
                 ref=None, colour=None, out=None, stream=None):
        """Statistics of the pictures in the slots (streams[k], slots[k]) as one
        ``int64`` torch tensor of shape ``(N or K, P, L)`` on
        ``cuda:{self.device}`` (stats.hip, ``stats_desc``; nothing is exported
        and nothing reaches the host): per item -- ``window`` = (x, y, cw, ch)
        of each of the N pictures (None: all of it), or the K boxes ``rois`` =
        [(k, x, y, cw, ch), ...] -- and per plane of ``planes`` ("y": P = 1;
        "yuv", chroma at its own resolution, and "rgb", the uint8 samples of
        ``to_tensor`` under ``colour``: P = 3) the L = 8 words ``count, sum,
        sumsq, min, max, sad, ssd, 0`` and, with ``hist``, 256 bins behind
        them (``stats_fields`` names them).  ``ref`` = (ref_streams,
        ref_slots), as many slots: sad and ssd of picture k against reference k
        over the same window (0 without).  Exact integers; ``out`` and
        ``stream`` as for ``to_tensor``: no host synchronisation, and a later
        decode into a named slot waits."""
        import torch
        n, c_streams, c_slots = self._pictures(streams, slots)
        if window is None and rois is None:
            window = (0, 0, self.w_mbs * 16, self.h_mbs * 16)
        desc, boxes, P, L = stats_desc(planes, window, rois, hist, colour, n, self.w_mbs * 16, self.h_mbs * 16)
        c_rs = c_rl = None
        if ref is not None:
            try:
                rs, rl = ref
                if len(rs) != n or len(rl) != n:
                    raise ValueError
            except (TypeError, ValueError):
                raise ValueError(f"ref: (ref_streams, ref_slots) naming {n} pictures, one per picture") from None
            c_rs, c_rl = (C.c_int * n)(*rs), (C.c_int * n)(*rl)
        items = len(boxes) if boxes is not None else n
        out, st = self._out((items, P, L), torch.int64, out, stream)
        if not hasattr(self._L, "h264mi_engine_export_stats") or \
                self._L.h264mi_engine_export_stats(self._h, n, c_streams, c_slots, c_rs, c_rl, C.byref(desc), boxes,
                                                   len(boxes) if boxes is not None else 0, out.data_ptr(), P * L * 8,
                                                   st) != 0:
            raise RuntimeError("h264mi_engine_export_stats failed (stream, slot or window out of range?)")
        return out

    def keep_records(self, on: bool = True) -> None:
        """Keep each picture's MB records on the device, per (stream, slot),
        from the next ``decode`` on (to_mbinfo reads them); ``on=False`` waits
        for the engine and frees them.  ``decode_device*`` launches retain
        nothing."""
        if self._L.h264mi_engine_keep_records(self._h, int(bool(on))) != 0:
            raise RuntimeError("h264mi_engine_keep_records failed")

    def forget_records(self, stream: int, slot: int) -> None:
        """Mark the slot's kept records as "no information" and, with
        ``keep_accmv`` on, reset its origin map."""
        if self._L.h264mi_engine_forget_records(self._h, stream, slot) != 0:
            raise RuntimeError("h264mi_engine_forget_records failed (keep_records and keep_accmv off, or a bad "
                               "stream or slot)")

    def to_mbinfo(self, streams: Sequence[int], slots: Sequence[int], channels=("mvx", "mvy"), window=None,
                  dtype=None, scale=None, bias=None, out=None, stream=None):
        """Motion vectors and MB side information of the pictures last
        decoded into the slots (streams[k], slots[k]) as one ``(n, C, bh,
        bw)`` torch tensor on ``cuda:{self.device}``, one element per luma 4x4
        block of ``window`` = (bx, by, bw, bh) in blocks (None: the whole
        picture, 4 * h_mbs rows of 4 * w_mbs) and per name in ``channels``
        (``mbinfo_desc``; a slot nothing was decoded into reads as "no
        information").  Needs ``keep_records()`` before the decodes.  ``out``
        and ``stream`` as for ``to_tensor``; the host is never synchronised."""
        return self._export_field("h264mi_engine_export_mbinfo", "keep_records", streams, slots, window,
                                  lambda w: mbinfo_desc(channels, w, dtype, scale, bias), out, stream, blocks=True)

    def keep_coefs(self, on: bool = True) -> None:
        """Keep each picture's coefficient blocks, and its records, on the
        device, per (stream, slot), from the next ``decode`` on (to_residual
        reads them): 27 blocks of 32 bytes per MB and slot, 7.05 MB per 1080p
        slot.  ``on=False`` waits for the engine, frees them and leaves the
        records to ``keep_records``' own switch.  ``decode_device*`` launches
        retain nothing."""
        if self._L.h264mi_engine_keep_coefs(self._h, int(bool(on))) != 0:
            raise RuntimeError("h264mi_engine_keep_coefs failed")

    def to_residual(self, streams: Sequence[int], slots: Sequence[int], planes="y", window=None, dtype=None,
                    scale=None, bias=None, out=None, stream=None):
        """The decoded residual of the pictures last decoded into the slots
        (streams[k], slots[k]) as one ``(n, 1 | 2 | 3, rows, columns)`` torch
        tensor on ``cuda:{self.device}``: ``planes`` "y" and "yuv" give ``(ch,
        cw)`` planes of ``window`` = (x, y, cw, ch) in luma samples (None: the
        whole MB-aligned picture), "uv" ``(ch / 2, cw / 2)`` (``residual_desc``;
        a slot nothing was decoded into reads as zeros).  Needs
        ``keep_coefs()`` before the decodes.  ``out`` and ``stream`` as for
        ``to_tensor``; the host is never synchronised."""
        return self._export_field("h264mi_engine_export_residual", "keep_coefs", streams, slots, window,
                                  lambda w: residual_desc(planes, w, dtype, scale, bias), out, stream,
                                  uv=planes == "uv")

    def keep_accmv(self, on: bool = True) -> None:
        """Keep each picture's origin map -- every luma sample traced back to
        its position in the key picture of its GOP -- on the device, per
        (stream, slot), from the next ``decode`` on (to_accmv reads them): 1024
        bytes per MB and slot, 8.36 MB per 1080p slot, and one gather launch
        per picture.  ``on=False`` waits for the engine and frees them.
        ``decode_device*`` launches retain nothing."""
        if not hasattr(self._L, "h264mi_engine_keep_accmv") or \
                self._L.h264mi_engine_keep_accmv(self._h, int(bool(on))) != 0:
            raise RuntimeError("h264mi_engine_keep_accmv failed")

    def to_accmv(self, streams: Sequence[int], slots: Sequence[int], channels=("adx", "ady"), window=None,
                 dtype=None, scale=None, bias=None, out=None, stream=None, size=None, filter=None):
        """The accumulated motion of the pictures last decoded into the slots
        (streams[k], slots[k]) as one ``(n, C, ch, cw)`` torch tensor on
        ``cuda:{self.device}``, one element per luma sample of ``window`` = (x,
        y, cw, ch) (None: the whole MB-aligned picture) and per name in
        ``channels`` (``accmv_desc``; a slot nothing was decoded into reads as
        (x, y, 0): no displacement, not anchored).  Needs ``keep_accmv()``
        before the decodes.  ``size`` = (oh, ow): the window's integer field
        resized on the GPU before the conversion (``accmv_desc``; a window at
        most 32 times the output and 16384 samples on each axis) -- the result
        is ``(n, C, oh, ow)``.  ``out`` and ``stream`` as for ``to_tensor``;
        the host is never synchronised.  (``filter``: ValueError; a field has
        the triangle only.)"""
        _no_filter(filter, "the accumulated motion is resized by the triangle")
        entry = "h264mi_engine_export_accmv" if size is None else "h264mi_engine_export_accmv_resized"
        return self._export_field(entry, "keep_accmv", streams, slots, window,
                                  lambda w: accmv_desc(channels, w, dtype, scale, bias, size), out, stream)

    def keep_accres(self, nkeys: int = 2) -> None:
        """Keep the samples of each stream's last ``nkeys`` (1..8) key pictures
        on the device beyond the life of their frame slots, from the next
        ``decode`` on (to_accres reads them): one frame per key (3.20 MB at
        1080p) and one device-to-device copy per key picture.  With 2, every
        picture of the previous GOP stays exportable after the next key picture
        was decoded.  Needs ``keep_accmv()`` first; ``keep_accmv(False)``
        switches this off too.  ``nkeys=0`` waits for the engine and frees
        them.  ``decode_device*`` launches retain nothing."""
        if not hasattr(self._L, "h264mi_engine_keep_accres") or \
                self._L.h264mi_engine_keep_accres(self._h, int(nkeys)) != 0:
            raise RuntimeError("h264mi_engine_keep_accres failed (keep_accmv off, or nkeys not in 0..8?)")

    def conceal(self, stream: int, slot: int, order: Sequence[int], decoded: Sequence[int]) -> None:
        """Neighbour-based concealment of the MBs ``order`` (in that order) of
        the picture in (stream, slot), in place, behind the work queued so far
        (``h264mi_engine_conceal``); ``decoded``: per MB 1 (decoded) or 0."""
        n = len(order)
        o = (C.c_int * max(n, 1))(*order)
        d = (C.c_uint8 * (self.w_mbs * self.h_mbs))(*decoded)
        if self._L.h264mi_engine_conceal(self._h, stream, slot, o, n, d) != 0:
            raise RuntimeError("h264mi_engine_conceal failed (a bad stream, slot or MB, or a picture too large)")

    def accres_held(self, stream: int, slot: int) -> bool:
        """Whether the key picture of the picture in (stream, slot) is held;
        to_accres gives zeros for a slot whose key is not."""
        r = self._L.h264mi_engine_accres_held(self._h, stream, slot) if hasattr(self._L, "h264mi_engine_accres_held") \
            else -1
        if r < 0:
            raise RuntimeError("h264mi_engine_accres_held failed (keep_accres off, or a bad stream or slot)")
        return bool(r)

    def to_accres(self, streams: Sequence[int], slots: Sequence[int], planes="y", window=None, dtype=None,
                  scale=None, bias=None, colour=None, unanchored="key", out=None, stream=None, size=None,
                  filter=None):
        """The accumulated residual of the pictures last decoded into the slots
        (streams[k], slots[k]) -- each sample minus its origin in the key
        picture of its GOP -- as one ``(n, 1 | 2 | 3, rows, columns)`` torch
        tensor on ``cuda:{self.device}``: ``planes`` "y", "yuv" and "rgb" give
        ``(ch, cw)`` planes of ``window`` = (x, y, cw, ch) in luma samples
        (None: the whole MB-aligned picture), "uv" ``(ch / 2, cw / 2)``
        (``accres_desc``; a slot whose key is not held -- ``accres_held`` --
        reads as zeros).  Needs ``keep_accmv()`` and ``keep_accres()`` before
        the decodes.  ``size`` = (oh, ow): each plane resized on the GPU as for
        ``to_accmv`` -- the result is ``(n, 1 | 2 | 3, oh, ow)``.  ``out`` and
        ``stream`` as for ``to_tensor``; the host is never synchronised.
        (``filter``: ValueError, as for ``to_accmv``.)"""
        _no_filter(filter, "the accumulated residual is resized by the triangle")
        entry = "h264mi_engine_export_accres" if size is None else "h264mi_engine_export_accres_resized"
        return self._export_field(entry, "keep_accres", streams, slots, window,
                                  lambda w: accres_desc(planes, w, dtype, scale, bias, colour, unanchored, size), out,
                                  stream, uv=planes == "uv")

    @property
    def device(self) -> int:
        return int(self._L.h264mi_engine_device(self._h))

    def alloc(self, nbytes: int) -> int:
        """Device memory on the engine's GPU (whatever the caller's current
        HIP device is)."""
        p = self._L.h264mi_engine_alloc(self._h, int(nbytes))
        if not p:
            raise RuntimeError(f"h264mi_engine_alloc({nbytes}) failed on device {self.device}")
        return int(p)

    def free(self, p: int) -> None:
        self._L.h264mi_engine_free(self._h, p)

    def upload(self, dst: int, src, nbytes: int) -> None:
        """H2D into memory of this engine's GPU (refused for another GPU's)."""
        if self._L.h264mi_engine_copy_h2d(self._h, dst, src, int(nbytes)) != 0:
            raise RuntimeError("h264mi_engine_copy_h2d failed (destination not on the engine's device?)")

    def pointer_device(self, p: int) -> int:
        return int(self._L.h264mi_pointer_device(p))

    def frame_ptr(self, stream: int, slot: int) -> int:
        """Device address of a frame slot (I420, chroma rows chroma_pitch
        bytes apart; slots slot_bytes apart)."""
        return int(self._L.h264mi_engine_frame_ptr(self._h, stream, slot))

    def sync(self) -> None:
        if self._L.h264mi_engine_sync(self._h) != 0:
            raise RuntimeError("h264mi_engine_sync failed")

    def kernel_name(self) -> str:
        """Reconstruction kernel of the last batch (diagnostics)."""
        return self._L.h264mi_engine_kernel(self._h).decode()

    def errors(self) -> int:
        return int(self._L.h264mi_engine_errors(self._h))

    def error_bits(self) -> int:
        """OR of the device flags of the pictures synced since the last call."""
        return int(self._L.h264mi_engine_error_bits(self._h))

    def rows_per_workgroup(self, npics: int) -> int:
        """MB rows per k_wgpp workgroup for a batch of npics pictures."""
        return int(self._L.h264mi_engine_rows_per_workgroup(self._h, npics))

    def last_timing_us(self):
        v = (C.c_float * 2)()
        if self._L.h264mi_engine_last_timing(self._h, v) != 0:
            return None
        return float(v[0]), float(v[1])

    def set_timing(self, max_batches: int, stride: int = 1) -> None:
        """HIP-event timing of up to max_batches launches, every stride-th one."""
        if self._L.h264mi_engine_set_timing(self._h, int(max_batches)) != 0:
            raise RuntimeError("h264mi_engine_set_timing failed")
        if self._L.h264mi_engine_set_timing_stride(self._h, int(stride)) != 0:
            raise RuntimeError("h264mi_engine_set_timing_stride failed")

    def timing_list(self, cap: int = 4096):
        """k_wgpp duration (us) of every recorded launch, in order."""
        if not hasattr(self._L, "h264mi_engine_timing_list"):
            return None
        v = (C.c_double * cap)()
        n = self._L.h264mi_engine_timing_list(self._h, v, int(cap))
        if n < 0:
            return None
        return [float(v[i]) for i in range(n)]

    def timing_report(self):
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        if self._L.h264mi_engine_timing_report(self._h, C.byref(a), C.byref(b), C.byref(n)) != 0:
            return None
        return a.value, b.value, n.value

    def close(self):
        if self._h:
            self._L.h264mi_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
