"""Host-side mirror of Broadway's JavaScript decoder API.

``Decoder(options).decode(nal, info)`` -> ``onPictureDecoded(buffer, width,
height, infos)`` with the semantics of templates/DecoderPost.js:55-285 on top
of the wasm glue of Decoder/src/Decoder.c:44-162:

* ``decode`` copies the input into the decoder's stream buffer (a 1 MiB heap
  buffer in the reference, DecoderPost.js:152/:283) and runs synchronously;
* ``onPictureDecoded`` receives the MB-aligned planar I420 picture
  (``width*height*3/2`` bytes, width/height multiples of 16, not cropped --
  H264SwDecApi.c:233-234; see ``crop`` below) plus the ``infos`` collected
  since the last picture with ``startDecoding``/``finishDecoding`` stamps (DecoderPost.js:77-103);
* after a picture completes, the rest of the buffer is dropped
  (Decoder.c:122-134) and the DPB is never flushed (Decoder.c:140), so
  pictures held for display reordering are not emitted.

* ``rgb: true`` (DecoderPost.js:82-97): ``onPictureDecoded`` receives a new
  RGBA array (``width*height*4`` bytes) converted on the GPU with the
  reference converter's per-pixel arithmetic (yuv2rgbcalc, :514-560) --
  ``H264SwDecNextPictureRGBA`` instead of ``H264SwDecNextPicture``.

* ``crop: true`` (an extension; the reference leaves cropping to its callers:
  DecTestBench -C, Player/YUVCanvas.js croppingParams): every picture is
  cropped to the SPS crop window on the GPU (``H264SwDecNextPictureCropped``)
  and ``onPictureDecoded(buffer, cropOutWidth, cropOutHeight, infos)`` receives
  a new packed array of ``cropOutWidth*cropOutHeight*3/2`` bytes -- or, with
  ``rgb: true`` as well, ``*4`` bytes of RGBA.  A stream without a crop window
  delivers the whole picture.

* ``tensor: true`` or ``tensor: {"dtype": ..., "mode": ..., "mean": ...,
  "std": ..., "scale": ..., "bias": ..., "size": (oh, ow), "filter": ...}`` (an extension for
  device consumers; needs torch, imported only on this path): nothing is
  copied to the host.
  ``onPictureDecoded(tensor, width, height, infos)`` receives a new
  ``(planes, height, width)`` torch tensor on the decoder's GPU, cropped to the
  SPS crop window, built by ``H264SwDecNextPictureTensor`` on torch's current
  stream -- the arguments of ``Engine.to_tensor`` (default: RGB, float16,
  scale 1/255).  With ``size`` the crop window is resized on the GPU
  (``H264SwDecNextPictureTensorResized``; with ``"fit": "letterbox" |
  "topleft" | "stretch"`` and ``"pad": 114 | (r, g, b)`` it is fitted into
  the canvas ``size`` with its aspect ratio kept and the rest padded,
  ``H264SwDecNextPictureTensorFit``): the tensor is ``(planes, oh, ow)``
  and the callback's width and height are ``ow`` and ``oh``; ``"filter":
  "bicubic"`` (with ``size``) resizes with the antialiased bicubic filter
  instead of the triangle (``Engine.to_tensor``).  It combines with
  neither ``rgb`` nor ``crop`` (ValueError).  ``colour`` picks the colour set
  of the R, G, B samples: "reference" (the default: BT.601 limited range, the
  values of ``rgb: true``), "bt601-full", "bt709", "bt709-full", or "stream"
  -- the set the VUI of each delivered picture's own SPS names
  (matrix_coefficients 1: BT.709; 5, 6: BT.601; video_full_range_flag), and
  where it names none the family of ``unspecified``: "bt601" (default),
  "bt709" or "size" (BT.709 from 1280 columns or 577 rows of the exported
  window).  ``decoder.tensor_colour`` names the set of the last tensor.
  ``"clip": T`` (with ``"step": s``, default 1; combines with every key
  above): the pictures as video clips.  Every s-th delivered picture is
  written in place into the current ``(planes, T, h, w)`` clip
  (``H264SwDecNextPictureTensorDest``) -- ``onPictureDecoded``
  still fires for it, with the strided view ``clip[:, t]`` -- and after the
  T-th ``onClipDecoded(clip, width, height)`` fires and a new clip is
  allocated; the pictures in between are taken and dropped.  A clip is
  contiguous (``layout: "nhwc"``: channels-last per frame), so a batch of them
  is NCTHW.  An incomplete last clip is not emitted: ``decoder.clip_fill`` is
  the number of pictures it holds.

* ``mbinfo: true`` or ``mbinfo: {"channels": ..., "dtype": ..., "scale": ...,
  "bias": ...}`` (an extension for device consumers; needs torch; combines
  with every output mode above): the decoder keeps each picture's MB records
  on the GPU, and before every ``onPictureDecoded`` call ``decoder.mbinfo`` is
  a new ``(C, bh, bw)`` torch tensor on the decoder's GPU -- the delivered
  picture's motion vectors and MB side information, one element per luma 4x4
  block covering the SPS crop window, built by ``H264SwDecLastPictureMbInfo``
  on torch's current stream; the arguments of ``Engine.to_mbinfo`` (default:
  channels ("mvx", "mvy"), int16).

* ``residual: true`` or ``residual: {"planes": ..., "dtype": ..., "scale": ...,
  "bias": ...}`` (an extension for device consumers; needs torch; combines
  with every output mode above and with ``mbinfo``): the decoder keeps each
  picture's coefficient blocks and records on the GPU, and before every
  ``onPictureDecoded`` call ``decoder.residual`` is a new ``(1 | 2 | 3, rows,
  columns)`` torch tensor on the decoder's GPU -- the delivered picture's
  decoded residual over the SPS crop window ("uv": half of it each way; the
  window must then be even), built by ``H264SwDecLastPictureResidual`` on
  torch's current stream; the arguments of ``Engine.to_residual`` (default:
  planes "y", int16).

* ``accmv: true`` or ``accmv: {"channels": ..., "dtype": ..., "scale": ...,
  "bias": ...}`` (an extension for device consumers; needs torch; combines
  with every output mode above and with ``mbinfo`` and ``residual``): the
  decoder keeps each picture's origin map on the GPU -- every luma sample
  traced back, through the pictures it was predicted from, to its position in
  the key picture of its GOP --, and before every ``onPictureDecoded`` call
  ``decoder.accmv`` is a new ``(C, ch, cw)`` torch tensor on the decoder's GPU
  -- the delivered picture's accumulated motion over the SPS crop window,
  built by ``H264SwDecLastPictureAccMotion`` on torch's current stream; the
  arguments of ``Engine.to_accmv`` (default: channels ("adx", "ady"), int16).
  With ``"size": (oh, ow)`` the field is resized on the GPU
  (``H264SwDecLastPictureAccMotionResized``) and ``decoder.accmv`` is ``(C, oh,
  ow)``.

* ``decoder.rois(boxes, size, ...)`` (an extension for device consumers; needs
  torch; no option: callable in every output mode, inside ``onPictureDecoded``
  and until the next ``decode``): boxes ``(x, y, cw, ch)`` of the delivered
  picture, in the coordinates of the SPS crop window, each resized on the GPU
  to ``size`` = (oh, ow) -- a new ``(K, planes, oh, ow)`` torch tensor on the
  decoder's GPU, built by ``H264SwDecLastPictureTensorRois`` on torch's current
  stream from one kernel launch per 32 boxes; the arguments of the ``tensor``
  option.

Unlike the reference module (a single global instance) every ``Decoder`` has
its own H264SwDec instance, so several streams can be decoded side by side.
Reconstruction always runs on the GPU through libh264mi.so; ``sliceMode``
(per-slice web workers) is not supported.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from . import _lib

STREAM_BUFFER_SIZE = 1024 * 1024


def _now() -> float:
    return time.perf_counter() * 1000.0


class _Field(NamedTuple):
    """A field export of the delivered picture (the option of its name)."""
    build: str              # its descriptor builder in .engine
    first: str              # the builder's first argument as an option key (the others: dtype, scale, bias)
    default: object         # and its default
    keep: str               # the H264SwDecKeep* call
    last: str               # the H264SwDecLastPicture* call
    shape: Callable         # (rows, columns) of (descriptor, x, y, cw, ch): what `last` covers of the crop window
    kept: str               # what the backend keeps for it (the error text of `keep`)
    what: str               # what it exports (the error text of `last`)
    resized: Optional[str] = None       # the H264SwDecLastPicture*Resized call of its `size` key (None: it has none)


# in the order __init__ takes the options; _emit exports in the reverse order
_FIELDS = {
    "mbinfo": _Field("mbinfo_desc", "channels", ("mvx", "mvy"), "H264SwDecKeepMbInfo", "H264SwDecLastPictureMbInfo",
                     lambda d, x, y, cw, ch: (((y + ch + 3) >> 2) - (y >> 2), ((x + cw + 3) >> 2) - (x >> 2)),
                     "MB records", "the MB records"),
    "residual": _Field("residual_desc", "planes", "y", "H264SwDecKeepResidual", "H264SwDecLastPictureResidual",
                       lambda d, x, y, cw, ch: tuple(v >> (d.planes == _lib.RESID_PLANES["uv"]) for v in (ch, cw)),
                       "coefficients", "the residual"),
    "accmv": _Field("accmv_desc", "channels", ("adx", "ady"), "H264SwDecKeepAccMotion", "H264SwDecLastPictureAccMotion",
                    lambda d, x, y, cw, ch: (ch, cw), "origin maps", "the origin map",
                    "H264SwDecLastPictureAccMotionResized"),
}


def rois_args(boxes, size, width, height, **kw):
    """``Decoder.rois``'s arguments as (descriptor, ``_lib.Roi`` array, planes,
    torch dtype): ``boxes`` = [(x, y, cw, ch), ...] on a delivered picture of
    width x height (0: no headers yet, so only the picture-independent rules
    are checked here), all of picture 0; ``kw``: the ``tensor`` option's keys.
    ValueError for anything the library would refuse."""
    from .engine import rois_desc                # (imports torch)
    try:
        boxes = [(0,) + tuple(b) for b in boxes]
    except TypeError:
        raise ValueError(f"rois: boxes {boxes!r}: a list of (x, y, cw, ch)") from None
    return rois_desc(boxes, size, 1, width or _lib.RESIZE_MAX_DIM, height or _lib.RESIZE_MAX_DIM, stream_ok=True, **kw)


def warps_args(mats, size, window, width, height, **kw):
    """``Decoder.warps``'s arguments as (descriptor, ``_lib.Warp`` array, planes,
    torch dtype): ``mats`` = [(m0, ..., m5), ...], all of picture 0, over
    ``window`` of a delivered picture of width x height (0: no headers yet);
    ``kw``: the ``tensor`` option's keys, ``border``, ``pad`` and ``layout``.
    ValueError for anything the library would refuse."""
    from .engine import warps_desc               # (imports torch)
    try:
        mats = [(0, tuple(m)) for m in mats]
    except TypeError:
        raise ValueError(f"warps: {mats!r}: a list of (m0, m1, m2, m3, m4, m5)") from None
    return warps_desc(mats, size, 1, window, width, height, stream_ok=True, **kw)


class Decoder:
    def __init__(self, options: Optional[dict] = None):
        self.options = dict(options or {})
        if self.options.get("sliceMode"):
            raise NotImplementedError("sliceMode (per-slice workers) is not part of the MI355X path")
        self._rgb = bool(self.options.get("rgb"))
        self._crop = bool(self.options.get("crop"))
        self._tensor = self.options.get("tensor") or None
        self._resized = self._fitted = False
        if self._tensor is not None:
            if self._rgb or self._crop:
                raise ValueError("tensor: not combinable with rgb or crop (mode='rgb' and the SPS window are part of it)")
            opts = {} if self._tensor is True else dict(self._tensor)
            unknown = set(opts) - {"dtype", "mode", "mean", "std", "scale", "bias", "size", "colour", "unspecified",
                                   "fit", "pad", "layout", "filter", "clip", "step"}
            if unknown:
                raise ValueError(f"tensor: unknown keys {sorted(unknown)}")
            from .engine import fit_desc, layout_desc, tensor_desc, tensor_layout       # (imports torch)
            fit, pad = opts.pop("fit", None), opts.pop("pad", None)
            self._clip_t, self._clip_step = opts.pop("clip", None), opts.pop("step", None)
            if self._clip_step is not None and self._clip_t is None:
                raise ValueError("tensor: step goes with clip")
            for what, v in (("clip", self._clip_t), ("step", self._clip_step)):
                if v is not None and (not isinstance(v, int) or isinstance(v, bool) or v < 1):
                    raise ValueError(f"tensor: {what} {v!r}: a positive integer")
            self._clip_step = self._clip_step or 1
            self._layout = opts.pop("layout", "nchw")
            tensor_layout(self._layout)
            self._tensor = tensor_desc(None, stream_ok=True, **opts)
            self._resized = opts.get("size") is not None
            self._fitted = fit is not None or pad is not None
            if self._fitted:
                if not self._resized:
                    raise ValueError("tensor: fit and pad go with size=(oh, ow), the canvas")
                desc, planes, dtype = self._tensor
                self._tensor = (fit_desc(desc, planes, "letterbox" if fit is None else fit, 114 if pad is None else pad),
                                planes, dtype)
            # "nhwc": the same descriptor under a layout, through the one call that takes it
            self._tensor_layout = layout_desc(self._tensor[0], self._layout) if self._layout != "nchw" else None
            self._device = int(os.environ.get("H264MI_DEVICE") or 0)     # the GPU H264SwDecInit takes (api.c)
            if self._clip_t is not None:
                self._clip_desc = self._tensor_layout or layout_desc(self._tensor[0], "nchw")
        self._fields = {}           # option -> (descriptor, channels or planes, torch dtype) of the fields asked for
        for name, f in _FIELDS.items():
            setattr(self, name, None)
            opts = self.options.get(name) or None
            if opts is not None:
                opts = {} if opts is True else dict(opts)
                unknown = set(opts) - {f.first, "dtype", "scale", "bias"} - ({"size"} if f.resized else set())
                if unknown:
                    raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
                from . import engine                 # (imports torch)
                self._fields[name] = getattr(engine, f.build)(opts.pop(f.first, f.default), None, **opts)
                self._device = int(os.environ.get("H264MI_DEVICE") or 0)
        self._L = _lib.mi()
        inst = C.c_void_p()
        ret = self._L.H264SwDecInit(C.byref(inst), 0)
        if ret != _lib.H264SWDEC_OK:
            raise RuntimeError(f"DECODER INITIALIZATION FAILED ({ret})")
        self._inst = inst
        for name in self._fields:
            f = _FIELDS[name]
            if not hasattr(self._L, f.keep) or getattr(self._L, f.keep)(inst, 1) != _lib.H264SWDEC_OK:
                self.close()
                raise RuntimeError(f"{name}: the backend cannot keep {f.kept} (there is no host fallback)")
        self._buf = (C.c_uint8 * STREAM_BUFFER_SIZE)()
        self._info = _lib.H264SwDecInfo()
        self._pic = _lib.H264SwDecPicture()
        self.infoAr: List[dict] = []
        self.pic_decode_number = 1
        self.pic_display_number = 1
        self.onPictureDecoded: Callable = lambda buffer, width, height, infos: None
        self.onHeadersDecoded: Callable = lambda: None
        # the `clip` key of the tensor option: the clip being filled, the pictures it holds, the pictures delivered
        self.onClipDecoded: Callable = lambda clip, width, height: None
        self._clip = None
        self.clip_fill = 0
        self._clip_seen = 0

    # DecoderPost.js:275-285 + Decoder.c:44-53
    def decode(self, typed_ar, par_info: Optional[dict] = None) -> None:
        data = bytes(typed_ar)
        if len(data) > STREAM_BUFFER_SIZE:
            raise ValueError("NAL larger than the 1 MiB stream buffer (DecoderPost.js:152)")
        if par_info is not None:
            self.infoAr.append(par_info)
            par_info["startDecoding"] = _now()
        C.memmove(self._buf, data, len(data))
        inp = _lib.H264SwDecInput()
        out = _lib.H264SwDecOutput()
        inp.pStream = C.cast(self._buf, C.POINTER(C.c_uint8))
        inp.dataLen = len(data)
        base = C.addressof(self._buf)
        while inp.dataLen > 0:
            self._decode_once(inp, out, base)

    # Decoder.c:100-162
    def _decode_once(self, inp, out, base) -> int:
        L = self._L
        inp.picId = self.pic_decode_number
        ret = L.H264SwDecDecode(self._inst, C.byref(inp), C.byref(out))

        def consumed() -> int:
            return C.cast(out.pStrmCurrPos, C.c_void_p).value - C.cast(inp.pStream, C.c_void_p).value

        if ret == _lib.H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY:
            if L.H264SwDecGetInfo(self._inst, C.byref(self._info)) != _lib.H264SWDEC_OK:
                return -1
            self.onHeadersDecoded()
            n = consumed()
            inp.dataLen -= n
            inp.pStream = out.pStrmCurrPos
        elif ret in (_lib.H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY, _lib.H264SWDEC_PIC_RDY):
            inp.dataLen = 0
            self.pic_decode_number += 1
            while True:
                if self._tensor is not None and self._clip_t is not None:
                    if not self._next_into_clip():
                        break
                elif self._tensor is not None:
                    desc, planes, dtype = self._tensor
                    w, h = self._out_size()
                    out, st = self._device_empty((planes, h, w), dtype, self._layout)
                    nxt = getattr(L, "H264SwDecNextPictureTensorLayout" if self._tensor_layout is not None else
                                  "H264SwDecNextPictureTensorFit" if self._fitted else
                                  "H264SwDecNextPictureTensorResized" if self._resized else "H264SwDecNextPictureTensor", None)
                    if self._tensor_layout is not None:
                        desc = self._tensor_layout
                    ret = nxt(self._inst, C.byref(self._pic), 0, C.byref(desc), out.data_ptr(), st) if nxt else \
                        _lib.H264SWDEC_PARAM_ERR
                    if ret == _lib.H264SWDEC_PARAM_ERR:
                        raise RuntimeError("tensor: the backend cannot export device tensors "
                                           "(there is no host fallback)")
                    if ret != _lib.H264SWDEC_PIC_RDY:
                        break
                    self.pic_display_number += 1
                    self._emit(self._pic, out)
                elif self._crop:
                    w, h = self._out_size()
                    out = np.empty(w * h * 4 if self._rgb else w * h * 3 // 2, dtype=np.uint8)
                    ret = L.H264SwDecNextPictureCropped(self._inst, C.byref(self._pic), 0, out.ctypes.data,
                                                        int(self._rgb))
                    if ret == _lib.H264SWDEC_PARAM_ERR:
                        raise RuntimeError("crop: the backend cannot crop (there is no host fallback)")
                    if ret != _lib.H264SWDEC_PIC_RDY:
                        break
                    self.pic_display_number += 1
                    self._emit(self._pic, out)
                elif self._rgb:
                    w, h = self._info.picWidth, self._info.picHeight
                    rgba = np.empty(w * h * 4, dtype=np.uint8)
                    if L.H264SwDecNextPictureRGBA(self._inst, C.byref(self._pic), 0,
                                                  rgba.ctypes.data) != _lib.H264SWDEC_PIC_RDY:
                        break
                    self.pic_display_number += 1
                    self._emit(self._pic, rgba)
                else:
                    if L.H264SwDecNextPicture(self._inst, C.byref(self._pic), 0) != _lib.H264SWDEC_PIC_RDY:
                        break
                    self.pic_display_number += 1
                    self._emit(self._pic)
        elif ret in (_lib.H264SWDEC_STRM_PROCESSED, _lib.H264SWDEC_STRM_ERR):
            inp.dataLen = 0
        return ret

    def _next_into_clip(self) -> bool:
        """The next delivered picture under ``tensor: {"clip": T, "step": s}``:
        every s-th one is written in place into frame ``clip_fill`` of the
        current ``(planes, T, h, w)`` clip (H264SwDecNextPictureTensorDest:
        the frame's strides are the destination) and handed to
        onPictureDecoded as that view; the T-th completes the clip, which goes
        to onClipDecoded, and the next picture starts a new one.  The pictures
        in between are taken with H264SwDecNextPicture and dropped.  False:
        no picture was ready."""
        L = self._L
        if self._clip_seen % self._clip_step:
            if L.H264SwDecNextPicture(self._inst, C.byref(self._pic), 0) != _lib.H264SWDEC_PIC_RDY:
                return False
            self._clip_seen += 1
            self.pic_display_number += 1
            return True
        import torch
        from .engine import dest_of_view, empty_clip
        _, planes, dtype = self._tensor
        w, h = self._out_size()
        dev = torch.device("cuda", self._device)
        if self._clip is None or tuple(self._clip.shape) != (planes, self._clip_t, h, w):
            with torch.cuda.device(dev):
                self._clip = empty_clip((1, planes, self._clip_t, h, w), dtype, dev, self._layout)[0]
            self.clip_fill = 0
        view = self._clip[:, self.clip_fill]
        dest, _ = dest_of_view(view[None], (1, planes, h, w), dtype, dev, self._layout)
        nxt = getattr(L, "H264SwDecNextPictureTensorDest", None)
        ret = nxt(self._inst, C.byref(self._pic), 0, C.byref(self._clip_desc), C.byref(dest), view.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream) if nxt else _lib.H264SWDEC_PARAM_ERR
        if ret == _lib.H264SWDEC_PARAM_ERR:
            raise RuntimeError("tensor: the backend cannot export into a clip (there is no host fallback)")
        if ret != _lib.H264SWDEC_PIC_RDY:
            return False
        self._clip_seen += 1
        self.pic_display_number += 1
        self.clip_fill += 1
        self._emit(self._pic, view)
        if self.clip_fill == self._clip_t:
            clip, self._clip, self.clip_fill = self._clip, None, 0
            self.onClipDecoded(clip, w, h)
        return True

    def _out_size(self):
        """(width, height) of the pictures handed to onPictureDecoded."""
        i = self._info
        if self._tensor is not None and self._resized:
            r = self._tensor[0].r if self._fitted else self._tensor[0]
            return r.ow, r.oh
        if (self._crop or self._tensor is not None) and i.croppingFlag:
            return i.cropParams.cropOutWidth, i.cropParams.cropOutHeight
        return i.picWidth, i.picHeight

    def _device_empty(self, shape, dtype, layout="nchw"):
        """(a new tensor on the decoder's GPU, torch's current stream there as a HIP handle)."""
        import torch
        dev = torch.device("cuda", self._device)
        with torch.cuda.device(dev):
            if layout != "nchw":
                from .engine import empty_layout
                return empty_layout(shape, dtype, dev, layout), torch.cuda.current_stream(dev).cuda_stream
            return torch.empty(shape, dtype=dtype, device=dev), torch.cuda.current_stream(dev).cuda_stream

    def _crop_window(self):
        """(x, y, cw, ch) of the active SPS's crop window (the whole picture without one)."""
        i = self._info
        if not i.croppingFlag:
            return 0, 0, i.picWidth, i.picHeight
        return (i.cropParams.cropLeftOffset, i.cropParams.cropTopOffset, i.cropParams.cropOutWidth,
                i.cropParams.cropOutHeight)

    def _export_field(self, name):
        """The delivered picture's field of that option over the crop window
        (the window its H264SwDecLastPicture* call takes for a descriptor
        without one; mbinfo: the blocks covering it)."""
        f = _FIELDS[name]
        desc, n, dtype = self._fields[name]
        resized = hasattr(desc, "oh")           # the option's `size`: a resize descriptor
        out, st = self._device_empty((n,) + ((desc.oh, desc.ow) if resized else f.shape(desc, *self._crop_window())),
                                     dtype)
        last = getattr(self._L, f.resized if resized else f.last, None)
        ret = last(self._inst, C.byref(desc), out.data_ptr(), st) if last else _lib.H264SWDEC_PARAM_ERR
        if ret != _lib.H264SWDEC_PIC_RDY:
            raise RuntimeError(f"{name}: the backend cannot export {f.what} ({ret}; there is no host fallback)")
        return out

    def _emit(self, pic, rgba=None) -> None:
        for name in reversed(self._fields):
            setattr(self, name, self._export_field(name))
        w, h = self._out_size()
        if rgba is not None:
            buf = rgba
        else:
            n = w * h * 3 // 2
            buf = np.ctypeslib.as_array(C.cast(pic.pOutputPicture, C.POINTER(C.c_uint8)), shape=(n,))
        infos = None
        if self.infoAr:
            infos = self.infoAr
            infos[0]["finishDecoding"] = _now()
        self.infoAr = []
        self.onPictureDecoded(buf, w, h, infos)

    def rois(self, boxes, size, mode="rgb", dtype=None, mean=None, std=None, scale=None, bias=None, colour=None,
             unspecified=None, fit=None, pad=None, layout="nchw", filter=None):
        """Boxes of the delivered picture as one new ``(K, planes, oh, ow)``
        torch tensor on the decoder's GPU, on torch's current stream
        (``H264SwDecLastPictureTensorRois``): ``boxes`` = [(x, y, cw, ch), ...]
        in the coordinates of the picture ``onPictureDecoded`` receives with
        ``crop`` or ``tensor`` (the SPS crop window; the whole picture where
        the stream has none), every box even, inside it and resized to ``size``
        = (oh, ow).  Callable inside ``onPictureDecoded`` and until the next
        ``decode``, in every output mode; needs torch.  The other arguments
        are those of the ``tensor`` option; ``colour="stream"`` gives every
        box the set the whole-picture tensor of that picture gets, and
        ``tensor_colour`` names it.  With ``fit`` ("letterbox", "topleft" or
        "stretch") and ``pad`` every box is fitted into ``size`` with its
        aspect ratio kept (``H264SwDecLastPictureTensorRoisFit``), as for
        ``Engine.to_tensor``.  ``layout="nhwc"``: the same values stored
        channels-last (``H264SwDecLastPictureTensorRoisLayout``), the result
        of the usual shape with channels_last strides.  ``filter="bicubic"``:
        every box through the antialiased bicubic filter (``Engine.to_tensor``)
        instead of the triangle.  ValueError for a bad argument,
        RuntimeError before a picture was delivered."""
        from .engine import layout_desc, tensor_layout
        nhwc = tensor_layout(layout) != 0
        _, _, cw, ch = self._crop_window()
        desc, arr, planes, dtype = rois_args(boxes, size, cw, ch, mode=mode, dtype=dtype, mean=mean, std=std, scale=scale,
                                             bias=bias, colour=colour, unspecified=unspecified, fit=fit, pad=pad,
                                             filter=filter)
        if not hasattr(self, "_device"):
            self._device = int(os.environ.get("H264MI_DEVICE") or 0)
        fitted = fit is not None or pad is not None
        r = desc.r if fitted else desc
        out, st = self._device_empty((len(arr), planes, r.oh, r.ow), dtype, layout)
        last = getattr(self._L, "H264SwDecLastPictureTensorRoisLayout" if nhwc else
                       "H264SwDecLastPictureTensorRoisFit" if fitted else "H264SwDecLastPictureTensorRois", None)
        if nhwc:
            desc = layout_desc(desc, layout)
        ret = last(self._inst, C.byref(desc), arr, len(arr), out.data_ptr(), st) if last else _lib.H264SWDEC_PARAM_ERR
        if ret == _lib.H264SWDEC_OK:
            raise RuntimeError("rois: no picture has been delivered since the last decode")
        if ret != _lib.H264SWDEC_PIC_RDY:
            raise RuntimeError(f"rois: the backend cannot export the boxes ({ret}; there is no host fallback)")
        return out

    def warps(self, mats, size, window=None, mode="rgb", dtype=None, mean=None, std=None, scale=None, bias=None,
              colour=None, unspecified=None, border=None, pad=None, layout="nchw"):
        """Affine warps of the delivered picture as one new ``(K, planes, oh,
        ow)`` torch tensor on the decoder's GPU, on torch's current stream
        (``H264SwDecLastPictureTensorWarps``): ``mats`` = [(m0, ..., m5), ...],
        the Q16 inverse maps of ``Engine.to_tensor(warps=)``
        (``engine.warp_q16``, ``engine.rotated_box_warp``), in the coordinates
        of ``window`` = (x, y, cw, ch) -- even, inside the picture
        ``onPictureDecoded`` receives with ``crop`` or ``tensor``; None: all of
        it.  No tap reads outside that window, so a crop's padding rows never
        show: ``border="constant"`` (default) gives ``pad`` there (default 0),
        "replicate" the window's edge.  Callable when ``rois`` is; the other
        arguments are those of the ``tensor`` option.  ValueError for a bad
        argument, RuntimeError before a picture was delivered."""
        _, _, cw, ch = self._crop_window()
        desc, arr, planes, dtype = warps_args(mats, size, window, cw, ch, mode=mode, dtype=dtype, mean=mean, std=std,
                                              scale=scale, bias=bias, colour=colour, unspecified=unspecified, border=border,
                                              pad=pad, layout=layout)
        if not hasattr(self, "_device"):
            self._device = int(os.environ.get("H264MI_DEVICE") or 0)
        out, st = self._device_empty((len(arr), planes, desc.oh, desc.ow), dtype, layout)
        last = getattr(self._L, "H264SwDecLastPictureTensorWarps", None)
        ret = last(self._inst, C.byref(desc), arr, len(arr), out.data_ptr(), st) if last else _lib.H264SWDEC_PARAM_ERR
        if ret == _lib.H264SWDEC_OK:
            raise RuntimeError("warps: no picture has been delivered since the last decode")
        if ret != _lib.H264SWDEC_PIC_RDY:
            raise RuntimeError(f"warps: the backend cannot export the warps ({ret}; there is no host fallback)")
        return out

    def stats(self, boxes=None, planes="y", hist=False, colour=None, window=None):
        """Statistics of the delivered picture as one new ``int64`` torch
        tensor of shape ``(K or 1, P, L)`` on the decoder's GPU, on torch's
        current stream (``H264SwDecLastPictureStats``; the picture is not
        exported): per box of ``boxes`` = [(x, y, cw, ch), ...], or for
        ``window`` (None: everything), both in the coordinates of the picture
        ``onPictureDecoded`` receives with ``crop`` or ``tensor``, even and
        inside it; ``planes``, ``hist`` and ``colour`` as for
        ``Engine.to_stats`` (``engine.stats_fields`` names the words), and
        ``colour="stream"`` takes the set the picture's VUI names, which
        ``tensor_colour`` then reports.  There is no reference picture here
        (sad and ssd are 0): compare consecutive histograms to detect a cut.
        Callable when ``rois`` is.  ValueError for a bad argument, RuntimeError
        before a picture was delivered."""
        import torch
        from .engine import stats_desc
        _, _, cw, ch = self._crop_window()
        try:
            rois = None if boxes is None else [(0,) + tuple(b) for b in boxes]
        except TypeError:
            raise ValueError(f"stats: boxes {boxes!r}: a list of (x, y, cw, ch)") from None
        desc, arr, P, L = stats_desc(planes, window, rois, hist, colour, 1, cw or None, ch or None, stream_ok=True)
        if not hasattr(self, "_device"):
            self._device = int(os.environ.get("H264MI_DEVICE") or 0)
        out, st = self._device_empty((len(arr) if arr is not None else 1, P, L), torch.int64)
        last = getattr(self._L, "H264SwDecLastPictureStats", None)
        ret = last(self._inst, C.byref(desc), arr, len(arr) if arr is not None else 0, out.data_ptr(), st) \
            if last else _lib.H264SWDEC_PARAM_ERR
        if ret == _lib.H264SWDEC_OK:
            raise RuntimeError("stats: no picture has been delivered since the last decode")
        if ret != _lib.H264SWDEC_PIC_RDY:
            raise RuntimeError(f"stats: the backend cannot take the statistics ({ret}; there is no host fallback)")
        return out

    @property
    def tensor_colour(self) -> Optional[str]:
        """The colour set of the last tensor delivered ("reference",
        "bt601-full", "bt709" or "bt709-full"); None before the first."""
        k = self._L.H264SwDecLastTensorColour(self._inst)
        return _lib.TENSOR_COLOUR_NAMES[k] if k >= 0 else None

    def info(self) -> _lib.H264SwDecInfo:
        return self._info

    def close(self) -> None:
        if self._inst:
            self._L.H264SwDecRelease(self._inst)
            self._inst = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_annexb(stream: bytes) -> List[bytes]:
    """Split an Annex-B stream into NAL units (with their start codes), the
    way Player/mp4.js feeds one NAL per decode() call."""
    out = []
    i, n = 0, len(stream)
    starts = []
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            s = i - 1 if i > 0 and stream[i - 1] == 0 else i
            starts.append(s)
            i += 3
        else:
            i += 1
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else n
        out.append(stream[s:e])
    return out
