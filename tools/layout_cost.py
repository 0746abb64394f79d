"""Diagnostics (not a test): what the interleaved (channels-last) layout of the
RGB tensor exports costs against the planar export, and against
what a caller does today for a channels-last tensor -- the planar export
followed by torch's conversion.  One process, device events, warm-up, legs
alternating; writes profiles/layout_cost.json (or the path given).
Conventions of tools/letterbox_cost.py.

Three workloads, those of tools/tensor_cost.py, letterbox_cost.py and
rois_cost.py, all RGB fp16, scale 1/255:
  plain_8x1080p   eight 1920x1080 windows of 1920x1088 frame slots, unresized
  letterbox_640   one such window letterboxed into a 640x640 canvas, pad 114
  rois_32         rois_cost.py's 32 boxes on eight pictures into 224x224
and three legs on each:
  <w>/nhwc           h264mi_tensor_layout_device_pitch, INTERLEAVED: one launch
  <w>/nchw           the existing planar call
  <w>/nchw_convert   the planar call, then torch's copy_ of the result into a
                     preallocated channels_last tensor
The bar: on each workload nhwc's median is no longer than nchw_convert's.  The
ratio nhwc / nchw is reported with medians and IQRs; it is not a bar.
Consecutive repetitions rotate through NSETS input and output buffer sets.
Before anything is timed the outputs are compared: nhwc must equal nchw as
tensors (torch.equal on the logical shape) and nchw_convert's channels_last
tensor byte for byte.

A sample is the device time between two events around REPS repetitions of a
leg, so it holds what the host's enqueue rate leaves idle on the device too --
what a caller sees.  host_enqueue_us is the host's own time to queue one
repetition (no synchronisation inside).

Usage: python tools/layout_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import empty_layout, fit_desc, layout_desc, rois_desc, tensor_desc  # noqa: E402
from rois_cost import BOXES, CH, CW, H, NP, W, stats  # noqa: E402

SAMPLES, REPS, NSETS = 15, 40, 6
CANVAS = (640, 640)                                     # (oh, ow) of letterbox_640
SIZE = (224, 224)                                       # (oh, ow) of rois_32
PAD = 114


def main():
    import torch
    assert torch.cuda.is_available(), "layout_cost.py measures on the GPU"
    L = _lib.mi()
    dev = torch.device("cuda")
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    zero = (C.c_size_t * 1)(0)
    st = torch.cuda.current_stream().cuda_stream
    window = (0, 0, CW, CH)

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    def bufs(shape):
        """per buffer set: the nhwc result, the planar result, the channels_last tensor torch converts into"""
        return ([empty_layout(shape, torch.float16, dev, "nhwc").zero_() for _ in range(NSETS)],
                [torch.zeros(shape, dtype=torch.float16, device=dev) for _ in range(NSETS)],
                [empty_layout(shape, torch.float16, dev, "nhwc").zero_() for _ in range(NSETS)])

    legs, outs = {}, {}

    def workload(name, shape, npics, offsets, planar_call, planar_desc, boxes):
        o_hwc, o_pl, o_cv = outs[name] = bufs(shape)
        ld = layout_desc(planar_desc, "nhwc")
        stride = shape[1] * shape[2] * shape[3] * 2
        nb = len(boxes) if boxes is not None else 0
        extra = (boxes, nb) if boxes is not None else ()

        def nhwc(i):
            chk(L.h264mi_tensor_layout_device_pitch(d_in[i].data_ptr(), offsets, npics, W, H, cpitch, C.byref(ld), boxes,
                                                    nb, o_hwc[i].data_ptr(), stride, st))

        def nchw(i):
            chk(planar_call(d_in[i].data_ptr(), offsets, npics, W, H, cpitch, C.byref(planar_desc), *extra,
                            o_pl[i].data_ptr(), stride, st))

        def nchw_convert(i):
            nchw(i)
            o_cv[i].copy_(o_pl[i])

        legs[name + "/nhwc"], legs[name + "/nchw"], legs[name + "/nchw_convert"] = nhwc, nchw, nchw_convert

    tdesc, planes, _ = tensor_desc(window, "rgb", torch.float16)
    workload("plain_8x1080p", (NP, 3, CH, CW), NP, offs, L.h264mi_tensor_device_pitch, tdesc, None)
    rdesc = tensor_desc(window, "rgb", torch.float16, size=CANVAS)[0]
    workload("letterbox_640", (1, 3) + CANVAS, 1, zero, L.h264mi_tensor_fit_device_pitch,
             fit_desc(rdesc, planes, "letterbox", PAD), None)
    sdesc, arr, _, _ = rois_desc(BOXES, SIZE, NP, W, H, "rgb", torch.float16)
    workload("rois_32", (len(BOXES), 3) + SIZE, NP, offs, L.h264mi_tensor_rois_device_pitch, sdesc, arr)

    for f in legs.values():                             # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    same = {}
    for name, (o_hwc, o_pl, o_cv) in outs.items():
        same[name + "_nhwc_equals_nchw"] = all(torch.equal(a, b) for a, b in zip(o_hwc, o_pl)) and bool(o_pl[0].any())
        same[name + "_nhwc_bytes_equal_torch_conversion"] = all(
            a.stride() == b.stride() and torch.equal(a.permute(0, 2, 3, 1).contiguous().view(torch.uint8),
                                                     b.permute(0, 2, 3, 1).contiguous().view(torch.uint8))
            for a, b in zip(o_hwc, o_cv))
    assert all(same.values()), f"different bytes: {same}"

    us = {k: [] for k in legs}
    host = {k: [] for k in legs}
    for _ in range(SAMPLES):
        for k, f in legs.items():                       # alternating, same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for r in range(REPS):
                f(r % NSETS)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
            host[k].append((t1 - t0) * 1e6 / REPS)
    res = {"shape": {"coded": [W, H], "window": list(window), "mode": "rgb", "dtype": "float16",
                     "plain_8x1080p": {"pictures": NP},
                     "letterbox_640": {"canvas_oh_ow": list(CANVAS), "pad": PAD},
                     "rois_32": {"pictures": NP, "size_oh_ow": list(SIZE), "boxes": len(BOXES)},
                     "samples": SAMPLES, "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "outputs_identical": same, "legs": {}, "bar": {}, "nhwc_over_nchw": {}}
    for k in legs:
        s = stats(us[k])
        s["host_enqueue_us"] = round(statistics.median(host[k]), 2)
        res["legs"][k] = s
    for name in outs:
        a, b, c = (res["legs"][f"{name}/{leg}"] for leg in ("nhwc", "nchw", "nchw_convert"))
        res["bar"][name] = {"nhwc_median_us": a["median_us"], "nchw_convert_median_us": c["median_us"],
                            "nhwc_over_nchw_convert": round(a["median_us"] / c["median_us"], 3),
                            "meets_bar": bool(a["median_us"] <= c["median_us"])}
        res["nhwc_over_nchw"][name] = {"nhwc_median_us": a["median_us"], "nhwc_iqr_us": a["iqr_us"],
                                       "nchw_median_us": b["median_us"], "nchw_iqr_us": b["iqr_us"],
                                       "ratio": round(a["median_us"] / b["median_us"], 3)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layout_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
