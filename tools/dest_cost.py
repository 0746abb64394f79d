"""Diagnostics (not a test): what writing a pixel export straight into a strided
destination (h264mi_tensor_dest) costs against what a caller does
without it -- the contiguous export into a temporary, then torch's copy_ into
the preallocated strided destination.  One process, device events, warm-up,
legs alternating; writes profiles/dest_cost.json (or the path given).
Conventions of tools/layout_cost.py.

Three workloads, all RGB fp16, scale 1/255, on 1920x1088 frame slots:
  clips_2x16   32 windows of 1920x1080 (eight pictures, four times each) resized
               to 224x224 as two 16-frame clips, (2, 3, 16, 224, 224) contiguous
  tubes_8x4    rois_cost.py's 32 boxes into 224x224 as eight tubes of T = 4,
               (8, 3, 4, 224, 224) contiguous
  tile_640x360 one 1920x1080 window resized to 640x360 into tile (1, 2) of a
               2 x 4 canvas, (3, 720, 2560)
and two legs on each:
  <w>/dest         h264mi_tensor_dest_device_pitch: one launch per 32 items
  <w>/export_copy  the existing contiguous call into a temporary, then copy_ of
                   the temporary's permuted view (the tile: of the temporary)
                   into the destination
The bar: on each workload dest's median is no longer than export_copy's.
Consecutive repetitions rotate through NSETS input and output buffer sets.
Before anything is timed the two legs' destinations are compared: torch.equal.

A sample is the device time between two events around REPS repetitions of a
leg, so it holds what the host's enqueue rate leaves idle on the device too --
what a caller sees.  host_enqueue_us is the host's own time to queue one
repetition (no synchronisation inside).

Usage: python tools/dest_cost.py [out.json]"""
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
from broadway_amd.engine import dest_of_view, layout_desc, rois_desc, tensor_desc  # noqa: E402
from rois_cost import BOXES, CH, CW, H, NP, W, stats  # noqa: E402

SAMPLES, REPS, NSETS = 15, 40, 6
SIZE = (224, 224)                                       # (oh, ow) of the clips and tubes
CLIP_T, TUBE_T = 16, 4
TILE = (360, 640)                                       # (oh, ow) of a tile; the canvas holds 2 x 4 of them
TILE_AT = (1, 2)                                        # (row, column) of the tile written


def main():
    import torch
    assert torch.cuda.is_available(), "dest_cost.py measures on the GPU"
    L = _lib.mi()
    dev = torch.device("cuda")
    f16 = torch.float16
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    offs32 = (C.c_size_t * 32)(*[(k % NP) * slot for k in range(32)])
    zero = (C.c_size_t * 1)(0)
    st = torch.cuda.current_stream().cuda_stream
    window = (0, 0, CW, CH)

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, outs = {}, {}

    def workload(name, nitems, npics, offsets, old_call, desc, boxes, size, dst_shape, view_of, tmp_view):
        """dst_shape: the destination tensors; view_of(dst): the view of one the items are written through (4-D
        (n, 3, oh, ow) or 5-D (b, 3, t, oh, ow)); tmp_view(tmp): the temporary (n, 3, oh, ow) as that view's shape"""
        d_new = [torch.zeros(dst_shape, dtype=f16, device=dev) for _ in range(NSETS)]
        d_old = [torch.zeros(dst_shape, dtype=f16, device=dev) for _ in range(NSETS)]
        tmp = [torch.zeros((nitems, 3) + size, dtype=f16, device=dev) for _ in range(NSETS)]
        outs[name] = (d_new, d_old)
        ld = layout_desc(desc, "nchw")
        v0 = view_of(d_new[0])
        dest, out_stride = dest_of_view(v0, tuple(v0.shape), f16, v0.device)
        first = v0.data_ptr() - d_new[0].data_ptr()
        nb = len(boxes) if boxes is not None else 0
        extra = (boxes, nb) if boxes is not None else ()
        item = 3 * size[0] * size[1] * 2

        def new(i):
            chk(L.h264mi_tensor_dest_device_pitch(d_in[i].data_ptr(), offsets, npics, W, H, cpitch, C.byref(ld), boxes, nb,
                                                  C.byref(dest), d_new[i].data_ptr() + first, out_stride, st))

        def export_copy(i):
            chk(old_call(d_in[i].data_ptr(), offsets, npics, W, H, cpitch, C.byref(desc), *extra, tmp[i].data_ptr(), item, st))
            view_of(d_old[i]).copy_(tmp_view(tmp[i]))

        legs[name + "/dest"], legs[name + "/export_copy"] = new, export_copy

    rdesc = tensor_desc(window, "rgb", f16, size=SIZE)[0]
    workload("clips_2x16", 32, 32, offs32, L.h264mi_tensor_resize_device_pitch, rdesc, None, SIZE,
             (32 // CLIP_T, 3, CLIP_T) + SIZE, lambda d: d,
             lambda t: t.view(32 // CLIP_T, CLIP_T, 3, *SIZE).permute(0, 2, 1, 3, 4))
    sdesc, arr, _, _ = rois_desc(BOXES, SIZE, NP, W, H, "rgb", f16)
    nb = len(BOXES)
    workload("tubes_8x4", nb, NP, offs, L.h264mi_tensor_rois_device_pitch, sdesc, arr, SIZE,
             (nb // TUBE_T, 3, TUBE_T) + SIZE, lambda d: d,
             lambda t: t.view(nb // TUBE_T, TUBE_T, 3, *SIZE).permute(0, 2, 1, 3, 4))
    tdesc = tensor_desc(window, "rgb", f16, size=TILE)[0]
    r0, c0 = TILE_AT[0] * TILE[0], TILE_AT[1] * TILE[1]
    workload("tile_640x360", 1, 1, zero, L.h264mi_tensor_resize_device_pitch, tdesc, None, TILE,
             (3, 2 * TILE[0], 4 * TILE[1]), lambda d: d[None, :, r0:r0 + TILE[0], c0:c0 + TILE[1]], lambda t: t)

    for f in legs.values():                             # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    same = {name + "_dest_equals_export_copy": all(torch.equal(a, b) for a, b in zip(d_new, d_old)) and bool(d_old[0].any())
            for name, (d_new, d_old) in outs.items()}
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
                     "clips_2x16": {"pictures": NP, "items": 32, "size_oh_ow": list(SIZE), "clip": CLIP_T},
                     "tubes_8x4": {"pictures": NP, "boxes": nb, "size_oh_ow": list(SIZE), "clip": TUBE_T},
                     "tile_640x360": {"tile_oh_ow": list(TILE), "canvas": [3, 2 * TILE[0], 4 * TILE[1]], "tile_at": list(TILE_AT)},
                     "samples": SAMPLES, "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "outputs_identical": same, "legs": {}, "bar": {}}
    for k in legs:
        s = stats(us[k])
        s["host_enqueue_us"] = round(statistics.median(host[k]), 2)
        res["legs"][k] = s
    for name in outs:
        a, b = (res["legs"][f"{name}/{leg}"] for leg in ("dest", "export_copy"))
        res["bar"][name] = {"dest_median_us": a["median_us"], "dest_iqr_us": a["iqr_us"],
                            "dest_range_us": [a["min_us"], a["max_us"]],
                            "export_copy_median_us": b["median_us"], "export_copy_iqr_us": b["iqr_us"],
                            "export_copy_range_us": [b["min_us"], b["max_us"]],
                            "dest_over_export_copy": round(a["median_us"] / b["median_us"], 3),
                            "meets_bar": bool(a["median_us"] <= b["median_us"])}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dest_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
