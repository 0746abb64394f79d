"""Diagnostics (not a test): what the region-of-interest export costs
(resize.hip k_tensor_resize's ROIS rows) against the same boxes
exported one call each by the single-window resized export, which is what a
caller had before.  One process, device events, warm-up, legs alternating;
writes profiles/rois_cost.json (or the path given).  Conventions of
tools/resize_cost.py.

8 pictures 1920x1088 in the frame-slot layout; 32 boxes, four per picture, of
mixed sizes from 64x128 to 640x480 (BOXES below, fixed), every one to 224x224
RGB fp16:
  rois_32          one h264mi_tensor_rois_device_pitch call (one launch)
  resize_32_calls  the same boxes as 32 h264mi_tensor_resize_device_pitch calls
and the same with 4 of the boxes (rois_4, resize_4_calls), where the per-row
window read weighs most against the work.  The bar: the one call takes no
longer than the calls it replaces (medians).  Consecutive repetitions rotate
through NSETS input and output buffer sets.  Before anything is timed the two
ways' outputs are compared: they must be the same bytes.

A sample is the device time between two events around REPS repetitions of a
leg, so it holds what the host's enqueue rate leaves idle on the device too --
what a caller sees.  host_enqueue_us is the host's own time to queue one
repetition (no synchronisation inside).

Usage: python tools/rois_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import rois_desc, tensor_desc  # noqa: E402

W, H, CW, CH, NP = 1920, 1088, 1920, 1080, 8
SAMPLES, REPS, NSETS = 15, 40, 6
SIZE = (224, 224)                                       # (oh, ow)
BOX_SIZES = [(64, 128), (96, 192), (128, 256), (160, 160), (224, 224), (320, 240), (480, 360), (640, 480)]    # (cw, ch)


def boxes():
    """(k, x, y, cw, ch): box j of picture k, sizes and positions spread over the picture, all even."""
    out = []
    for k in range(NP):
        for j in range(4):
            cw, ch = BOX_SIZES[(k + 2 * j + (j >> 1)) % len(BOX_SIZES)]
            x = 2 * ((37 * k + 211 * j + 5) % ((CW - cw) // 2 + 1))
            y = 2 * ((53 * k + 97 * j + 3) % ((CH - ch) // 2 + 1))
            out.append((k, x, y, cw, ch))
    return out


BOXES = boxes()
FEW = [BOXES[0], BOXES[9], BOXES[18], BOXES[27]]        # four boxes on four pictures, four sizes


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2), "spread_us": round(max(us) - min(us), 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "rois_cost.py measures on the GPU"
    L = _lib.mi()
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream
    stride = 3 * SIZE[0] * SIZE[1] * 2

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, outs = {}, {}
    for name, blist in (("32", BOXES), ("4", FEW)):
        n = len(blist)
        desc, arr, _, _ = rois_desc(blist, SIZE, NP, W, H, "rgb", torch.float16)
        singles = [(tensor_desc(b[1:], "rgb", torch.float16, size=SIZE)[0], (C.c_size_t * 1)(b[0] * slot)) for b in blist]
        o_rois = [torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
        o_calls = [torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
        outs[name] = (o_rois, o_calls)

        def rois(i, desc=desc, arr=arr, n=n, o=o_rois):
            chk(L.h264mi_tensor_rois_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc), arr, n,
                                                  o[i].data_ptr(), stride, st))

        def calls(i, singles=singles, o=o_calls):
            base = o[i].data_ptr()
            for r, (d, off) in enumerate(singles):
                chk(L.h264mi_tensor_resize_device_pitch(d_in[i].data_ptr(), off, 1, W, H, cpitch, C.byref(d),
                                                        base + r * stride, stride, st))

        legs[f"rois_{name}"] = (rois, n)
        legs[f"resize_{name}_calls"] = (calls, n)
    for f, _ in legs.values():                          # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    same = {name: all(torch.equal(a, b) for a, b in zip(*outs[name])) and bool(outs[name][0][0].abs().sum() > 0)
            for name in outs}
    assert all(same.values()), f"the two ways give different bytes: {same}"
    us = {k: [] for k in legs}
    host = {k: [] for k in legs}
    for _ in range(SAMPLES):
        for k, (f, _) in legs.items():                  # alternating, same process
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
    res = {"shape": {"pictures": NP, "coded": [W, H], "mode": "rgb", "dtype": "float16", "size_oh_ow": list(SIZE),
                     "boxes_k_x_y_cw_ch": [list(b) for b in BOXES], "few_boxes": [list(b) for b in FEW],
                     "samples": SAMPLES, "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "outputs_identical": same, "legs": {}}
    for k, (_, n) in legs.items():
        s = stats(us[k])
        s["boxes"] = n
        s["host_enqueue_us"] = round(statistics.median(host[k]), 2)
        s["bytes_read"] = sum(b[3] * b[4] * 3 // 2 for b in (BOXES if n == len(BOXES) else FEW))
        s["bytes_written"] = n * stride
        res["legs"][k] = s
    for name in outs:
        a, b = res["legs"][f"rois_{name}"], res["legs"][f"resize_{name}_calls"]
        res[f"bar_{name}"] = {"one_call_median_us": a["median_us"], "calls_median_us": b["median_us"],
                              "one_call_over_calls": round(a["median_us"] / b["median_us"], 3),
                              "meets_bar": bool(a["median_us"] <= b["median_us"])}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rois_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
