"""Diagnostics (not a test): what the bicubic filter of the resized tensor export
costs (resize.hip with H264MI_RESIZE_BICUBIC)
  1. against what a caller had before it: the planar fp16 full-size export
     (h264mi_tensor_device_pitch) followed by torch's
     F.interpolate(mode="bicubic", antialias=True) on the device into a
     preallocated tensor (aten's out= variant; for boxes, one call per box on a
     slice of the full-size tensor);
  2. against the triangle filter on the same legs in the same process.
One process, device events, warm-up, legs alternating; writes
profiles/bicubic_cost.json (or the path given).  Conventions of
tools/resize_cost.py: 8 pictures 1920x1088 in the frame-slot layout, window
1920x1080, RGB fp16, 15 samples of 24 launches, consecutive launches rotating
through NSETS buffer sets.  Legs: the eight windows to 224x224 and to 384x640
(oh x ow), and tools/rois_cost.py's 32 boxes to 224x224.  No pass mark: medians
with min, max and IQR, and the ratios.  Before anything is timed the fused
result is compared with the torch path's on the same pictures (scale 1/255, so
data in [0, 1]): the largest difference is recorded, against torch's result as
it is and clamped to [0, 1] (the export clamps, torch does not).

Usage: python tools/bicubic_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import rois_desc, tensor_desc  # noqa: E402
from rois_cost import BOXES  # noqa: E402

W, H, CW, CH, NP = 1920, 1088, 1920, 1080, 8
SAMPLES, REPS, NSETS = 15, 24, 6
SIZES = [(224, 224), (384, 640)]                        # (oh, ow)
BOX_SIZE = (224, 224)


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "bicubic_cost.py measures on the GPU"
    L = _lib.mi()
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    aa_out = getattr(getattr(torch.ops.aten, "_upsample_bicubic2d_aa", None), "out", None)

    def interpolate(src, size, out):
        """torch's antialiased bicubic of src (n, 3, h, w) into the preallocated out (n, 3) + size"""
        if aa_out is not None:
            aa_out(src, list(size), False, out=out)
        else:
            out.copy_(F.interpolate(src, size=size, mode="bicubic", antialias=True, align_corners=False))

    fdesc, planes, _ = tensor_desc((0, 0, CW, CH), "rgb", torch.float16)
    full = [torch.empty((NP, planes, CH, CW), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    fstride = planes * CH * CW * 2

    def export_full(i):
        chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(fdesc), full[i].data_ptr(),
                                         fstride, st))

    legs, outs = {"tensor_rgb_float16_full": export_full}, {}
    for oh, ow in SIZES:
        tag = f"{oh}x{ow}"
        stride = planes * oh * ow * 2
        for filt in ("bicubic", "triangle"):
            desc = tensor_desc((0, 0, CW, CH), "rgb", torch.float16, size=(oh, ow), filter=filt)[0]
            o = [torch.zeros((NP, planes, oh, ow), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
            outs[f"{filt}_{tag}"] = o

            def fused(i, desc=desc, o=o, stride=stride):
                chk(L.h264mi_tensor_resize_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc),
                                                        o[i].data_ptr(), stride, st))
            legs[f"{filt}_{tag}"] = fused
        o = [torch.zeros((NP, planes, oh, ow), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
        outs[f"full_plus_torch_{tag}"] = o

        def torch_path(i, o=o, size=(oh, ow)):
            export_full(i)
            interpolate(full[i], size, o[i])
        legs[f"full_plus_torch_{tag}"] = torch_path
    n = len(BOXES)
    bstride = planes * BOX_SIZE[0] * BOX_SIZE[1] * 2
    for filt in ("bicubic", "triangle"):
        desc, arr, _, _ = rois_desc(BOXES, BOX_SIZE, NP, W, H, "rgb", torch.float16, filter=filt)
        o = [torch.zeros((n, planes) + BOX_SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
        outs[f"{filt}_boxes"] = o

        def fused_boxes(i, desc=desc, arr=arr, o=o):
            chk(L.h264mi_tensor_rois_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc), arr, n,
                                                  o[i].data_ptr(), bstride, st))
        legs[f"{filt}_boxes"] = fused_boxes
    o = [torch.zeros((n, planes) + BOX_SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    outs["full_plus_torch_boxes"] = o

    def torch_boxes(i, o=o):
        export_full(i)
        for r, (k, x, y, cw, ch) in enumerate(BOXES):
            interpolate(full[i][k:k + 1, :, y:y + ch, x:x + cw], BOX_SIZE, o[i][r:r + 1])
    legs["full_plus_torch_boxes"] = torch_boxes

    for f in legs.values():                             # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    diff = {}
    for tag in [f"{oh}x{ow}" for oh, ow in SIZES] + ["boxes"]:
        a, b = outs[f"bicubic_{tag}"][0].float(), outs[f"full_plus_torch_{tag}"][0].float()
        assert bool(a.abs().sum() > 0) and bool(b.abs().sum() > 0)
        diff[tag] = {"max_abs_diff_vs_torch": round(float((a - b).abs().max()), 6),
                     "max_abs_diff_vs_torch_clamped_0_1": round(float((a - b.clamp(0.0, 1.0)).abs().max()), 6),
                     "in_units_of_1_over_255": round(float((a - b.clamp(0.0, 1.0)).abs().max()) * 255.0, 4)}
    us = {k: [] for k in legs}
    for _ in range(SAMPLES):
        for k, f in legs.items():                       # alternating, same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(REPS):
                f(r % NSETS)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    res = {"shape": {"pictures": NP, "coded": [W, H], "window": [0, 0, CW, CH], "mode": "rgb", "dtype": "float16",
                     "sizes_oh_ow": SIZES, "boxes": n, "box_size_oh_ow": list(BOX_SIZE), "samples": SAMPLES,
                     "launches_per_sample": REPS, "buffer_sets_rotated": NSETS,
                     "torch_path": "aten._upsample_bicubic2d_aa.out" if aa_out is not None else "F.interpolate + copy_",
                     "torch": torch.__version__},
           "largest_difference_on_0_1_data": diff, "legs": {k: stats(v) for k, v in us.items()}, "ratios": {}}
    for tag in [f"{oh}x{ow}" for oh, ow in SIZES] + ["boxes"]:
        bic, tri, alt = (res["legs"][f"{k}_{tag}"]["median_us"] for k in ("bicubic", "triangle", "full_plus_torch"))
        res["ratios"][tag] = {"bicubic_over_full_plus_torch": round(bic / alt, 4),
                              "full_plus_torch_over_bicubic": round(alt / bic, 2),
                              "bicubic_over_triangle": round(bic / tri, 3)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bicubic_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
