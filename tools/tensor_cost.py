"""Diagnostics (not a test): what exporting pictures as device tensors costs
(tensor.hip), against the kernel it is modelled on and against the host path it
replaces.  One process, device events, warm-up, legs alternating; writes
profiles/tensor_cost.json (or the path given).  Conventions of
tools/crop_cost.py.

(a) kernel time per byte moved (read + written), 8 pictures 1920x1088 ->
    window 1920x1080 from the frame-slot layout, RGB planes as uint8, fp16,
    bf16 and fp32 (and uint8 and fp16 with colour set 2, BT.709 limited,
    against the default leg of the same dtype), against k_crop_rgba
    (h264mi_crop_device_pitch, rgba) on the same slots in the same run.  The bar is the comparator: a tensor
    kernel may cost more per byte moved by no more than the spread (max -
    min) of the comparator's samples; the interquartile range is recorded
    beside it.  Consecutive launches rotate through NSETS input and output
    buffers, more than the 256 MB Infinity Cache holds, so every launch
    reads and writes HBM.
(b) Engine.to_tensor of 8 slots (one launch, nothing leaves the device;
    timed to torch.cuda.synchronize) against 8 x Engine.read_crop(rgba=True)
    (kernel + D2H + sync each), wall time per picture.

Usage: python tools/tensor_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import Engine, tensor_desc  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
W, H, CW, CH, NP = 1920, 1088, 1920, 1080, 8
SAMPLES, REPS, NSETS = 15, 24, 6


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def kernel_leg(torch, L):
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    sets = range(NSETS)
    rbytes = NP * CW * CH * 3 // 2
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    rgba = [torch.empty(NP * CW * CH * 4, dtype=torch.uint8, device="cuda") for _ in sets]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs = {"crop_rgba": (lambda i: chk(L.h264mi_crop_device_pitch(d_in[i].data_ptr(), rgba[i].data_ptr(), W, H, cpitch, 0, 0,
                                                                 CW, CH, 1, NP, slot, CW * CH * 4, st)),
                          NP * CW * CH * 4)}
    keep = []
    for dtype in (torch.uint8, torch.float16, torch.bfloat16, torch.float32):
        desc, planes, _ = tensor_desc((0, 0, CW, CH), "rgb", dtype)
        outs = [torch.empty((NP, planes, CH, CW), dtype=dtype, device="cuda") for _ in sets]
        stride = planes * CH * CW * outs[0].element_size()
        keep.append((desc, outs))

        def f(i, desc=desc, outs=outs, stride=stride):
            chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc),
                                             outs[i].data_ptr(), stride, st))
        legs["tensor_rgb_" + str(dtype).split(".")[1]] = (f, NP * stride)
    # the same export with colour set 2 (BT.709 limited): the COL instantiations
    for dtype in (torch.uint8, torch.float16):
        desc, planes, _ = tensor_desc((0, 0, CW, CH), "rgb", dtype, colour="bt709")
        outs = [torch.empty((NP, planes, CH, CW), dtype=dtype, device="cuda") for _ in sets]
        stride = planes * CH * CW * outs[0].element_size()
        keep.append((desc, outs))

        def f(i, desc=desc, outs=outs, stride=stride):
            chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc),
                                             outs[i].data_ptr(), stride, st))
        legs["tensor_rgb_" + str(dtype).split(".")[1] + "_bt709"] = (f, NP * stride)
    us = {k: [] for k in legs}
    for k, (f, _) in legs.items():                      # warm-up: code objects, every shape
        for i in sets:
            f(i)
    torch.cuda.synchronize()
    for _ in range(SAMPLES):
        for k, (f, _) in legs.items():                  # alternating, same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(REPS):
                f(r % NSETS)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    out = {}
    for k, (_, wbytes) in legs.items():
        s = stats(us[k])
        s["bytes_read"], s["bytes_written"] = rbytes, wbytes
        s["ps_per_byte_moved"] = round(s["median_us"] * 1e6 / (rbytes + wbytes), 3)
        bps = (wbytes + rbytes) / (s["median_us"] * 1e-6)
        s["bytes_per_s_read_plus_written"] = round(bps)
        s["kernel_share_of_hbm_peak"] = round(bps / HBM_PEAK, 3)
        out[k] = s
    b = out["crop_rgba"]
    moved_b = b["bytes_read"] + b["bytes_written"]
    spread = (b["max_us"] - b["min_us"]) * 1e6 / moved_b
    iqr = b["iqr_us"] * 1e6 / moved_b
    # a colour leg against the default leg of its dtype: same bytes moved, the bar is the default's own spread
    for a in [k for k in legs if k.endswith("_bt709")]:
        d = out[a[:-len("_bt709")]]
        dspread = (d["max_us"] - d["min_us"]) * 1e6 / (d["bytes_read"] + d["bytes_written"])
        over = out[a]["ps_per_byte_moved"] - d["ps_per_byte_moved"]
        out[a + "_vs_default"] = {"extra_ps_per_byte_moved": round(over, 3),
                                  "default_spread_ps_per_byte_moved": round(dspread, 3),
                                  "within_default_spread": bool(over <= dspread)}
    for a in [k for k in legs if k != "crop_rgba"]:
        over = out[a]["ps_per_byte_moved"] - b["ps_per_byte_moved"]
        out[a + "_vs_crop_rgba"] = {"extra_ps_per_byte_moved": round(over, 3),
                                    "comparator_spread_ps_per_byte_moved": round(spread, 3),
                                    "within_comparator_spread": bool(over <= spread),
                                    "comparator_iqr_ps_per_byte_moved": round(iqr, 3),
                                    "within_comparator_iqr": bool(over <= iqr)}
    return out


def engine_leg(torch):
    eng = Engine(W // 16, H // 16, NP, 2)
    streams, slots = list(range(NP)), [0] * NP
    out = torch.empty((NP, 3, CH, CW), dtype=torch.float16, device="cuda")

    def tensor():
        eng.to_tensor(streams, slots, window=(0, 0, CW, CH), out=out)
        torch.cuda.synchronize()

    def tensor_call_only():
        eng.to_tensor(streams, slots, window=(0, 0, CW, CH), out=out)

    def read():
        for s in streams:
            eng.read_crop(s, 0, 0, 0, CW, CH, rgba=True)

    legs = {"to_tensor_8_slots_fp16": tensor, "read_crop_rgba_x8": read, "to_tensor_8_slots_fp16_call_only": tensor_call_only}
    us = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(SAMPLES):
        for k, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(3):
                f()
            us[k].append((time.perf_counter() - t0) * 1e6 / 3 / NP)
            torch.cuda.synchronize()
    res = {k: {kk.replace("_us", "_us_per_picture"): v for kk, v in stats(v).items()} for k, v in us.items()}
    res["read_crop_over_to_tensor"] = round(res["read_crop_rgba_x8"]["median_us_per_picture"] /
                                            res["to_tensor_8_slots_fp16"]["median_us_per_picture"], 1)
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "tensor_cost.py measures on the GPU"
    L = _lib.mi()
    res = {"shape": {"pictures": NP, "coded": [W, H], "window": [0, 0, CW, CH], "mode": "rgb", "samples": SAMPLES,
                     "launches_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "a_kernel": kernel_leg(torch, L), "b_engine": engine_leg(torch)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tensor_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
