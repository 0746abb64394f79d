"""Diagnostics (not a test): what the accumulated residual costs (accres.hip,
k_accres), against a plain device-to-device copy of as many bytes.  One
process, device events, warm-up, legs alternating; writes
profiles/accres_cost.json (or the path given).  Conventions of
tools/mbinfo_cost.py and tools/accmv_cost.py.

Kernel time per byte moved (read + written) over eight 120x68-MB pictures
(1080p) per sample unit, through the origin maps of running the chain over the
generated stream bench_1080p_s100 (config 3, seed 100, 60 frames; the engine's
serial rule, on the host, through h264mi_accmv_step_device), on frames of
random samples (the gather's addresses come from the maps, not the samples),
each picture with a key frame of its own.
  y_int16    h264mi_accres_device, planes Y as int16
  rgb_fp16   planes RGB (colour id 2) as fp16, scale 1 / 255
A leg reads its maps, the planes of the current frames it uses and as many key
samples (one per current sample: the gather reads partly used lines, so the
traffic can be more than this count), and writes its tensors.  Each leg's
comparator is a device-to-device copy (torch's copy_ of a contiguous buffer:
one hipMemcpyAsync) of half the bytes the leg moves, so that both read plus
write the same total.  The bar is the comparator's cost per byte moved plus the
spread (max - min) of its samples.  Consecutive units rotate through NSETS sets
of buffers, each leg's more than the 256 MB Infinity Cache holds, so every
launch reads and writes HBM.

Usage: python tools/accres_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import MBREC_BYTES, Capture, accres_desc  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
WM, HM, NP = 120, 68, 8
SAMPLES, REPS, NSETS = 15, 24, 24
W, H = 16 * WM, 16 * HM
MAP = WM * HM * 1024       # bytes of an origin map
CPITCH = (8 * WM + 127) & ~127
FRAME = W * H + 2 * CPITCH * (H // 2)      # bytes of a frame in the slot layout


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "accres_cost.py measures on the GPU"
    L = _lib.mi()
    cap = Capture(gen.generate(3, 100, nframes=60))
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs) == (WM, HM) and cap.npics >= NP
    ns = cap.nslots
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    # the chain, on the device; the P pictures' maps are kept
    pool = torch.zeros((ns, MAP), dtype=torch.uint8, device="cuda")
    ser, key, pmaps = [0] * ns, 0, []
    for i, p in enumerate(cap.pictures):
        rec = np.frombuffer(cap.records_bytes(i), dtype=np.uint8).reshape(-1, MBREC_BYTES)
        k = not (rec[:, 0] <= 1).any()
        key += k
        use = [s for s in range(ns) if s != p.cur_slot and key and ser[s] == key and not k]
        ptrs = (C.c_void_p * ns)(*[pool[s].data_ptr() if s in use else None for s in range(ns)])
        d_rec = torch.from_numpy(rec.copy()).to("cuda")
        chk(L.h264mi_accmv_step_device(d_rec.data_ptr(), WM, HM, ptrs, ns, int(k), pool[p.cur_slot].data_ptr(), st))
        torch.cuda.synchronize()
        ser[p.cur_slot] = key
        if not k:
            pmaps.append(pool[p.cur_slot].clone())
    assert len(pmaps) >= NP
    anchored = float(torch.stack([(m.view(torch.int32) < 0).float().mean() for m in pmaps]).mean())

    gen_ = torch.Generator(device="cuda").manual_seed(5)
    sets = range(NSETS)
    maps = [torch.stack([pmaps[(i + k) % len(pmaps)] for k in range(NP)]) for i in sets]
    curs = [torch.randint(0, 256, (NP, FRAME), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    keys = [torch.randint(0, 256, (NP, FRAME), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    del pmaps
    moff = (C.c_size_t * NP)(*[k * MAP for k in range(NP)])
    foff = (C.c_size_t * NP)(*[k * FRAME for k in range(NP)])
    legs, keep = {}, []
    for name, planes, dtype, scale, colour, read_per_pic in (
            ("y_int16", "y", torch.int16, None, None, MAP + 2 * W * H),
            ("rgb_fp16", "rgb", torch.float16, 1.0 / 255.0, "bt709", MAP + 2 * (W * H * 3 // 2))):
        desc, npl, _ = accres_desc(planes, (0, 0, W, H), dtype, scale, None, colour)
        touts = [torch.empty((NP, npl, H, W), dtype=dtype, device="cuda") for _ in sets]
        stride = npl * H * W * touts[0].element_size()
        keep.append((desc, touts))

        def f(i, desc=desc, touts=touts, stride=stride):
            chk(L.h264mi_accres_device(curs[i].data_ptr(), foff, keys[i].data_ptr(), foff, maps[i].data_ptr(), moff, NP,
                                       WM, HM, C.byref(desc), touts[i].data_ptr(), stride, st))
        legs[name] = (f, NP * read_per_pic, NP * stride)
    for name in list(legs):
        _, rb, wb = legs[name]
        half = (rb + wb) // 2
        src = [torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
        dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in sets]
        keep.append((src, dst))

        def g(i, src=src, dst=dst):
            dst[i].copy_(src[i])
        legs[name + "_d2d_copy"] = (g, half, half)
    assert all(NSETS * (r + w) > 256 << 20 for _, r, w in legs.values())
    us = {k: [] for k in legs}
    for k, (f, _, _) in legs.items():                   # warm-up: code objects, every buffer
        for i in sets:
            f(i)
    torch.cuda.synchronize()
    for _ in range(SAMPLES):
        for k, (f, _, _) in legs.items():               # alternating, same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(REPS):
                f(r % NSETS)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    out = {}
    for k, (_, rb, wb) in legs.items():
        s = stats(us[k])
        s["bytes_read"], s["bytes_written"] = rb, wb
        s["ps_per_byte_moved"] = round(s["median_us"] * 1e6 / (rb + wb), 3)
        bps = (rb + wb) / (s["median_us"] * 1e-6)
        s["bytes_per_s_read_plus_written"] = round(bps)
        s["share_of_hbm_peak"] = round(bps / HBM_PEAK, 3)
        out[k] = s
    for a in [k for k in legs if not k.endswith("_d2d_copy")]:
        b = out[a + "_d2d_copy"]
        moved = b["bytes_read"] + b["bytes_written"]
        spread = (b["max_us"] - b["min_us"]) * 1e6 / moved
        over = out[a]["ps_per_byte_moved"] - b["ps_per_byte_moved"]
        out[a + "_vs_d2d_copy"] = {"extra_ps_per_byte_moved": round(over, 3),
                                   "comparator_spread_ps_per_byte_moved": round(spread, 3),
                                   "bar_ps_per_byte_moved": round(b["ps_per_byte_moved"] + spread, 3),
                                   "within_bar": bool(over <= spread),
                                   "kernel_over_comparator": round(out[a]["median_us"] / b["median_us"], 3)}
    res = {"shape": {"pictures_per_unit": NP, "mbs": [WM, HM], "samples": SAMPLES, "units_per_sample": REPS,
                     "buffer_sets_rotated": NSETS, "stream": "gen.generate(3, 100, nframes=60)", "slots": ns,
                     "anchored_share_of_the_p_pictures_maps": round(anchored, 3)},
           "hbm_peak_bytes_per_s": HBM_PEAK, "legs": out}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accres_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
