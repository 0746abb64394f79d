"""Diagnostics (not a test): what the accumulated motion costs (accmv.hip,
k_accmv_step and k_accmv), against a plain device-to-device copy of as many
bytes.  One process, device events, warm-up, legs alternating; writes
profiles/accmv_cost.json (or the path given).  Conventions of
tools/mbinfo_cost.py.

Kernel time per byte moved (read + written) over eight 120x68-MB pictures
(1080p) per sample unit, with the records the parser produced for the generated
stream bench_1080p_s100 (config 3, seed 100, 60 frames) and the origin maps of
running the chain over it (the engine's serial rule, on the host, through
h264mi_accmv_step_device).
  step          h264mi_accmv_step_device for eight P pictures: the stateless call
                takes one picture, so a unit is eight launches (the engine puts
                the pictures of a batch into one)
  adx_ady_fp16  h264mi_accmv_device, channels (adx, ady) as fp16, scale 0.25
  all5_int16    all five channels as int16
The step reads its pictures' records and, counted as one word per sample, the
reference maps (a sample of an intra MB reads nothing, so this over-counts by
the intra share), and writes a map per picture.  An export reads its maps and
writes its tensors.  Each leg's comparator is a device-to-device copy (torch's
copy_ of a contiguous buffer: one hipMemcpyAsync) of half the bytes the leg
moves, so that both read plus write the same total.  The bar is the
comparator's cost per byte moved plus the spread (max - min) of its samples.
Consecutive units rotate through NSETS sets of buffers, each leg's more than the
256 MB Infinity Cache holds, so every launch reads and writes HBM.

Beside it: the k_wgpp launch a batch's step queues behind (eight streams, the
engine's own event timing), and the step's share of it.

Usage: python tools/accmv_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import MBREC_BYTES, Capture, Engine, accmv_desc  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
WM, HM, NP = 120, 68, 8
SAMPLES, REPS, NSETS = 15, 24, 24
MAP = WM * HM * 1024       # bytes of an origin map


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "accmv_cost.py measures on the GPU"
    L = _lib.mi()
    cap = Capture(gen.generate(3, 100, nframes=60))
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs) == (WM, HM) and cap.npics >= NP
    ns = cap.nslots
    st = torch.cuda.current_stream().cuda_stream
    batch = WM * HM * MBREC_BYTES

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    # the chain, on the device: per picture whether it is a key picture and which slots it may read
    recs = [np.frombuffer(cap.records_bytes(i), dtype=np.uint8).reshape(-1, MBREC_BYTES) for i in range(cap.npics)]
    d_recs = [torch.from_numpy(r.copy()).to("cuda") for r in recs]
    pool = torch.zeros((ns, MAP), dtype=torch.uint8, device="cuda")
    ser, key, usable, is_key = [0] * ns, 0, [], []
    for i, p in enumerate(cap.pictures):
        k = not (recs[i][:, 0] <= 1).any()
        key += k
        use = [s for s in range(ns) if s != p.cur_slot and key and ser[s] == key and not k]
        ptrs = (C.c_void_p * ns)(*[pool[s].data_ptr() if s in use else None for s in range(ns)])
        chk(L.h264mi_accmv_step_device(d_recs[i].data_ptr(), WM, HM, ptrs, ns, int(k), pool[p.cur_slot].data_ptr(), st))
        ser[p.cur_slot] = key
        usable.append(use)
        is_key.append(k)
    torch.cuda.synchronize()
    anchored = float((pool.view(torch.int32) < 0).float().mean())
    ppics = [i for i in range(cap.npics) if not is_key[i]]
    assert len(ppics) >= NP

    gen_ = torch.Generator(device="cuda").manual_seed(5)
    sets = range(NSETS)
    legs, keep = {}, []

    # step: set i steps the eight P pictures from the i-th on, from its own copy of the slots' maps
    pools = [pool.clone() for _ in sets]
    outs = [torch.empty((NP, MAP), dtype=torch.uint8, device="cuda") for _ in sets]
    calls = []
    for i in sets:
        one = []
        for k in range(NP):
            p = ppics[(i + k) % len(ppics)]
            ptrs = (C.c_void_p * ns)(*[pools[i][s].data_ptr() if s in usable[p] else None for s in range(ns)])
            one.append((d_recs[p].data_ptr(), ptrs, outs[i][k].data_ptr()))
        calls.append(one)
    keep.append((pools, outs, calls))

    def step(i):
        for rec, ptrs, out in calls[i]:
            chk(L.h264mi_accmv_step_device(rec, WM, HM, ptrs, ns, 0, out, st))
    legs["step"] = (step, NP * (batch + MAP), NP * MAP)

    offs = (C.c_size_t * NP)(*[k * MAP for k in range(NP)])
    for name, chans, dtype, scale in (("adx_ady_fp16", ("adx", "ady"), torch.float16, 0.25),
                                      ("all5_int16", ("adx", "ady", "jx", "jy", "anchored"), torch.int16, None)):
        desc, nch, _ = accmv_desc(chans, (0, 0, 16 * WM, 16 * HM), dtype, scale)
        touts = [torch.empty((NP, nch, 16 * HM, 16 * WM), dtype=dtype, device="cuda") for _ in sets]
        stride = nch * 16 * HM * 16 * WM * touts[0].element_size()
        keep.append((desc, touts))

        def f(i, desc=desc, touts=touts, stride=stride):
            chk(L.h264mi_accmv_device(outs[i].data_ptr(), offs, NP, WM, HM, C.byref(desc), touts[i].data_ptr(), stride, st))
        legs[name] = (f, NP * MAP, NP * stride)
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

    # the k_wgpp launch a batch's step queues behind: eight streams decoding the stream side by side
    eng = Engine(WM, HM, NP, ns)
    eng.set_timing(cap.npics)
    for p in cap.pictures:
        eng.decode(list(range(NP)), [p] * NP)
    eng.sync()
    per = [u for u, k in zip(eng.timing_list(cap.npics) or [], is_key) if not k and u > 0]      # the P pictures' launches
    eng.close()
    wgpp_us = statistics.median(per) if per else None
    step_us = out["step"]["median_us"]
    res = {"shape": {"pictures_per_unit": NP, "mbs": [WM, HM], "samples": SAMPLES, "units_per_sample": REPS,
                     "buffer_sets_rotated": NSETS, "stream": "gen.generate(3, 100, nframes=60)", "slots": ns,
                     "key_pictures": int(sum(is_key)), "anchored_share_of_the_final_maps": round(anchored, 3)},
           "hbm_peak_bytes_per_s": HBM_PEAK, "legs": out,
           "beside_k_wgpp": {"step_us_per_picture": round(step_us / NP, 2),
                             "k_wgpp_us_per_launch_of_8_pictures": None if wgpp_us is None else round(wgpp_us, 1),
                             "step_share_of_k_wgpp": None if wgpp_us is None else round(step_us / wgpp_us, 4)}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accmv_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
