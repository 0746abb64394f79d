"""Diagnostics (not a test): what the resized field exports cost
(field_resize.hip, k_field_resize), against the full-resolution export of the
same channels and window -- what a caller has to run today before any resize of
their own.  One process, device events, warm-up, legs alternating; writes
profiles/field_resize_cost.json (or the path given).  Conventions of
tools/accres_cost.py.

Eight 120x68-MB pictures (1080p) per sample unit, window (0, 0, 1920, 1080),
through the origin maps of running the chain over the generated stream
bench_1080p_s100 (config 3, seed 100, 60 frames; the engine's serial rule, on
the host, through h264mi_accmv_step_device), on frames of random samples, each
picture with a key frame of its own.
  accmv_fp16_224        h264mi_accmv_resize_device, ("adx", "ady") as fp16 -> 224 x 224
  accmv_fp16_full       h264mi_accmv_device, the same channels and window
  accres_rgb_fp16_224   h264mi_accres_resize_device, planes RGB (colour id 2) as fp16, scale 1 / 255 -> 224 x 224
  accres_rgb_fp16_full  h264mi_accres_device, the same planes and window
A resized leg reads the bytes its full-resolution leg reads and writes about 40
times fewer.  The bar: the resized leg's median is no higher than the
full-resolution leg's median plus that leg's own spread (max - min of its
samples).  Consecutive units rotate through NSETS sets of buffers, each leg's
more than the 256 MB Infinity Cache holds, so every launch reads HBM.

Usage: python tools/field_resize_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import MBREC_BYTES, Capture, accmv_desc, accres_desc  # noqa: E402

WM, HM, NP = 120, 68, 8
SAMPLES, REPS, NSETS = 15, 24, 24
W, H = 16 * WM, 16 * HM
WIN = (0, 0, 1920, 1080)
SIZE = (224, 224)
MAP = WM * HM * 1024       # bytes of an origin map
CPITCH = (8 * WM + 127) & ~127
FRAME = W * H + 2 * CPITCH * (H // 2)      # bytes of a frame in the slot layout


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "field_resize_cost.py measures on the GPU"
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

    gen_ = torch.Generator(device="cuda").manual_seed(5)
    sets = range(NSETS)
    maps = [torch.stack([pmaps[(i + k) % len(pmaps)] for k in range(NP)]) for i in sets]
    curs = [torch.randint(0, 256, (NP, FRAME), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    keys = [torch.randint(0, 256, (NP, FRAME), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    del pmaps
    moff = (C.c_size_t * NP)(*[k * MAP for k in range(NP)])
    foff = (C.c_size_t * NP)(*[k * FRAME for k in range(NP)])
    wmap = 4 * WIN[2] * WIN[3]                  # bytes of the window's map words
    legs, keep = {}, []

    def add(name, call, desc, shape, read_per_pic):
        touts = [torch.empty((NP,) + shape, dtype=torch.float16, device="cuda") for _ in sets]
        stride = touts[0][0].numel() * 2
        keep.append((desc, touts))

        def f(i):
            chk(call(i, desc, touts[i].data_ptr(), stride))
        legs[name] = (f, NP * read_per_pic, NP * stride)

    def mv(entry):
        return lambda i, desc, out, stride: entry(maps[i].data_ptr(), moff, NP, WM, HM, C.byref(desc), out, stride, st)

    def res(entry):
        return lambda i, desc, out, stride: entry(curs[i].data_ptr(), foff, keys[i].data_ptr(), foff, maps[i].data_ptr(),
                                                  moff, NP, WM, HM, C.byref(desc), out, stride, st)

    chans = ("adx", "ady")
    add("accmv_fp16_224", mv(L.h264mi_accmv_resize_device), accmv_desc(chans, WIN, torch.float16, size=SIZE)[0],
        (2,) + SIZE, wmap)
    add("accmv_fp16_full", mv(L.h264mi_accmv_device), accmv_desc(chans, WIN, torch.float16)[0], (2, WIN[3], WIN[2]), wmap)
    rgb = dict(planes="rgb", window=WIN, dtype=torch.float16, scale=1.0 / 255.0, colour="bt709")
    rread = wmap + 2 * (WIN[2] * WIN[3] * 3 // 2)
    add("accres_rgb_fp16_224", res(L.h264mi_accres_resize_device), accres_desc(size=SIZE, **rgb)[0], (3,) + SIZE, rread)
    add("accres_rgb_fp16_full", res(L.h264mi_accres_device), accres_desc(**rgb)[0], (3, WIN[3], WIN[2]), rread)
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
        s["us_per_picture"] = round(s["median_us"] / NP, 2)
        out[k] = s
    for a in ("accmv_fp16", "accres_rgb_fp16"):
        small, full = out[a + "_224"], out[a + "_full"]
        spread = full["max_us"] - full["min_us"]
        out[a + "_224_vs_full"] = {"full_median_us": full["median_us"], "full_spread_us": round(spread, 2),
                                   "bar_us": round(full["median_us"] + spread, 2), "resized_median_us": small["median_us"],
                                   "resized_spread_us": round(small["max_us"] - small["min_us"], 2),
                                   "bar": "met" if small["median_us"] <= full["median_us"] + spread else "missed",
                                   "resized_over_full": round(small["median_us"] / full["median_us"], 3),
                                   "bytes_written_full_over_resized": round(full["bytes_written"] / small["bytes_written"], 1)}
    res_ = {"shape": {"pictures_per_unit": NP, "mbs": [WM, HM], "window": list(WIN), "size": list(SIZE), "samples": SAMPLES,
                      "units_per_sample": REPS, "buffer_sets_rotated": NSETS, "stream": "gen.generate(3, 100, nframes=60)",
                      "slots": ns},
            "legs": out}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "field_resize_cost.json")
    with open(path, "w") as f:
        json.dump(res_, f, indent=1)
        f.write("\n")
    print(json.dumps(res_, indent=1))


if __name__ == "__main__":
    main()
