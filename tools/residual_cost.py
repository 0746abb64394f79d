"""Diagnostics (not a test): what exporting the decoded residual as device
tensors costs (residual.hip, k_residual), against a plain device-to-device copy
of as many bytes.  One process, device events, warm-up, legs alternating;
writes profiles/residual_cost.json (or the path given).  Conventions of
tools/mbinfo_cost.py.

Kernel time per byte moved (read + written) of h264mi_residual_device over
eight 120x68-MB pictures (1080p) per launch, the whole MB-aligned picture,
with the records and coefficient blocks the parser produced for the generated
stream bench_1080p_s100 (config 3, seed 100, 60 frames): real coefficient
density, most MBs of its P pictures skipped or uncoded.
  y_int16     planes "y" as int16
  yuv_fp16    planes "yuv" as fp16 with scale 1 / 255
A leg reads its pictures' record batches and coefficient pools (counted whole:
the kernel asks for 16 of a record's 96 bytes and skips I_PCM blocks, but the
lines come from HBM all the same) and writes its tensors.  Each leg's
comparator is a device-to-device copy (torch's copy_ of a contiguous buffer:
one hipMemcpyAsync) of half the bytes the leg moves, so that both read plus
write the same total.  The bar is the comparator's cost per byte moved plus the
spread (max - min) of its samples.  Consecutive launches rotate through NSETS
sets of buffers (set i holds the eight pictures from picture 2 i on), each
leg's more than the 256 MB Infinity Cache holds, so every launch reads and
writes HBM.

Usage: python tools/residual_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import MBREC_BYTES, Capture, residual_desc  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
WM, HM, NP = 120, 68, 8
SAMPLES, REPS, NSETS = 15, 24, 24


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "residual_cost.py measures on the GPU"
    L = _lib.mi()
    cap = Capture(gen.generate(3, 100, nframes=60))
    assert cap.errors == 0 and (cap.w_mbs, cap.h_mbs) == (WM, HM) and cap.npics >= NP
    batch = WM * HM * MBREC_BYTES
    d_rec, d_coef, bases, nblk, rbytes = [], [], [], [], []
    coded = zero = 0
    for i in range(NSETS):
        pics = [(2 * i + k) % cap.npics for k in range(NP)]
        recs = b"".join(cap.records_bytes(p) for p in pics)
        pool, base = b"", []
        for p in pics:
            base.append(len(pool) // 32)
            pool += cap.coef_bytes(p)
        r = np.frombuffer(recs, dtype=np.uint8).reshape(-1, MBREC_BYTES)
        cbits = r[:, 8:12].copy().view("<u4").reshape(-1)
        live = np.isin(r[:, 0], (0, 2, 3)) & ((cbits & 0x7FFFFFF) != 0)
        coded += int(live.sum())
        zero += int((~live).sum())
        d_rec.append(torch.from_numpy(r.copy()).to("cuda"))
        d_coef.append(torch.from_numpy(np.frombuffer(pool + bytes(64), dtype=np.uint8).copy()).to("cuda"))
        bases.append((C.c_uint32 * NP)(*base))
        nblk.append(len(pool) // 32)
        rbytes.append(len(recs) + len(pool))
    offs = (C.c_size_t * NP)(*[k * batch for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    sets = range(NSETS)
    rmean = sum(rbytes) // NSETS

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, keep = {}, []
    for name, planes, dtype, scale in (("y_int16", "y", torch.int16, None), ("yuv_fp16", "yuv", torch.float16, 1 / 255)):
        desc, npl, _ = residual_desc(planes, (0, 0, 16 * WM, 16 * HM), dtype, scale)
        outs = [torch.empty((NP, npl, 16 * HM, 16 * WM), dtype=dtype, device="cuda") for _ in sets]
        stride = npl * 16 * HM * 16 * WM * outs[0].element_size()
        wbytes = NP * stride
        half = (rmean + wbytes) // 2
        src = [torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
        dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in sets]
        keep.append((desc, outs, src, dst))

        def f(i, desc=desc, outs=outs, stride=stride):
            chk(L.h264mi_residual_device(d_rec[i].data_ptr(), offs, d_coef[i].data_ptr(), bases[i], nblk[i], NP, WM, HM,
                                         C.byref(desc), outs[i].data_ptr(), stride, st))

        def g(i, src=src, dst=dst):
            dst[i].copy_(src[i])
        legs[name] = (f, rmean, wbytes)
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
    res = {"shape": {"pictures_per_launch": NP, "mbs": [WM, HM], "samples": SAMPLES, "launches_per_sample": REPS,
                     "buffer_sets_rotated": NSETS, "stream": "gen.generate(3, 100, nframes=60)",
                     "mbs_with_coefficients_share": round(coded / (coded + zero), 3),
                     "coefficient_blocks_per_picture_mean": round(sum(nblk) / (NSETS * NP))},
           "hbm_peak_bytes_per_s": HBM_PEAK, "legs": out}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "residual_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
