"""Diagnostics (not a test): what exporting motion vectors and MB side
information as device tensors costs (mbinfo.hip, k_mbinfo), against a plain
device-to-device copy of as many bytes.  One process, device events, warm-up,
legs alternating; writes profiles/mbinfo_cost.json (or the path given).
Conventions of tools/tensor_cost.py.

Kernel time per byte moved (read + written) of h264mi_mbinfo_device over eight
120x68-MB record batches (1080p) per launch, the whole 480x272 block grid:
  mv_ref_fp16   ("mvx", "mvy", "ref_idx") as fp16 with scale 0.25
  all9_int16    all nine channels as int16
Each leg's comparator is a device-to-device copy (torch's copy_ of a contiguous
buffer: one hipMemcpyAsync) of half the bytes the leg moves, so that both read
plus write the same total.  The bar is the comparator's cost per byte moved
plus the spread (max - min) of its samples.  Consecutive launches rotate through
NSETS sets of buffers, each leg's more than the 256 MB Infinity Cache holds, so
every launch reads and writes HBM.

Usage: python tools/mbinfo_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import MBREC_BYTES, mbinfo_desc  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
WM, HM, NP = 120, 68, 8
SAMPLES, REPS, NSETS = 15, 24, 24
CHANNELS = ("mvx", "mvy", "ref_idx", "ref_slot", "mb_type", "qp", "intra_mode", "coded", "slice")


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def main():
    import torch
    assert torch.cuda.is_available(), "mbinfo_cost.py measures on the GPU"
    L = _lib.mi()
    batch = WM * HM * MBREC_BYTES
    rbytes = NP * batch
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    sets = range(NSETS)
    d_in = []
    for _ in sets:
        r = torch.randint(0, 256, (NP * WM * HM, MBREC_BYTES), dtype=torch.uint8, device="cuda", generator=gen_)
        r[:, 0] = torch.randint(0, 5, (NP * WM * HM,), dtype=torch.uint8, device="cuda", generator=gen_)      # MBT_*
        d_in.append(r)
    offs = (C.c_size_t * NP)(*[k * batch for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, keep = {}, []
    for name, chans, dtype, scale in (("mv_ref_fp16", CHANNELS[:3], torch.float16, 0.25),
                                      ("all9_int16", CHANNELS, torch.int16, None)):
        desc, nch, _ = mbinfo_desc(chans, (0, 0, 4 * WM, 4 * HM), dtype, scale)
        outs = [torch.empty((NP, nch, 4 * HM, 4 * WM), dtype=dtype, device="cuda") for _ in sets]
        stride = nch * 4 * HM * 4 * WM * outs[0].element_size()
        wbytes = NP * stride
        half = (rbytes + wbytes) // 2
        src = [torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
        dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in sets]
        keep.append((desc, outs, src, dst))

        def f(i, desc=desc, outs=outs, stride=stride):
            chk(L.h264mi_mbinfo_device(d_in[i].data_ptr(), offs, NP, WM, HM, C.byref(desc), outs[i].data_ptr(), stride, st))

        def g(i, src=src, dst=dst):
            dst[i].copy_(src[i])
        legs[name] = (f, rbytes, wbytes)
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
    res = {"shape": {"batches_per_launch": NP, "mbs": [WM, HM], "blocks": [4 * WM, 4 * HM], "samples": SAMPLES,
                     "launches_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "hbm_peak_bytes_per_s": HBM_PEAK, "legs": out}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mbinfo_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
