"""Diagnostics (not a test): what cropped output costs on the GPU (crop.hip),
against what it replaces.  One process, device events, warm-up, A and B
alternating; writes profiles/crop_cost.json (or the path given).

(a) kernel time per output byte, 8 pictures 1920x1088 -> 1920x1080 from the
    frame-slot layout: cropped RGBA vs k_yuv2rgba on the same pictures at
    1920x1088; cropped I420 vs a device-to-device hipMemcpyAsync of the same
    byte count.  The bar is the comparator: the cropped kernel may cost more
    per output byte by no more than the spread (max - min) of the comparator's
    samples; the interquartile range is recorded beside it, since one slow
    sample sets max - min.  Consecutive launches rotate through NSETS input
    and output buffers, more than the 256 MB Infinity Cache holds, so every
    launch reads and writes HBM and bytes/s over the HBM peak is the kernel's
    share of peak.
(b) h264mi_engine_read_crop of one 1080p slot into pinned memory: kernel +
    one contiguous D2H vs three hipMemcpy2DAsync straight from the slot
    (issued here, on the HIP runtime the process holds).
(c) host CPU per picture: h264mi_dec -C on bench_1080p_s100 vs h264mi_dec
    plus a byte-loop crop on the calling thread (tools/ubench/crop_loop.c).

Usage: python tools/crop_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import Engine  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec peak
W, H, CW, CH, NP = 1920, 1088, 1920, 1080, 8
SAMPLES, REPS, NSETS = 15, 24, 6


def hip_runtime():
    """The HIP runtime this process already holds (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2)}


def kernel_leg(torch, L):
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    n420 = CW * CH * 3 // 2
    sets = range(NSETS)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in sets]
    rgba_full = [torch.empty(NP * W * H * 4, dtype=torch.uint8, device="cuda") for _ in sets]
    rgba_crop = [torch.empty(NP * CW * CH * 4, dtype=torch.uint8, device="cuda") for _ in sets]
    i420_crop = [torch.empty(NP * n420, dtype=torch.uint8, device="cuda") for _ in sets]
    copy_dst = [torch.empty(NP * n420, dtype=torch.uint8, device="cuda") for _ in sets]
    st = torch.cuda.current_stream().cuda_stream
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs = {
        "crop_rgba": (lambda i: chk(L.h264mi_crop_device_pitch(d_in[i].data_ptr(), rgba_crop[i].data_ptr(), W, H, cpitch, 0, 0,
                                                             CW, CH, 1, NP, slot, CW * CH * 4, st)),
                      NP * CW * CH * 4, NP * CW * CH * 3 // 2),
        "yuv2rgba_full": (lambda i: chk(L.h264mi_yuv2rgba_device_pitch(d_in[i].data_ptr(), rgba_full[i].data_ptr(), W, H, cpitch,
                                                                     NP, slot, W * H * 4, st)),
                          NP * W * H * 4, NP * W * H * 3 // 2),
        "crop_i420": (lambda i: chk(L.h264mi_crop_device_pitch(d_in[i].data_ptr(), i420_crop[i].data_ptr(), W, H, cpitch, 0, 0,
                                                             CW, CH, 0, NP, slot, n420, st)),
                      NP * n420, NP * n420),
        "memcpy_d2d": (lambda i: chk(hip.hipMemcpyAsync(copy_dst[i].data_ptr(), d_in[i].data_ptr(), NP * n420, D2D, st)),
                       NP * n420, NP * n420),
    }
    us = {k: [] for k in legs}
    for k, (f, _, _) in legs.items():                   # warm-up: code objects, every shape
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
    for k, (_, wbytes, rbytes) in legs.items():
        s = stats(us[k])
        s["output_bytes"] = wbytes
        s["ps_per_output_byte"] = round(s["median_us"] * 1e6 / wbytes, 3)
        bps = (wbytes + rbytes) / (s["median_us"] * 1e-6)
        s["bytes_per_s_read_plus_written"] = round(bps)
        s["kernel_share_of_hbm_peak"] = round(bps / HBM_PEAK, 3)
        out[k] = s
    for a, b in (("crop_rgba", "yuv2rgba_full"), ("crop_i420", "memcpy_d2d")):
        spread = (out[b]["max_us"] - out[b]["min_us"]) * 1e6 / out[b]["output_bytes"]
        over = out[a]["ps_per_output_byte"] - out[b]["ps_per_output_byte"]
        iqr = out[b]["iqr_us"] * 1e6 / out[b]["output_bytes"]
        out[a + "_vs_" + b] = {"extra_ps_per_output_byte": round(over, 3),
                               "comparator_spread_ps_per_output_byte": round(spread, 3),
                               "within_comparator_spread": bool(over <= spread),
                               "comparator_iqr_ps_per_output_byte": round(iqr, 3),
                               "within_comparator_iqr": bool(over <= iqr)}
    return out


def read_leg(torch, L):
    eng = Engine(W // 16, H // 16, 1, 2)
    dst = torch.empty(CW * CH * 3 // 2, dtype=torch.uint8).pin_memory()
    full = torch.empty(W * H * 3 // 2, dtype=torch.uint8).pin_memory()

    hip = hip_runtime()
    vp, sz = C.c_void_p, C.c_size_t
    hip.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, C.c_int, vp]
    hip.hipMemcpy2DAsync.restype = C.c_int
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipStreamSynchronize.restype = C.c_int
    D2H = 2
    src = L.h264mi_engine_frame_ptr(eng._h, 0, 0)
    cpitch = L.h264mi_engine_chroma_pitch(eng._h)

    def crop():
        if L.h264mi_engine_read_crop(eng._h, 0, 0, 0, 0, CW, CH, 0, dst.data_ptr()) != 0:
            raise RuntimeError("read_crop failed")

    def copy2d():
        # what h264mi_engine_read_crop does, with the kernel and its copy
        # replaced by one strided copy per plane (null stream)
        rc = L.h264mi_engine_sync(eng._h)
        d, cw2, ch2 = dst.data_ptr(), CW // 2, CH // 2
        su = src + W * H
        rc |= hip.hipMemcpy2DAsync(d, CW, src, W, CW, CH, D2H, None)
        rc |= hip.hipMemcpy2DAsync(d + CW * CH, cw2, su, cpitch, cw2, ch2, D2H, None)
        rc |= hip.hipMemcpy2DAsync(d + CW * CH + cw2 * ch2, cw2, su + cpitch * (H // 2), cpitch, cw2, ch2, D2H, None)
        rc |= hip.hipStreamSynchronize(None)
        if rc != 0:
            raise RuntimeError("strided copies failed")

    legs = {"kernel_plus_one_d2h": crop, "three_memcpy2d": copy2d,
            "uncropped_read": lambda: L.h264mi_engine_read(eng._h, 0, 0, full.data_ptr())}
    us = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(5):
            f()
    for _ in range(SAMPLES * 2):
        for k, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(5):
                f()
            us[k].append((time.perf_counter() - t0) * 1e6 / 5)
    out = {k: stats(v) for k, v in us.items()}
    out["faster"] = min(("kernel_plus_one_d2h", "three_memcpy2d"), key=lambda k: out[k]["median_us"])
    return out


def host_leg():
    exe = os.path.join(_lib.LIB_DIR, "h264mi_dec")
    loop = os.path.join(ROOT, "tools", "ubench", "crop_loop")
    if not os.path.exists(loop):
        subprocess.run(["cc", "-O2", loop + ".c", "-o", loop], check=True)
    stream = gen.generate(3, 100, nframes=60)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s100.h264")
        open(src, "wb").write(stream)
        for name, extra in (("h264mi_dec_C", ["-C"]), ("h264mi_dec", [])) * 2:     # alternating, second pass kept
            r = subprocess.run([exe, "-Onone", "-T", "-r3"] + extra + [src], capture_output=True, text=True, check=True)
            kv = dict(l.split(None, 1) for l in r.stdout.splitlines() if " " in l)
            pics = int(kv["pictures"].split()[0])
            out[name] = {"pictures": pics,
                         "decode_thread_cpu_us_per_picture": round(float(kv["cpu_decode_threads_seconds"]) * 1e6 / pics, 1),
                         "process_cpu_us_per_picture": round(float(kv["cpu_seconds"]) * 1e6 / pics, 1),
                         "t_copy_us_per_picture": round(float(kv["t_copy"]) * 1e6 / pics, 1)}
    r = subprocess.run([loop, str(W), str(H), "0", "0", str(CW), str(CH), "200"], capture_output=True, text=True, check=True)
    out["host_byte_loop_us_per_picture"] = float(r.stdout.split()[1])
    out["h264mi_dec_plus_host_byte_loop_us_per_picture"] = round(
        out["h264mi_dec"]["decode_thread_cpu_us_per_picture"] + out["host_byte_loop_us_per_picture"], 1)
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "crop_cost.py measures on the GPU"
    L = _lib.mi()
    res = {"shape": {"pictures": NP, "coded": [W, H], "crop": [0, 0, CW, CH], "samples": SAMPLES, "launches_per_sample": REPS,
                     "buffer_sets_rotated": NSETS},
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "a_kernel": kernel_leg(torch, L), "b_engine_read": read_leg(torch, L), "c_host_cpu": host_leg()}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "crop_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
