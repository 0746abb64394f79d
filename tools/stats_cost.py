"""Diagnostics (not a test): what the statistics export (stats.hip)
costs against what a caller does without it -- the uint8 export of the same
samples into a preallocated tensor, then torch on the device: one bincount over
all planes, sum, an int64 square-sum, amin / amax, and the abs and squared
difference sums against the reference's export.  Conventions of
tools/dest_cost.py (device events, warm-up, legs alternating, rotating buffer
sets); every leg runs in a process of its own under a time limit, and the tool
ends at the first one that fails.  Writes profiles/stats_cost.json (or the path
given).

Four workloads on 1920x1088 pictures (packed I420), window 1920x1080:
  y_moments       eight pictures, Y, no histogram, no reference
  yuv_hist        eight pictures, YUV with the histogram
  rgb_hist_ref    eight pictures, RGB (BT.709) with the histogram against eight reference pictures
  boxes_rgb_hist  rois_cost.py's 32 boxes (64x128 .. 640x480) over the eight pictures, RGB with the histogram
each on two contents -- `decoded`: pictures of gen.generate(3, 100) through the
engine; `flat`: every sample 128, the histogram's worst case -- and two legs:
  <w>/<content>/stats     h264mi_stats_device_pitch
  <w>/<content>/baseline  export + torch (the baseline of yuv_hist exports packed
                          I420 through h264mi_crop_device_pitch: the tensor export has no chroma planes; the
                          boxes take one unresized export per box)
Before anything is timed the two legs' integers are compared.  There is no bar:
the ratio stats / baseline is reported, and one above 1 on a 1080p leg is a
finding for DESIGN.

Usage: python tools/stats_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from broadway_amd import _lib, gen  # noqa: E402
from broadway_amd.engine import Capture, Engine, stats_desc, tensor_desc  # noqa: E402
from rois_cost import BOXES, CH, CW, H, NP, W, stats  # noqa: E402

SAMPLES, REPS, NSETS = 15, 20, 4
WORKLOADS = ("y_moments", "yuv_hist", "rgb_hist_ref", "boxes_rgb_hist")
CONTENTS = ("decoded", "flat")
LEG_TIMEOUT = 240           # seconds, per child process


def pictures(content, torch):
    """NSETS device buffers of 2 * NP packed I420 pictures each (the second NP: the references), and a picture's bytes."""
    pic = W * H * 3 // 2
    if content == "flat":
        return [torch.full((2 * NP * pic,), 128, dtype=torch.uint8, device="cuda") for _ in range(NSETS)], pic
    cap = Capture(gen.generate(3, 100, nframes=2 * NP + NSETS))
    assert cap.errors == 0 and (cap.w_mbs * 16, cap.h_mbs * 16) == (W, H) and cap.npics >= 2 * NP + NSETS - 1
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    host = []
    for p in cap.pictures[:2 * NP + NSETS - 1]:
        eng.decode([0], [p])
        host.append(torch.from_numpy(eng.read(0, p.cur_slot).copy()))
    eng.close()
    return [torch.cat(host[i:i + 2 * NP]).to("cuda") for i in range(NSETS)], pic


def leg_main(workload, content, path):
    import torch
    assert torch.cuda.is_available(), "stats_cost.py measures on the GPU"
    L = _lib.mi()
    st = torch.cuda.current_stream().cuda_stream
    d_in, pic = pictures(content, torch)
    cp = W // 2
    offs = (C.c_size_t * NP)(*[k * pic for k in range(NP)])
    roffs = (C.c_size_t * NP)(*[(NP + k) * pic for k in range(NP)])
    window = (0, 0, CW, CH)
    planes, hist, ref, boxes = {"y_moments": ("y", False, False, None), "yuv_hist": ("yuv", True, False, None),
                                "rgb_hist_ref": ("rgb", True, True, None), "boxes_rgb_hist": ("rgb", True, False, BOXES)}[workload]
    colour = "bt709" if planes == "rgb" else None
    desc, arr, P, Lw = stats_desc(planes, None if boxes else window, boxes, hist, colour, NP, W, H)
    items = len(boxes) if boxes else NP
    out_new = [torch.zeros((items, P, Lw), dtype=torch.int64, device="cuda") for _ in range(NSETS)]
    out_old = [torch.zeros((items, P, Lw), dtype=torch.int64, device="cuda") for _ in range(NSETS)]

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    def new(i):
        chk(L.h264mi_stats_device_pitch(d_in[i].data_ptr(), offs, d_in[i].data_ptr() if ref else None, roffs if ref else None, NP,
                                        W, H, cp, C.byref(desc), arr, len(boxes) if boxes else 0, out_new[i].data_ptr(),
                                        P * Lw * 8, st))

    def torch_stats(o, s, r=None):
        """o (n, P, L) from the samples s (n, P, rows, cols) uint8 (and r): what a caller writes today."""
        n = s.shape[0]
        v = s.reshape(n * P, -1)
        w = v.to(torch.int64)
        o[:, :, 0] = v.shape[1]
        o[:, :, 1] = w.sum(1).view(n, P)
        o[:, :, 2] = (w * w).sum(1).view(n, P)
        o[:, :, 3] = v.amin(1).view(n, P)
        o[:, :, 4] = v.amax(1).view(n, P)
        if r is not None:
            d = w - r.reshape(n * P, -1).to(torch.int64)
            o[:, :, 5] = d.abs().sum(1).view(n, P)
            o[:, :, 6] = (d * d).sum(1).view(n, P)
        if hist:
            base = torch.arange(n * P, device=v.device, dtype=torch.int64).view(-1, 1) * 256
            o[:, :, 8:] = torch.bincount((w + base).view(-1), minlength=n * P * 256).view(n, P, 256)

    if planes == "yuv":
        tmp = [torch.empty((NP, CW * CH * 3 // 2), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]

        def old(i):
            chk(L.h264mi_crop_device_pitch(d_in[i].data_ptr(), tmp[i].data_ptr(), W, H, cp, 0, 0, CW, CH, 0, NP, pic,
                                           CW * CH * 3 // 2, st))
            torch_stats(out_old[i][:, :1], tmp[i][:, :CW * CH].view(NP, 1, CH, CW))
            torch_stats(out_old[i][:, 1:], tmp[i][:, CW * CH:].view(NP, 2, CH // 2, CW // 2))
    elif boxes:
        tds = [tensor_desc((x, y, cw, ch), "rgb", torch.uint8, colour=colour)[0] for _, x, y, cw, ch in boxes]
        tmp = [[torch.empty((1, 3, ch, cw), dtype=torch.uint8, device="cuda") for _, _, _, cw, ch in boxes] for _ in range(NSETS)]
        one = [(C.c_size_t * 1)(k * pic) for k, *_ in boxes]

        def old(i):
            for b, (td, t) in enumerate(zip(tds, tmp[i])):
                chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), one[b], 1, W, H, cp, C.byref(td), t.data_ptr(), t.numel(), st))
                torch_stats(out_old[i][b:b + 1], t)
    else:
        mode = "rgb" if planes == "rgb" else "gray"
        td = tensor_desc(window, mode, torch.uint8, colour=colour)[0]
        tmp = [torch.empty((NP, P, CH, CW), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        rtmp = [torch.empty((NP, P, CH, CW), dtype=torch.uint8, device="cuda") for _ in range(NSETS)] if ref else None

        def old(i):
            chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cp, C.byref(td), tmp[i].data_ptr(), P * CH * CW, st))
            if ref:
                chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), roffs, NP, W, H, cp, C.byref(td), rtmp[i].data_ptr(),
                                                 P * CH * CW, st))
            torch_stats(out_old[i], tmp[i], rtmp[i] if ref else None)
    legs = {"stats": new, "baseline": old}
    for f in legs.values():                             # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(out_new, out_old)) and bool(out_new[0].any())
    assert same, "the two legs' integers differ"
    us, host = {k: [] for k in legs}, {k: [] for k in legs}
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
    res = {"outputs_identical": same, "legs": {}}
    for k in legs:
        res["legs"][k] = dict(stats(us[k]), host_enqueue_us=round(statistics.median(host[k]), 2))
    res["stats_over_baseline"] = round(res["legs"]["stats"]["median_us"] / res["legs"]["baseline"]["median_us"], 3)
    with open(path, "w") as f:
        json.dump(res, f)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stats_cost.json")
    res = {"shape": {"coded": [W, H], "window": [0, 0, CW, CH], "pictures": NP, "boxes": len(BOXES), "layout": "packed I420",
                     "rgb_colour": "bt709", "samples": SAMPLES, "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS,
                     "decoded": "gen.generate(3, 100) through the engine", "flat": 128},
           "workloads": {}}
    part = path + ".part"
    for w in WORKLOADS:
        for c in CONTENTS:
            try:                                        # one process and one time limit per leg pair; the first failure ends the tool
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", w, c, part], timeout=LEG_TIMEOUT)
            except subprocess.TimeoutExpired:
                sys.exit(f"stats_cost.py: {w}/{c} ran into its time limit of {LEG_TIMEOUT} s; nothing more is started")
            if p.returncode != 0:
                sys.exit(f"stats_cost.py: {w}/{c} failed ({p.returncode}); nothing more is started")
            with open(part) as f:
                res["workloads"].setdefault(w, {})[c] = json.load(f)
            os.remove(part)
            print(w, c, json.dumps(res["workloads"][w][c]), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        leg_main(*sys.argv[2:])
    else:
        main()
