"""Diagnostics (not a test): what the affine-warped export costs (warp.hip
k_tensor_warp) against what a caller had before it -- the planar
fp16 export of the whole windows, then torch.nn.functional.grid_sample over
them.  One process, device events, warm-up, legs alternating; writes
profiles/warp_cost.json (or the path given).  Conventions of tools/rois_cost.py.

8 pictures 1920x1088 in the frame-slot layout, window 1920x1080; 32 warps, four
per picture: the boxes of tools/rois_cost.py (BOXES, fixed), each turned by a
fixed angle in +-45 degrees about its centre (engine.rotated_box_warp), every
one to RGB fp16 at 112x112 and at 224x224:
  warps_32         one h264mi_tensor_warps_device_pitch call (one launch)
  grid_sample_32   h264mi_tensor_device_pitch of the 8 windows as planar fp16,
                   then one F.grid_sample(bilinear, padding_mode="zeros",
                   align_corners=True) per picture over its four boxes' grids
                   (made once, outside the timed region), fp16 like the export
  grid_sample32_32 the same through fp32 (fp32 export, fp32 grids, the result
                   cast to fp16): what a caller who needs the positions exact
                   to better than fp16's 11 bits would run; for information
  rois_32          h264mi_tensor_rois_device_pitch on the upright boxes at the
                   same sizes: the scale of the existing fused kernel, for
                   information only (it computes something else)
and the same with 4 of the warps on 4 pictures (only those are exported).  The
bar: warps_* is faster than grid_sample_* -- median below, ranges not
overlapping.  Before anything is timed the warped bytes are compared with the
oracle (tests/_warp.py) on the first buffer set, and the float legs with the
warped result: max |a - b| on the unit constants, bound 2 / 255, recorded (the
bound is asserted at the end, after the file is written).

Measured on an MI355X (profiles/warp_cost.json): the bar is met
in all four workloads (warps / grid_sample 0.081 .. 0.124), the bytes equal the
oracle's, and the bound against grid_sample as specified -- fp16 throughout --
is MISSED: max |a - b| 0.451 (112x112) and 0.467 (224x224), because an fp16
grid holds a normalised coordinate to 11 bits, about +-0.5 sample on 1920
columns; against grid_sample32 the maximum is 0.0054 <= 2 / 255.  The assertion
stays on the specified comparator, so this tool ends with an AssertionError
after it has written its file.

A sample is the device time between two events around REPS repetitions of a
leg, so it holds what the host's enqueue rate leaves idle on the device too.

Usage: python tools/warp_cost.py [out.json]"""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import rois_desc, rotated_box_warp, tensor_desc, warps_desc  # noqa: E402
from rois_cost import BOXES, CH, CW, H, NP, W  # noqa: E402

SAMPLES, REPS, NSETS = 15, 40, 6
SIZES = [(112, 112), (224, 224)]                        # (oh, ow)
ANGLES = [((37 * r + 11) % 91) - 45 for r in range(len(BOXES))]        # fixed, -45 .. 45 degrees
FEW = [0, 9, 18, 27]                                    # four warps on four pictures, four box sizes
WINDOW = (0, 0, CW, CH)
BOUND = 2.0 / 255.0


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2), "spread_us": round(max(us) - min(us), 2)}


def warps_of(size, idx):
    """[(k, m)] of the boxes idx at `size`: box (k, x, y, cw, ch) turned by its angle about its centre."""
    return [(BOXES[r][0], rotated_box_warp(BOXES[r][1] + BOXES[r][3] / 2, BOXES[r][2] + BOXES[r][4] / 2, BOXES[r][3],
                                           BOXES[r][4], ANGLES[r], size)) for r in idx]


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    import _crop
    import _warp as Wp
    assert torch.cuda.is_available(), "warp_cost.py measures on the GPU"
    L = _lib.mi()
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    st = torch.cuda.current_stream().cuda_stream
    host0 = d_in[0].cpu().numpy()
    pics0 = [host0[k * slot:(k + 1) * slot] for k in range(NP)]

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, check = {}, {}
    for size in SIZES:
        oh, ow = size
        stride = 3 * oh * ow * 2
        for tag, idx in (("32", list(range(len(BOXES)))), ("4", FEW)):
            name = f"{tag}_{oh}"
            warps = warps_of(size, idx)
            n = len(warps)
            used = sorted({k for k, _ in warps})        # the pictures leg b has to export
            offs_all = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
            offs_used = (C.c_size_t * len(used))(*[k * slot for k in used])
            wd, warr, _, _ = warps_desc(warps, size, NP, WINDOW, W, H, "rgb", torch.float16)
            rd, rarr, _, _ = rois_desc([BOXES[r] for r in idx], size, NP, W, H, "rgb", torch.float16)
            o_warp = [torch.zeros((n, 3, oh, ow), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
            o_rois = [torch.zeros((n, 3, oh, ow), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
            # leg b: per picture, its warps' grids stacked along the rows; normalised with align_corners=True
            per_pic = {k: [r for r, (kk, _) in enumerate(warps) if kk == k] for k in used}
            ii, jj = np.mgrid[0:oh, 0:ow].astype(np.float64)
            grids = {}
            for k, rs in per_pic.items():
                g = []
                for r in rs:
                    m = warps[r][1]
                    x = (m[0] * jj + m[1] * ii + m[2]) / 65536.0
                    y = (m[3] * jj + m[4] * ii + m[5]) / 65536.0
                    g.append(np.stack([2.0 * x / (CW - 1) - 1.0, 2.0 * y / (CH - 1) - 1.0], axis=-1))
                grids[k] = torch.from_numpy(np.concatenate(g, axis=0)[None]).to("cuda")
            variants = {}
            for fdt, label in ((torch.float16, "grid_sample"), (torch.float32, "grid_sample32")):
                td, _, _ = tensor_desc(WINDOW, "rgb", fdt)
                es = 2 if fdt == torch.float16 else 4
                whole = [torch.zeros((len(used), 3, CH, CW), dtype=fdt, device="cuda") for _ in range(2)]
                gr = {k: g.to(fdt) for k, g in grids.items()}
                o = [torch.zeros((n, 3, oh, ow), dtype=torch.float16, device="cuda") for _ in range(NSETS)]

                def leg_b(i, td=td, es=es, whole=whole, gr=gr, o=o, used=used, per_pic=per_pic, offs_used=offs_used, oh=oh):
                    wh = whole[i & 1]
                    chk(L.h264mi_tensor_device_pitch(d_in[i].data_ptr(), offs_used, len(used), W, H, cpitch, C.byref(td),
                                                     wh.data_ptr(), 3 * CH * CW * es, st))
                    for u, k in enumerate(used):
                        s = F.grid_sample(wh[u:u + 1], gr[k], mode="bilinear", padding_mode="zeros", align_corners=True)
                        rs = per_pic[k]
                        # (grid_sample has no out=: its rows are copied into the preallocated output, box by box)
                        o[i][rs[0]:rs[0] + len(rs)].copy_(s[0].view(3, len(rs), oh, -1).transpose(0, 1))
                variants[label] = (leg_b, o)

            def leg_a(i, wd=wd, warr=warr, n=n, o=o_warp, stride=stride):
                chk(L.h264mi_tensor_warps_device_pitch(d_in[i].data_ptr(), offs_all, NP, W, H, cpitch, C.byref(wd), warr, n,
                                                       o[i].data_ptr(), stride, st))

            def leg_c(i, rd=rd, rarr=rarr, n=n, o=o_rois, stride=stride):
                chk(L.h264mi_tensor_rois_device_pitch(d_in[i].data_ptr(), offs_all, NP, W, H, cpitch, C.byref(rd), rarr, n,
                                                      o[i].data_ptr(), stride, st))

            legs[f"warps_{name}"] = (leg_a, n)
            for label, (f, _) in variants.items():
                legs[f"{label}_{name}"] = (f, n)
            legs[f"rois_{name}"] = (leg_c, n)
            check[name] = (warps, size, o_warp, {label: o for label, (_, o) in variants.items()})
            # the warps of a picture are consecutive in the list (leg b's copy relies on it)
            assert all(rs == list(range(rs[0], rs[0] + len(rs))) for rs in per_pic.values())
    for f, _ in legs.values():                          # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()

    # byte equality with the oracle on buffer set 0, before anything is timed
    samples = {}
    verdict = {}
    for name, (warps, size, o_warp, floats) in check.items():
        got = o_warp[0].cpu().numpy().view(np.uint8)
        h = hashlib.sha256()
        for r, (k, m) in enumerate(warps):
            if k not in samples:
                samples[k] = np.ascontiguousarray(Wp.window_samples(
                    _crop.crop_i420(pics0[k], W, H, 0, 0, CW, CH, cpitch=cpitch), CW, CH, "rgb"))
            want = Wp.elements(Wp.warp_planes(samples[k], m, size), "float16", "unit")
            assert np.array_equal(got[r].reshape(-1), want), f"{name}: warp {r} differs from the oracle"
            h.update(want.tobytes())
        assert hashlib.sha256(got.tobytes()).hexdigest() == h.hexdigest()
        a = o_warp[0].float()
        verdict[name] = {"oracle_sha256": h.hexdigest(), "bytes_equal_oracle": True}
        for label, o in floats.items():
            d = float((a - o[0].float()).abs().max())
            verdict[name][f"max_abs_diff_{label}"] = round(d, 6)
            verdict[name][f"{label}_within_2_over_255"] = bool(d <= BOUND)

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
    res = {"shape": {"pictures": NP, "coded": [W, H], "window": list(WINDOW), "mode": "rgb", "dtype": "float16",
                     "sizes_oh_ow": [list(s) for s in SIZES], "boxes_k_x_y_cw_ch": [list(b) for b in BOXES],
                     "angles_deg": ANGLES, "few": FEW, "border": "constant", "pad": 0, "samples": SAMPLES,
                     "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS, "bound": BOUND},
           "checks": verdict, "legs": {}}
    for k, (_, n) in legs.items():
        s = stats(us[k])
        s["warps"] = n
        s["host_enqueue_us"] = round(statistics.median(host[k]), 2)
        res["legs"][k] = s
    for name in check:
        a, b = res["legs"][f"warps_{name}"], res["legs"][f"grid_sample_{name}"]
        res[f"bar_{name}"] = {"warps_median_us": a["median_us"], "grid_sample_median_us": b["median_us"],
                              "warps_over_grid_sample": round(a["median_us"] / b["median_us"], 3),
                              "ranges_overlap": bool(a["max_us"] >= b["min_us"]),
                              "meets_bar": bool(a["median_us"] < b["median_us"] and a["max_us"] < b["min_us"])}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warp_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    missed = [n for n, v in verdict.items() if not v["grid_sample_within_2_over_255"]]
    assert not missed, f"max |warps - grid_sample| beyond 2 / 255: {missed}"


if __name__ == "__main__":
    main()
