"""Diagnostics (not a test): what the letterboxed tensor export costs
(resize.hip k_tensor_resize's FIT rows) against code this export
leaves alone.  One process, device events, warm-up, legs alternating; writes
profiles/letterbox_cost.json (or the path given).  Conventions of
tools/resize_cost.py and tools/rois_cost.py.

(a) one 1920x1080 crop window of a 1920x1088 frame slot into a 640x640 RGB
    fp16 canvas, pad 114, scale 1/255 (content 640x360 between two 140-row
    bars):
      fit_1080p        one h264mi_tensor_fit_device_pitch call (one launch)
      three_ops_1080p  what a caller does today: a fill of the canvas with the
                       pad element (torch fill_), h264mi_tensor_resize_device_pitch
                       into a (3, 360, 640) temporary, and a strided device
                       copy of it into the canvas (torch copy_)
    The bar: the one call takes no longer than the three operations (medians).
(b) tools/rois_cost.py's 32 boxes on eight 1080p pictures into 224x224 RGB fp16:
      rois_fit_32      one h264mi_tensor_rois_fit_device_pitch call, every box
                       letterboxed
      rois_32          the existing h264mi_tensor_rois_device_pitch call, every
                       box stretched
    The ratio is reported; it is not a bar.
Consecutive repetitions rotate through NSETS input and output buffer sets.
Before anything is timed the outputs are compared: (a)'s two ways must give the
same bytes, and in (b) every letterboxed box must be the single-window
letterboxed export of that window and the list with fit = stretch the existing
call's bytes.

A sample is the device time between two events around REPS repetitions of a
leg, so it holds what the host's enqueue rate leaves idle on the device too --
what a caller sees.  host_enqueue_us is the host's own time to queue one
repetition (no synchronisation inside).

Usage: python tools/letterbox_cost.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import fit_desc, letterbox_fit, rois_desc, tensor_desc  # noqa: E402
from rois_cost import BOXES, CH, CW, H, NP, W, stats  # noqa: E402

SAMPLES, REPS, NSETS = 15, 40, 6
CANVAS = (640, 640)                                     # (oh, ow) of (a)
SIZE = (224, 224)                                       # (oh, ow) of (b)
PAD = 114


def main():
    import torch
    assert torch.cuda.is_available(), "letterbox_cost.py measures on the GPU"
    L = _lib.mi()
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    zero = (C.c_size_t * 1)(0)
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    # (a)
    window = (0, 0, CW, CH)
    rw, rh, px, py = letterbox_fit(CW, CH, CANVAS)
    assert (rw, rh, px, py) == (640, 360, 0, 140)
    rdesc, planes, _ = tensor_desc(window, "rgb", torch.float16, size=CANVAS)
    fdesc = fit_desc(rdesc, planes, "letterbox", PAD)
    inner = tensor_desc(window, "rgb", torch.float16, size=(rh, rw))[0]
    # the pad element: fma(114, 1/255, 0) in fp32, rounded once to fp16
    pad_elem = float((torch.tensor(float(PAD), dtype=torch.float32) * torch.tensor(rdesc.t.scale[0], dtype=torch.float32))
                     .to(torch.float16))
    o_fit = [torch.zeros((3,) + CANVAS, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    o_ops = [torch.zeros((3,) + CANVAS, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    tmp = [torch.zeros((3, rh, rw), dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    canvas_bytes = 3 * CANVAS[0] * CANVAS[1] * 2

    def fit_1080p(i):
        chk(L.h264mi_tensor_fit_device_pitch(d_in[i].data_ptr(), zero, 1, W, H, cpitch, C.byref(fdesc), o_fit[i].data_ptr(),
                                             canvas_bytes, st))

    def three_ops_1080p(i):
        o_ops[i].fill_(pad_elem)
        chk(L.h264mi_tensor_resize_device_pitch(d_in[i].data_ptr(), zero, 1, W, H, cpitch, C.byref(inner),
                                                tmp[i].data_ptr(), 3 * rh * rw * 2, st))
        o_ops[i][:, py:py + rh, px:px + rw].copy_(tmp[i])

    # (b)
    n = len(BOXES)
    stride = 3 * SIZE[0] * SIZE[1] * 2
    sdesc, arr, _, _ = rois_desc(BOXES, SIZE, NP, W, H, "rgb", torch.float16)
    ldesc = rois_desc(BOXES, SIZE, NP, W, H, "rgb", torch.float16, fit="letterbox", pad=PAD)[0]
    o_rfit = [torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]
    o_rois = [torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda") for _ in range(NSETS)]

    def rois_fit_32(i):
        chk(L.h264mi_tensor_rois_fit_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(ldesc), arr, n,
                                                  o_rfit[i].data_ptr(), stride, st))

    def rois_32(i):
        chk(L.h264mi_tensor_rois_device_pitch(d_in[i].data_ptr(), offs, NP, W, H, cpitch, C.byref(sdesc), arr, n,
                                              o_rois[i].data_ptr(), stride, st))

    legs = {"fit_1080p": fit_1080p, "three_ops_1080p": three_ops_1080p, "rois_fit_32": rois_fit_32, "rois_32": rois_32}
    for f in legs.values():                             # warm-up: code objects, every buffer set
        for i in range(NSETS):
            f(i)
    torch.cuda.synchronize()
    same = {"a_one_call_vs_three_ops": all(torch.equal(a, b) for a, b in zip(o_fit, o_ops)) and
            bool((o_fit[0][:, py:py + rh] != pad_elem).any()) and bool((o_fit[0][:, :py] == pad_elem).all())}
    one = torch.zeros((3,) + SIZE, dtype=torch.float16, device="cuda")
    per_box = True
    for r, b in enumerate(BOXES):
        d = fit_desc(tensor_desc(b[1:], "rgb", torch.float16, size=SIZE)[0], 3, "letterbox", PAD)
        chk(L.h264mi_tensor_fit_device_pitch(d_in[0].data_ptr(), (C.c_size_t * 1)(b[0] * slot), 1, W, H, cpitch, C.byref(d),
                                             one.data_ptr(), stride, st))
        per_box = per_box and torch.equal(one, o_rfit[0][r])
    same["b_box_vs_single_window_fit"] = per_box
    stretch = rois_desc(BOXES, SIZE, NP, W, H, "rgb", torch.float16, fit="stretch", pad=PAD)[0]
    o_st = torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda")
    chk(L.h264mi_tensor_rois_fit_device_pitch(d_in[0].data_ptr(), offs, NP, W, H, cpitch, C.byref(stretch), arr, n,
                                              o_st.data_ptr(), stride, st))
    same["b_stretch_vs_existing_call"] = torch.equal(o_st, o_rois[0])
    assert all(same.values()), f"different bytes: {same}"

    us = {k: [] for k in legs}
    host = {k: [] for k in legs}
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
    fits = [letterbox_fit(b[3], b[4], SIZE) for b in BOXES]
    res = {"shape": {"coded": [W, H], "mode": "rgb", "dtype": "float16", "pad": PAD,
                     "a": {"window": list(window), "canvas_oh_ow": list(CANVAS), "fit_rw_rh_px_py": [rw, rh, px, py]},
                     "b": {"pictures": NP, "size_oh_ow": list(SIZE), "boxes_k_x_y_cw_ch": [list(b) for b in BOXES],
                           "fits_rw_rh_px_py": [list(f) for f in fits],
                           "content_share_of_canvas": round(sum(f[0] * f[1] for f in fits) / (n * SIZE[0] * SIZE[1]), 3)},
                     "samples": SAMPLES, "repetitions_per_sample": REPS, "buffer_sets_rotated": NSETS},
           "outputs_identical": same, "legs": {}}
    for k in legs:
        s = stats(us[k])
        s["host_enqueue_us"] = round(statistics.median(host[k]), 2)
        res["legs"][k] = s
    a, b = res["legs"]["fit_1080p"], res["legs"]["three_ops_1080p"]
    res["bar_a"] = {"one_call_median_us": a["median_us"], "three_ops_median_us": b["median_us"],
                    "one_call_over_three_ops": round(a["median_us"] / b["median_us"], 3),
                    "meets_bar": bool(a["median_us"] <= b["median_us"])}
    a, b = res["legs"]["rois_fit_32"], res["legs"]["rois_32"]
    res["ratio_b"] = {"letterboxed_median_us": a["median_us"], "stretched_median_us": b["median_us"],
                      "letterboxed_over_stretched": round(a["median_us"] / b["median_us"], 3)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "letterbox_cost.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
