"""Diagnostics (not a test): the colour sets of the RGB tensor exports (DESIGN
3.5f) -- did the default export move, and what does a colour set cost.  One
process, device events, warm-up, 15 samples of 24 launches, legs alternating,
rotating buffer sets; writes profiles/colour_cost.json (or --out).
Conventions of tools/tensor_cost.py and tools/resize_cost.py.

8 pictures 1920x1088 in the frame-slot layout, window 1920x1080, RGB:
full-size uint8 and fp16 (h264mi_tensor_device_pitch) and fp16 -> 224x224
(h264mi_tensor_resize_device_pitch).  Inputs rotate through 12 sets (307 MB,
more than the 256 MB Infinity Cache holds), outputs through 6.

(a) the default did not move (with --parent-lib DIR, a build of the parent
    commit's libh264mi.so loaded beside this one; only the two stateless
    entry points are called in it): the default legs of both libraries
    alternate in this process; this library's median must lie within the
    parent's own min..max of the same leg.
(b) what the colour costs: the same export with colour set 2 (BT.709 limited:
    the COL instantiations, six integers from the kernel arguments) against
    the default leg of the same dtype in this run -- same bytes moved, so the
    bar of DESIGN 3.5a is: median no more than the default's median plus the
    default's own spread (max - min).

Usage: python tools/colour_cost.py [--parent-lib DIR] [--out out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from broadway_amd import _lib  # noqa: E402
from broadway_amd.engine import tensor_desc  # noqa: E402

W, H, CW, CH, NP = 1920, 1088, 1920, 1080, 8
SAMPLES, REPS, NSETS_IN, NSETS_OUT = 15, 24, 12, 6
SIZE = (224, 224)


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "iqr_us": round(q[2] - q[0], 2), "samples_us": [round(u, 2) for u in us]}


def load_parent(path):
    """The parent build beside ours: RTLD_LOCAL, the two stateless calls."""
    L = C.CDLL(os.path.join(path, "libh264mi.so"), mode=C.RTLD_LOCAL)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, d in (("h264mi_tensor_device_pitch", _lib.TensorDesc), ("h264mi_tensor_resize_device_pitch", _lib.TensorResizeDesc)):
        f = getattr(L, name)
        f.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, C.POINTER(d), vp, sz, vp]
        f.restype = i32
    return L


def run(torch, libs):
    cpitch = 1024                                       # H264MI_CPITCH(120)
    slot = W * H + cpitch * H
    gen_ = torch.Generator(device="cuda").manual_seed(3)
    rbytes = NP * CW * CH * 3 // 2
    d_in = [torch.randint(0, 256, (NP * slot,), dtype=torch.uint8, device="cuda", generator=gen_) for _ in range(NSETS_IN)]
    offs = (C.c_size_t * NP)(*[k * slot for k in range(NP)])
    st = torch.cuda.current_stream().cuda_stream

    def chk(rc):
        if rc != 0:
            raise RuntimeError("launch failed")

    legs, keep = {}, []
    for dtype, size in ((torch.uint8, None), (torch.float16, None), (torch.float16, SIZE)):
        oh, ow = size or (CH, CW)
        outs = [torch.empty((NP, 3, oh, ow), dtype=dtype, device="cuda") for _ in range(NSETS_OUT)]
        stride = 3 * oh * ow * outs[0].element_size()
        base = f"{'resize' if size else 'tensor'}_rgb_{str(dtype).split('.')[1]}" + (f"_{oh}x{ow}" if size else "")
        for lib, L in libs.items():
            for colour in ((None, "bt709") if lib == "this" else (None,)):
                desc = tensor_desc((0, 0, CW, CH), "rgb", dtype, size=size, colour=colour)[0]
                call = L.h264mi_tensor_resize_device_pitch if size else L.h264mi_tensor_device_pitch
                keep.append((desc, outs))

                def f(i, call=call, desc=desc, outs=outs, stride=stride):
                    chk(call(d_in[i % NSETS_IN].data_ptr(), offs, NP, W, H, cpitch, C.byref(desc),
                             outs[i % NSETS_OUT].data_ptr(), stride, st))
                legs[f"{lib}:{base}" + (f"_{colour}" if colour else "")] = (f, NP * stride)
    us = {k: [] for k in legs}
    for f, _ in legs.values():                          # warm-up: code objects, every shape
        for i in range(NSETS_IN):
            f(i)
    torch.cuda.synchronize()
    for _ in range(SAMPLES):
        for k, (f, _) in legs.items():                  # alternating, same process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(REPS):
                f(r)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    out = {}
    for k, (_, wbytes) in legs.items():
        s = stats(us[k])
        s["bytes_read"], s["bytes_written"] = rbytes, wbytes
        s["ps_per_byte_moved"] = round(s["median_us"] * 1e6 / (rbytes + wbytes), 3)
        out[k] = s
    res = {"legs": out, "a_default_did_not_move": {}, "b_colour_cost": {}}
    for k in [k for k in legs if k.startswith("this:") and not k.endswith("_bt709")]:
        name = k.split(":", 1)[1]
        d = out[k]
        if "parent:" + name in out:
            p = out["parent:" + name]
            res["a_default_did_not_move"][name] = {
                "parent_median_us": p["median_us"], "parent_min_us": p["min_us"], "parent_max_us": p["max_us"],
                "this_median_us": d["median_us"],
                "within_parent_min_max": bool(p["min_us"] <= d["median_us"] <= p["max_us"])}
        c = out[k + "_bt709"]
        spread = round(d["max_us"] - d["min_us"], 2)
        moved = d["bytes_read"] + d["bytes_written"]
        res["b_colour_cost"][name] = {
            "default_median_us": d["median_us"], "default_spread_us": spread, "bar_us": round(d["median_us"] + spread, 2),
            "colour_median_us": c["median_us"], "meets_bar": bool(c["median_us"] <= d["median_us"] + spread),
            "extra_ps_per_byte_moved": round((c["median_us"] - d["median_us"]) * 1e6 / moved, 3),
            "default_spread_ps_per_byte_moved": round(spread * 1e6 / moved, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="directory of a build of the parent commit's libh264mi.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_cost.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "colour_cost.py measures on the GPU"
    libs = {"this": _lib.mi()}
    if a.parent_lib:
        libs = {"parent": load_parent(a.parent_lib), "this": libs["this"]}
    res = {"shape": {"pictures": NP, "coded": [W, H], "window": [0, 0, CW, CH], "mode": "rgb", "colour": "bt709 (id 2)",
                     "resize_oh_ow": SIZE, "samples": SAMPLES, "launches_per_sample": REPS,
                     "input_sets_rotated": NSETS_IN, "output_sets_rotated": NSETS_OUT,
                     "parent_library_loaded": bool(a.parent_lib)}}
    res.update(run(torch, libs))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}, indent=1))


if __name__ == "__main__":
    main()
