"""Diagnostics (not a test): A/B of the export cost tools between two builds of
the library in one GPU call, as tools/ab.sh does for the bench -- box-to-box
clock variation is larger than what is looked for here.  tools/ab_build.sh
puts builds into abtest/<name>/; this runs tools/tensor_cost.py,
resize_cost.py, rois_cost.py and warp_cost.py ROUNDS times per build,
interleaved (a fresh process each, H264MI_LIB_DIR naming the build; a tool that
exits non-zero ends the run, with one exception: warp_cost.py writes its result
and then judges torch's fp16 grid_sample against the export, and a run that
ends on exactly that assertion is kept and listed under "nonzero_exit"), and
writes profiles/dest_ab.json (or the path given):
per leg of each tool -- every object of its output that has a median and an
IQR -- both builds' median of the rounds' medians and largest IQR, and whether
B's median exceeds A's by no more than the larger of the two IQRs.

Usage (GPU box): python tools/ab_costs.py A B [out.json]     (ROUNDS=3)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["tensor_cost", "resize_cost", "rois_cost", "warp_cost"]
MEDIANS = ("median_us", "median_us_per_picture")
IQRS = ("iqr_us", "iqr_us_per_picture")
KNOWN = "AssertionError: max |warps - grid_sample| beyond 2 / 255"      # warp_cost.py's last line, after its result


def legs(node, path=()):
    """(name, median, iqr) of every object below `node` that holds both."""
    if not isinstance(node, dict):
        return
    m = next((node[k] for k in MEDIANS if k in node), None)
    q = next((node[k] for k in IQRS if k in node), None)
    if m is not None and q is not None:
        yield "/".join(path), float(m), float(q)
        return
    for k, v in node.items():
        yield from legs(v, path + (k,))


def main():
    a, b = sys.argv[1], sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "dest_ab.json")
    rounds = int(os.environ.get("ROUNDS", "3"))
    tmp = os.path.join(ROOT, "build", "ab_costs")
    os.makedirs(tmp, exist_ok=True)
    runs, nonzero = {}, {}
    for r in range(rounds):
        for tool in TOOLS:
            for v in (a, b):
                path = os.path.join(tmp, f"{tool}_{v}_{r}.json")
                env = dict(os.environ, H264MI_LIB_DIR=os.path.join(ROOT, "abtest", v))
                if os.path.exists(path):
                    os.remove(path)
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), path], env=env,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300)
                if p.returncode != 0:
                    last = (p.stderr.strip().splitlines() or [""])[-1]
                    if p.returncode != 1 or not os.path.exists(path) or not last.startswith(KNOWN):
                        sys.exit(f"{tool} on {v} failed ({p.returncode}):\n{p.stderr[-2000:]}")
                    nonzero[f"{tool}/{v}/{r}"] = last[:300]
                with open(path) as f:
                    for name, m, q in legs(json.load(f)):
                        runs.setdefault(f"{tool}/{name}", {}).setdefault(v, []).append((m, q))
                print(f"round {r} {tool} {v}", flush=True)
    res = {"builds": {"a": a, "b": b}, "rounds": rounds, "nonzero_exit": nonzero, "legs": {},
           "b_within_larger_iqr_of_a": True}
    for name, by in sorted(runs.items()):
        ma, mb = (statistics.median(m for m, _ in by[v]) for v in (a, b))
        qa, qb = (max(q for _, q in by[v]) for v in (a, b))
        ok = mb - ma <= max(qa, qb)
        res["legs"][name] = {"a_median_us": round(ma, 2), "a_iqr_us": round(qa, 2), "b_median_us": round(mb, 2),
                             "b_iqr_us": round(qb, 2), "b_over_a": round(mb / ma, 3), "within": bool(ok)}
        res["b_within_larger_iqr_of_a"] = bool(res["b_within_larger_iqr_of_a"] and ok)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
