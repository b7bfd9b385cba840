#!/usr/bin/env python3
"""Screened exact k-NN throughput: Builder.exact_knn(screened=True) of this commit against Builder.exact_knn of a
library built from the parent commit, in alternating processes.

  python scripts/exact_screened_throughput.py --parent-root ../parent --n 1000000 --dim 128 --metric cosine --k 10

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (6) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout and times exact_knn_f32, then a child that imports this tree's and times exact_knn_f32(screened=True).
A child loads n x dim normal rows on a ring graph (neither call reads the graph), runs its call once as a warm-up (the
first screened call also makes the per-slot sums of squares), then --inner (3) times, and reports the median of those:
one figure per process.  The driver writes, per shape, the median and min … max of the six figures of each side, the
screen's stats (candidates per query, routed queries) and, from one more screened call on a profiling builder, the
split of device time between its five kinds of launch (HIP events around every launch on the builder's stream) to
profiles/exact_screened_throughput.json (OUT=path overrides; a run adds its shape to the file it finds).  The
screened child also runs this tree's exact_knn_f32 once and checks that the two results are identical.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "exact_screened_throughput.json"


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    sys.path.insert(1, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch
    import hannoy_amd as H
    from exact_knn_throughput import Ring
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    assert os.path.abspath(H.__file__).startswith(os.path.abspath(a.root)), H.__file__
    metric = ["cosine", "euclidean"].index(a.metric)
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    kw = {"screened": True} if a.child == "screened" else {}
    res = {"side": a.child, "device": torch.cuda.get_device_name(0)}
    with H.Builder(H.F32ItemSet(metric, x), prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        def timed():
            t0 = time.perf_counter()
            r = b.exact_knn_f32(q, k=a.k, **kw)
            return time.perf_counter() - t0, r

        _, got = timed()
        res["seconds"] = statistics.median(timed()[0] for _ in range(a.inner))
        if kw:
            stats = b.exact_screen_stats()
            want = b.exact_knn_f32(q, k=a.k)
            res["identical_results"] = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
            b.set_profiling(True)
            timed()
            res.update({"n_screened": stats[0], "n_routed": stats[1], "candidates_per_query": stats[2] / max(stats[0], 1),
                        "device_time_split": dict(zip(("scan_hi_ms", "topk_ms", "scan_lo_ms", "collect_ms", "settle_ms"),
                                                      b.exact_screen_times()))})
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "euclidean"])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--processes", type=int, default=6)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--parent-root")
    ap.add_argument("--child", choices=["plain", "screened"])
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root:
        raise SystemExit("--parent-root: a checkout of the parent commit with its library built")
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--metric", a.metric, "--queries", str(a.queries), "--k", str(a.k),
             "--inner", str(a.inner)]
    env = {k: v for k, v in os.environ.items() if k != "HNY_LIB"}
    sides = {"plain": [], "screened": []}
    for _ in range(a.processes):
        for side, root in (("plain", a.parent_root), ("screened", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))

    def summary(rs):
        t = [r["seconds"] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last = sides["screened"][-1]
    split = last["device_time_split"]
    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "k": a.k, "processes": a.processes,
           "inner": a.inner, "device": last["device"], "exact_knn_parent": summary(sides["plain"]),
           "exact_knn_screened": summary(sides["screened"]),
           "identical_results": all(r["identical_results"] for r in sides["screened"]),
           "n_screened": last["n_screened"], "n_routed": last["n_routed"],
           "candidates_per_query": last["candidates_per_query"], "device_time_split": split,
           # the 2 n q d model over both scans
           "model_tflops_scan": 2 * 2.0 * a.queries * a.n * a.dim / 1e12
           / max((split["scan_hi_ms"] + split["scan_lo_ms"]) / 1e3, 1e-9)}
    res["screened_median_below_parent_min"] = res["exact_knn_screened"]["median_s"] < res["exact_knn_parent"]["min_s"]
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_{a.metric}_q{a.queries}_k{a.k}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit("exact_knn(screened=True) and exact_knn disagree")


if __name__ == "__main__":
    main()
