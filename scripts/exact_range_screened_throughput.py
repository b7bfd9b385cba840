#!/usr/bin/env python3
"""Screened exact range search throughput: Builder.exact_range / exact_range_count(screened=True) of this commit
against the same calls without `screened` of a library built from the parent commit, in alternating processes.

  python scripts/exact_range_screened_throughput.py --parent-root ../parent --n 1000000 --dim 128 --metric cosine --hits 100

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (6) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout and times exact_range_count_f32 and exact_range_f32, then a child that imports this tree's and times
both with screened=True.  A child loads n x dim normal rows on a ring graph (the calls never read the graph), takes as
each query's radius the distance of its --hits-th nearest item (exact_knn_f32), runs each call once as a warm-up (the
first screened call also makes the per-slot sums of squares), then --inner (3) times, and reports the medians: one
figure per call and process.  The driver writes, per shape, the median and min … max of the six figures of each side
and call, the screen's stats per query (certain and settled pairs of the counts call and of the hits call) and, from
one more pair of screened calls on a profiling builder, the device time of the scans and of the settling, to
profiles/exact_range_screened_throughput.json (OUT=path overrides; a run adds its shape to the file it finds).  The
screened child also runs this tree's unscreened calls once and checks that the results are identical.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "exact_range_screened_throughput.json"


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
        radius = b.exact_knn_f32(q, k=a.hits)[1][:, a.hits - 1].copy()

        def timed(call, **more):
            t0 = time.perf_counter()
            r = call(q, radius, **kw, **more)
            return time.perf_counter() - t0, r

        for name, call in (("count", b.exact_range_count_f32), ("hits", b.exact_range_f32)):
            _, got = timed(call)
            res[name + "_seconds"] = statistics.median(timed(call)[0] for _ in range(a.inner))
            if name == "hits":
                res["hits_per_query"] = float(got[0][-1]) / a.queries
            if not kw:
                continue
            stats = b.exact_range_screen_stats()
            want = getattr(b, "exact_range_count_f32" if name == "count" else "exact_range_f32")(q, radius)
            pairs = zip(got, want) if name == "hits" else [(got, want)]
            res[name + "_identical"] = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in pairs)
            b.set_profiling(True)
            timed(call)
            b.set_profiling(False)
            res[name + "_stats"] = {"n_screened": stats[0], "n_routed": stats[1],
                                    "certain_per_query": stats[2] / max(stats[0], 1),
                                    "settled_per_query": stats[3] / max(stats[0], 1),
                                    "device_time_split": dict(zip(("scan_ms", "settle_ms"), b.exact_range_screen_times()))}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "euclidean"])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--hits", type=int, default=100)
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
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--metric", a.metric, "--queries", str(a.queries), "--hits",
             str(a.hits), "--inner", str(a.inner)]
    env = {k: v for k, v in os.environ.items() if k != "HNY_LIB"}
    sides = {"plain": [], "screened": []}
    for _ in range(a.processes):
        for side, root in (("plain", a.parent_root), ("screened", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))

    def summary(rs, key):
        t = [r[key] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last = sides["screened"][-1]
    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "hits_asked": a.hits,
           "hits_per_query": last["hits_per_query"], "processes": a.processes, "inner": a.inner, "device": last["device"],
           "identical_results": all(r["count_identical"] and r["hits_identical"] for r in sides["screened"])}
    for name in ("count", "hits"):
        res[name] = {"parent": summary(sides["plain"], name + "_seconds"),
                     "screened": summary(sides["screened"], name + "_seconds"), **last[name + "_stats"]}
        res[name]["screened_median_below_parent_min"] = res[name]["screened"]["median_s"] < res[name]["parent"]["min_s"]
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_{a.metric}_q{a.queries}_h{a.hits}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit("the screened range calls and their namesakes disagree")


if __name__ == "__main__":
    main()
