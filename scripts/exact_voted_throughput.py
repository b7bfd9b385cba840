#!/usr/bin/env python3
"""Voted exact k-NN throughput: Builder.exact_knn(screened="votes") of this commit against Builder.exact_knn of a
library built from the parent commit, in alternating processes.

  python scripts/exact_voted_throughput.py --parent-root ../parent --n 1000000 --dim 128 --metric cosine --k 10

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (6) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout and times exact_knn_f32, then a child that imports this tree's and times
exact_knn_f32(screened="votes").  A child loads n x dim normal rows on a ring graph (neither call reads the graph), runs
its call once as a warm-up (the first voted call also makes the per-slot sums of squares), then --inner (3) times, and
reports the median of those: one figure per process.  --sorted draws the rows around 1 000 centres and stores them in
cluster order, ids sorted by cluster: what the spread pilot sample is for.  --pilot FACTOR,MIN sets the two constants
of the pilot's sample size for the voted children (the library's measuring hooks HNY_VOTE_PILOT_FACTOR / _MIN; 0,0: no
pilot); such a run is stored under its own key.  The driver writes, per run, the median and min … max of the six
figures of each side, the pairs the pilot computed and the pairs settled per query and, from one more voted call on a
profiling builder, the device time of the pilot, the scans and the settles (HIP events around every launch on the
builder's stream) to profiles/exact_voted_throughput.json (OUT=path overrides; a run adds itself to the file it
finds).  The voted child also runs this tree's exact_knn_f32 once and checks that the two results are identical.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "exact_voted_throughput.json"


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
    if a.sorted:  # rows around 1 000 centres, stored cluster by cluster; the queries near rows of their own
        centre = np.sort(rng.integers(0, 1000, a.n))
        x = 4 * rng.standard_normal((1000, a.dim), dtype=np.float32)[centre] + x
        q = x[rng.integers(0, a.n, a.queries)] + np.float32(0.5) * q
    kw = {"screened": "votes"} if a.child == "voted" else {}
    res = {"side": a.child, "device": torch.cuda.get_device_name(0)}
    with H.Builder(H.F32ItemSet(metric, x), prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        def timed():
            t0 = time.perf_counter()
            r = b.exact_knn_f32(q, k=a.k, **kw)
            return time.perf_counter() - t0, r

        _, got = timed()
        res["seconds"] = statistics.median(timed()[0] for _ in range(a.inner))
        if kw:
            stats = b.exact_vote_stats()
            want = b.exact_knn_f32(q, k=a.k)
            res["identical_results"] = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
            b.set_profiling(True)
            timed()
            res.update({"n_voted": stats[0], "n_routed": stats[1], "pilot_pairs_per_query": stats[2] / max(stats[0], 1),
                        "settled_pairs_per_query": stats[3] / max(stats[0], 1),
                        "device_time_split": dict(zip(("pilot_ms", "scans_ms", "settles_ms"), b.exact_vote_times()))})
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
    ap.add_argument("--sorted", action="store_true")
    ap.add_argument("--pilot", help="FACTOR,MIN of the pilot's sample size (default: the library's 8,4096)")
    ap.add_argument("--parent-root")
    ap.add_argument("--child", choices=["plain", "voted"])
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root:
        raise SystemExit("--parent-root: a checkout of the parent commit with its library built")
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--metric", a.metric, "--queries", str(a.queries), "--k", str(a.k),
             "--inner", str(a.inner)] + (["--sorted"] if a.sorted else [])
    env = {k: v for k, v in os.environ.items() if k not in ("HNY_LIB", "HNY_VOTE_PILOT_FACTOR", "HNY_VOTE_PILOT_MIN")}
    if a.pilot:
        env["HNY_VOTE_PILOT_FACTOR"], env["HNY_VOTE_PILOT_MIN"] = a.pilot.split(",")
    sides = {"plain": [], "voted": []}
    for _ in range(a.processes):
        for side, root in (("plain", a.parent_root), ("voted", ROOT)):
            if side == "plain" and a.pilot:
                continue  # a sweep point: the parent's figure is the one of the run without --pilot
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))

    def summary(rs):
        t = [r["seconds"] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last = sides["voted"][-1]
    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "k": a.k, "processes": a.processes,
           "inner": a.inner, "rows": "sorted by cluster" if a.sorted else "normal", "pilot": a.pilot or "8,4096",
           "device": last["device"], "exact_knn_voted": summary(sides["voted"]),
           "identical_results": all(r["identical_results"] for r in sides["voted"]),
           **{k: last[k] for k in ("n_voted", "n_routed", "pilot_pairs_per_query", "settled_pairs_per_query",
                                   "device_time_split")}}
    if sides["plain"]:
        res["exact_knn_parent"] = summary(sides["plain"])
        res["voted_median_below_parent_min"] = res["exact_knn_voted"]["median_s"] < res["exact_knn_parent"]["min_s"]
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    key = f"{a.n}x{a.dim}_{a.metric}_q{a.queries}_k{a.k}" + ("_sorted" if a.sorted else "")
    runs[key + (f"_pilot{a.pilot}" if a.pilot else "")] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit('exact_knn(screened="votes") and exact_knn disagree')


if __name__ == "__main__":
    main()
