#!/usr/bin/env python3
"""Filtered voted exact k-NN throughput: Builder.exact_knn_filtered_f32(screened="votes") of this commit against
Builder.exact_knn_filtered_f32 of a library built from the parent commit, in alternating processes.

  python scripts/exact_filtered_voted_throughput.py --parent-root ../parent --n 1000000 --dim 128 --filters 32

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (3) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout and times exact_knn_filtered_f32, then a child that imports this tree's and times the same call with
screened="votes".  A child loads n x dim normal rows on a ring graph (neither call reads the graph), draws --filters
independent filters of about --density (0.1) of the items, gives query i the filter i % filters, runs its call once as a
warm-up (the first voted call also makes the per-slot sums of squares), then --inner (3) times, and reports the median
of those: one figure per process.  The voted child also runs this tree's plain call once and checks that the two
results are identical, and reports hny_builder_exact_rows_read of both, the vote stats and, from one more voted call on
a profiling builder, the device time of the pilot, the scans (tile masks included) and the settles.  The driver writes
the median and min .. max of each side to profiles/exact_filtered_voted_throughput.json (OUT=path overrides; a run adds
itself to the file it finds).  Acceptance: every figure of the voted side below the parent's minimum.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "exact_filtered_voted_throughput.json"


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
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    filters = [np.flatnonzero(rng.random(a.n) < a.density).astype(np.uint32) for _ in range(a.filters)]
    fof = np.arange(a.queries) % a.filters
    kw = {"screened": "votes"} if a.child == "voted" else {}
    res = {"side": a.child, "device": torch.cuda.get_device_name(0)}
    with H.Builder(H.F32ItemSet(0, x), prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        def timed():
            t0 = time.perf_counter()
            r = b.exact_knn_filtered_f32(q, filters, fof, k=a.k, **kw)
            return time.perf_counter() - t0, r

        _, got = timed()
        res["seconds"] = statistics.median(timed()[0] for _ in range(a.inner))
        res["rows_read"] = b.exact_rows_read()
        if kw:
            stats = b.exact_vote_stats()
            want = b.exact_knn_filtered_f32(q, filters, fof, k=a.k)
            res["rows_read_plain"] = b.exact_rows_read()
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
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--parent-root")
    ap.add_argument("--child", choices=["plain", "voted"])
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root:
        raise SystemExit("--parent-root: a checkout of the parent commit with its library built")
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--filters", str(a.filters), "--density", str(a.density),
             "--queries", str(a.queries), "--k", str(a.k), "--inner", str(a.inner)]
    env = {k: v for k, v in os.environ.items() if k not in ("HNY_LIB", "HNY_EXACT_SKIP")}
    sides = {"plain": [], "voted": []}
    for _ in range(a.processes):
        for side, root in (("plain", a.parent_root), ("voted", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=900).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))

    def summary(rs):
        t = [r["seconds"] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last = sides["voted"][-1]
    res = {"n": a.n, "dim": a.dim, "metric": "cosine", "filters": a.filters, "density": a.density, "queries": a.queries,
           "k": a.k, "processes": a.processes, "inner": a.inner, "device": last["device"],
           "exact_knn_filtered_voted": summary(sides["voted"]), "exact_knn_filtered_parent": summary(sides["plain"]),
           "identical_results": all(r["identical_results"] for r in sides["voted"]),
           "rows_read_parent": sides["plain"][-1]["rows_read"],
           **{k: last[k] for k in ("rows_read", "rows_read_plain", "n_voted", "n_routed", "pilot_pairs_per_query",
                                   "settled_pairs_per_query", "device_time_split")}}
    res["every_voted_figure_below_parent_min"] = (res["exact_knn_filtered_voted"]["max_s"]
                                                  < res["exact_knn_filtered_parent"]["min_s"])
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_cosine_q{a.queries}_k{a.k}_f{a.filters}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit('exact_knn_filtered(screened="votes") and exact_knn_filtered disagree')


if __name__ == "__main__":
    main()
