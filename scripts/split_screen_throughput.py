#!/usr/bin/env python3
"""Split-bf16 scan: the screened range calls and the voted k-NN of this commit under
Builder.set_screen_precision("bf16x3") against the same calls of a library built from the parent commit, which run on
the f32 scan, in alternating processes.

  python scripts/split_screen_throughput.py --parent-root ../parent --n 1000000 --dim 128 --metric cosine

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (6) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout, then a child that imports this tree's and switches the split scan on.  A child loads n x dim normal
f32 rows on a ring graph (no call reads the graph) and times, for --queries (1 024) normal queries:
exact_range_count(screened=True) and exact_range(screened=True) with each query's radius at its 100th distance, and
exact_knn(screened="votes") for k = 10 and 100.  Every call runs once as a warm-up, then --inner (3) times; the figure
of a process is the median of those.  The driver writes, per call, the median and min … max of the figures of each
side and, from one more run of each call on a profiling builder (HIP events around every launch on the builder's
stream), the device time of scans and settles and the certain / settled pairs per query — of the split scan and, in
the same process on the same inputs, of this tree's f32 scan — to profiles/split_screen_throughput.json (OUT=path
overrides; a run adds itself to the file it finds).  The split child also checks its results against this tree's
plain calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "split_screen_throughput.json"
METRICS = {"cosine": 0, "euclidean": 1}
CALLS = ("range_count", "range", "knn_k10", "knn_k100")


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
    metric = METRICS[a.metric]
    rng = np.random.default_rng(42)
    codes, headers = H.encode_vectors(metric, rng.standard_normal((a.n, a.dim), dtype=np.float32), gpu=True)
    qc, qh = H.encode_vectors(metric, rng.standard_normal((a.queries, a.dim), dtype=np.float32))
    items = H.ItemSet(metric, a.dim, np.arange(a.n, dtype=np.uint32), codes, headers, np.zeros(a.n, np.uint8))
    split = a.child == "split"
    res = {"side": a.child, "device": torch.cuda.get_device_name(0), "seconds": {}}
    same = lambda x, y: all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(x, y))  # noqa: E731
    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        q = dict(qcodes=qc, qheaders=qh)
        radius = b.exact_knn(k=100, **q)[1][:, 99].copy()
        if split:
            b.set_screen_precision("bf16x3")
        calls = {"range_count": lambda **kw: (b.exact_range_count(radius, **q, **kw),),
                 "range": lambda **kw: b.exact_range(radius, **q, **kw),
                 "knn_k10": lambda **kw: b.exact_knn(k=10, **q, **kw),
                 "knn_k100": lambda **kw: b.exact_knn(k=100, **q, **kw)}
        how = lambda name: {"screened": "votes" if name.startswith("knn") else True}  # noqa: E731

        def timed(name):
            t0 = time.perf_counter()
            r = calls[name](**how(name))  # every call ends in a copy of its results to the host
            return time.perf_counter() - t0, r

        def profiled():
            pairs, ms = {}, {}
            for name in CALLS:
                timed(name)
                if name.startswith("knn"):
                    s = b.exact_vote_stats()
                    pairs[name] = {"n_voted": s[0], "n_routed": s[1], "pilot": s[2] / max(s[0], 1), "settled": s[3] / max(s[0], 1)}
                    ms[name] = dict(zip(("pilot", "scans", "settles"), b.exact_vote_times()))
                else:
                    s = b.exact_range_screen_stats()
                    pairs[name] = {"n_screened": s[0], "n_routed": s[1], "certain": s[2] / max(s[0], 1), "settled": s[3] / max(s[0], 1)}
                    ms[name] = dict(zip(("scans", "settles"), b.exact_range_screen_times()))
            return pairs, ms

        got = {name: timed(name)[1] for name in CALLS}
        for name in CALLS:
            res["seconds"][name] = statistics.median(timed(name)[0] for _ in range(a.inner))
        b.set_profiling(True)
        res["pairs_per_query"], res["device_ms"] = profiled()
        if split:
            res["identical_results"] = all(same(got[name], calls[name]()) for name in CALLS)
            b.set_screen_precision("f32")
            res["f32_pairs_per_query"], res["f32_device_ms"] = profiled()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="cosine", choices=sorted(METRICS))
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--processes", type=int, default=6)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--parent-root")
    ap.add_argument("--child", choices=["parent", "split"])
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root:
        raise SystemExit("--parent-root: a checkout of the parent commit with its library built")
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--metric", a.metric, "--queries", str(a.queries), "--inner", str(a.inner)]
    env = {k: v for k, v in os.environ.items() if k not in ("HNY_LIB", "HNY_VOTE_PILOT_FACTOR", "HNY_VOTE_PILOT_MIN")}
    sides = {"parent": [], "split": []}
    for _ in range(a.processes):
        for side, root in (("parent", a.parent_root), ("split", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))
            print(side, sides[side][-1]["seconds"], flush=True)

    def summary(rs, name):
        t = [r["seconds"][name] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last, plast = sides["split"][-1], sides["parent"][-1]
    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "processes": a.processes, "inner": a.inner,
           "rows": "normal f32", "radius": "each query's 100th distance", "device": last["device"],
           "identical_results": all(r["identical_results"] for r in sides["split"]),
           "pairs_per_query": {"bf16x3": last["pairs_per_query"], "f32_same_process": last["f32_pairs_per_query"]},
           "device_ms": {"bf16x3": last["device_ms"], "f32_same_process": last["f32_device_ms"],
                         "f32_parent": plast["device_ms"]}, "calls": {}}
    for name in CALLS:
        s, p = summary(sides["split"], name), summary(sides["parent"], name)
        res["calls"][name] = {"bf16x3": s, "parent_f32": p, "ratio_of_medians": p["median_s"] / s["median_s"],
                              "split_max_below_parent_min": s["max_s"] < p["min_s"]}
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_{a.metric}_q{a.queries}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit("the split-scan calls and the plain calls disagree")


if __name__ == "__main__":
    main()
