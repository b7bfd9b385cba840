#!/usr/bin/env python3
"""Manhattan on the bitmap scan: the screened range calls and the voted k-NN of this commit with
Builder.set_l1_screen() against the plain calls of a library built from the parent commit, in alternating processes.

  python scripts/l1_screen_throughput.py --parent-root ../parent --n 1000000 --dim 128
  python scripts/l1_screen_throughput.py --parent-root ../parent --n 200000 --dim 768

--parent-root is a checkout of the parent commit whose library is built (python -m hannoy_amd.buildlib there).  The
driver starts --processes (6) pairs of child processes, one after the other: a child that imports hannoy_amd from the
parent checkout and times the plain calls, then a child that imports this tree's, switches the L1 screen on and times
the same calls with screened=True / screened="votes".  A child encodes n x dim normal f32 rows for Manhattan, loads
them on a ring graph (no call reads the graph) and times, for --queries (1 024) encoded queries: exact_range_count and
exact_range with each query's radius at its 100th distance, and exact_knn for k = 10 and 100.  Every call runs once as
a warm-up, then --inner (3) times; the figure of a process is the median of those.  The driver writes, per call, the
median and min … max of the figures of each side, the certain and settled pairs per query of the count call, the
settled pairs per query of the voted calls and, from one more run on a profiling builder, the device time of scans
and settles (HIP events around every launch on the builder's stream) to profiles/l1_screen_throughput.json (OUT=path
overrides; a run adds itself to the file it finds).  The screened child also runs this tree's plain calls once and
checks that the results are identical.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "l1_screen_throughput.json"
MANHATTAN = 2
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
    metric = MANHATTAN
    rng = np.random.default_rng(42)
    codes, headers = H.encode_vectors(metric, rng.standard_normal((a.n, a.dim), dtype=np.float32), gpu=True)
    qc, qh = H.encode_vectors(metric, rng.standard_normal((a.queries, a.dim), dtype=np.float32))
    items = H.ItemSet(metric, a.dim, np.arange(a.n, dtype=np.uint32), codes, headers, np.zeros(a.n, np.uint8))
    on = a.child == "screened"
    res = {"side": a.child, "device": torch.cuda.get_device_name(0), "seconds": {}}
    same = lambda x, y: all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(x, y))  # noqa: E731
    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        q = dict(qcodes=qc, qheaders=qh)
        radius = b.exact_knn(k=100, **q)[1][:, 99].copy()
        if on:
            b.set_l1_screen()
        calls = {"range_count": lambda **kw: (b.exact_range_count(radius, **q, **kw),),
                 "range": lambda **kw: b.exact_range(radius, **q, **kw),
                 "knn_k10": lambda **kw: b.exact_knn(k=10, **q, **kw),
                 "knn_k100": lambda **kw: b.exact_knn(k=100, **q, **kw)}
        how = lambda name: {} if not on else {"screened": "votes" if name.startswith("knn") else True}  # noqa: E731

        def timed(name):
            t0 = time.perf_counter()
            r = calls[name](**how(name))  # every call ends in a copy of its results to the host
            return time.perf_counter() - t0, r

        got = {name: timed(name)[1] for name in CALLS}
        for name in CALLS:
            res["seconds"][name] = statistics.median(timed(name)[0] for _ in range(a.inner))
        if on:
            res["identical_results"] = all(same(got[name], calls[name]()) for name in CALLS)
            b.set_profiling(True)
            res["pairs_per_query"], res["device_ms"] = {}, {}
            for name in CALLS:
                timed(name)
                if name.startswith("knn"):
                    s = b.exact_vote_stats()
                    res["pairs_per_query"][name] = {"n_voted": s[0], "n_routed": s[1], "pilot": s[2] / max(s[0], 1),
                                                    "settled": s[3] / max(s[0], 1)}
                    res["device_ms"][name] = dict(zip(("pilot", "scans", "settles"), b.exact_vote_times()))
                else:
                    s = b.exact_range_screen_stats()
                    res["pairs_per_query"][name] = {"n_screened": s[0], "n_routed": s[1], "certain": s[2] / max(s[0], 1),
                                                    "settled": s[3] / max(s[0], 1)}
                    res["device_ms"][name] = dict(zip(("scans", "settles"), b.exact_range_screen_times()))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=1024)
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
    shape = ["--n", str(a.n), "--dim", str(a.dim), "--queries", str(a.queries), "--inner", str(a.inner)]
    env = {k: v for k, v in os.environ.items() if k not in ("HNY_LIB", "HNY_VOTE_PILOT_FACTOR", "HNY_VOTE_PILOT_MIN")}
    sides = {"plain": [], "screened": []}
    for _ in range(a.processes):
        for side, root in (("plain", a.parent_root), ("screened", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root] + shape,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            sides[side].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:]))
            print(side, sides[side][-1]["seconds"], flush=True)

    def summary(rs, name):
        t = [r["seconds"][name] for r in rs]
        return {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "per_process_s": t}
    last = sides["screened"][-1]
    res = {"n": a.n, "dim": a.dim, "metric": "manhattan", "queries": a.queries, "processes": a.processes, "inner": a.inner,
           "rows": "normal f32, encoded", "radius": "each query's 100th distance", "device": last["device"],
           "identical_results": all(r["identical_results"] for r in sides["screened"]),
           "pairs_per_query": last["pairs_per_query"], "device_ms": last["device_ms"], "calls": {}}
    for name in CALLS:
        s, p = summary(sides["screened"], name), summary(sides["plain"], name)
        res["calls"][name] = {"l1_screen": s, "parent_plain": p, "ratio_of_medians": p["median_s"] / s["median_s"]}
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_manhattan_q{a.queries}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not res["identical_results"]:
        raise SystemExit("the screened calls and the plain calls disagree")


if __name__ == "__main__":
    main()
