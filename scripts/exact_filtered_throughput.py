#!/usr/bin/env python3
"""Exact k-NN with a candidates filter per query: hny_builder_exact_knn_filtered_f32 against the loop it replaces.

On ONE builder of n x dim items (loaded on a ring graph: the scan never reads the graph), 1 024 f32 queries and F
distinct filters of about 10 % of the items each (independent Bernoulli samples), queries dealt round-robin, it times
for every F of --filters
  (a) the loop: one Builder.exact_knn_f32(candidates=filter) call per distinct filter on that filter's queries;
  (b) one Builder.exact_knn_filtered_f32 call;
  (c) the same call with HNY_EXACT_SKIP=0 (an all-ones tile mask: every row is read),
checks that (a), (b) and (c) are identical (ids, distance bits, counts) and writes the wall clock of the whole call or
calls, the spread of the repetitions and Builder.exact_rows_read() of (b) and (c) to
profiles/exact_filtered_throughput.json (OUT=path overrides; a run adds its shape to the file it finds).  One
warm-up of each, then --repeat timed repetitions, alternating; medians.  Wall clock only: no counter is read.
Last, on a second builder of the same items in strict mode (x86_order), one unfiltered exact_knn_f32 call of the same
queries, timed alike ("strict_exact_knn_f32"): the path that hands every live item to the one-wave scan.

  python scripts/exact_filtered_throughput.py --n 200000 --dim 768
  python scripts/exact_filtered_throughput.py --n 1000000 --dim 128
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "exact_filtered_throughput.json"


class Ring:
    """every item linked to its two neighbours in id order on layer 0: a valid stored graph at no cost"""

    def __init__(self, np, n):
        ids = np.arange(n, dtype=np.uint32)
        self.rec_item, self.rec_layer = ids, np.zeros(n, np.uint8)
        self.offsets = np.arange(n + 1, dtype=np.uint64) * 2
        self.nbrs = np.sort(np.stack([np.roll(ids, 1), np.roll(ids, -1)], 1), 1).astype(np.uint32).ravel()
        self.entry_points, self.max_level = ids[:1].copy(), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "euclidean", "manhattan"])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--filters", default="1,32,1024", help="numbers of distinct filters")
    ap.add_argument("--fraction", type=float, default=0.1, help="share of the items in every filter")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hannoy_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    metric = ["cosine", "euclidean", "manhattan"].index(a.metric)
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    items = H.F32ItemSet(metric, x)
    row_bytes = (H.vector_bytes(metric, a.dim) + 15) // 16 * 16
    qt = 32
    while qt > 4 and qt * row_bytes > 65536:
        qt //= 2
    ids = np.arange(a.n, dtype=np.uint32)
    size = max(1, int(a.n * a.fraction))
    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "k": a.k, "row_bytes": row_bytes,
           "queries_per_tile": qt, "filter_size_expected": size, "repeat": a.repeat,
           "device": torch.cuda.get_device_name(0),
           "figures": "wall clock of the whole call(s); rows_read is the library's own count, no hardware counter",
           "filters": {}}
    ok = True

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    def stats(ts):
        return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}

    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        for nf in [int(v) for v in a.filters.split(",")]:
            # independent samples: every item is in a filter with probability --fraction
            frng = np.random.default_rng(1000 + nf)
            filters = [ids[frng.random(a.n, dtype=np.float32) < a.fraction] for f in range(nf)]
            fo = np.arange(a.queries) % nf
            groups = [np.flatnonzero(fo == f) for f in range(nf)]
            rows_read = {}

            def loop():
                ids = np.zeros((a.queries, a.k), np.uint32)
                dists = np.zeros((a.queries, a.k), np.float32)
                counts = np.zeros(a.queries, np.uint32)
                for f, rows in enumerate(groups):
                    ids[rows], dists[rows], counts[rows] = b.exact_knn_f32(q[rows], k=a.k, candidates=filters[f])
                return ids, dists, counts

            def one(skip):
                def run():
                    os.environ["HNY_EXACT_SKIP"] = "1" if skip else "0"
                    try:
                        r = b.exact_knn_filtered_f32(q, filters, fo, k=a.k)
                    finally:
                        os.environ.pop("HNY_EXACT_SKIP", None)
                    rows_read[skip] = b.exact_rows_read()
                    return r
                return run

            runs = {"loop": loop, "filtered": one(True), "filtered_skip0": one(False)}
            first = {name: timed(fn)[1] for name, fn in runs.items()}  # the warm-up
            same = all(np.array_equal(g.view(np.uint32), w.view(np.uint32))
                       for name in ("filtered", "filtered_skip0") for g, w in zip(first[name], first["loop"]))
            ok &= same
            ts = {name: [] for name in runs}
            for _ in range(a.repeat):
                for name, fn in runs.items():
                    ts[name].append(timed(fn)[0])
            entry = {name: stats(t) for name, t in ts.items()}
            entry["identical_results"] = bool(same)
            entry["rows_read"] = {"filtered": rows_read[True], "filtered_skip0": rows_read[False],
                                  "tiles_x_n": -(-a.queries // qt) * a.n}
            entry["loop_over_filtered"] = entry["loop"]["median_s"] / entry["filtered"]["median_s"]
            entry["skip0_over_filtered"] = entry["filtered_skip0"]["median_s"] / entry["filtered"]["median_s"]
            if nf == 1:
                entry["exact_knn_f32_single_call"] = entry["loop"]  # the loop IS the one call
            res["filters"][str(nf)] = entry
            print(nf, json.dumps(entry), flush=True)
    # strict mode (x86_order): exact_knn_f32 over every live item goes to the one-wave scan
    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1, x86_order=True) as b:
        ts = [timed(lambda: b.exact_knn_f32(q, k=a.k))[0] for _ in range(1 + a.repeat)][1:]  # the first warms up
        res["strict_exact_knn_f32"] = stats(ts)
        print("strict", json.dumps(res["strict_exact_knn_f32"]), flush=True)
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_{a.metric}_q{a.queries}_k{a.k}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the filtered call and the loop of exact_knn calls disagree")


if __name__ == "__main__":
    main()
