#!/usr/bin/env python3
"""Exact range search throughput: hny_builder_exact_range_count and hny_builder_exact_range against
hny_builder_exact_knn(k = 10) of the same build, the yardstick (one dense scan plus a top-k merge).

On ONE builder of n x dim items (loaded on a ring graph: the scan never reads the graph) and the same f32 queries, for
radii that hold about 10, about 1 000 and about 50 000 hits per query, it times Builder.exact_range_count_f32,
Builder.exact_range_f32 and Builder.exact_knn_f32(k = 10), checks that every repetition of a call returns the same
bytes and that the counts are the full call's row sizes, and writes seconds, queries/s, hits and the ratios to the
yardstick to profiles/exact_range_throughput.json (OUT=path overrides; a run adds its shape to the file it finds).
The radii are per query: the 10th and 1 000th distance of exact_knn(k = 1 000), and for 50 000 hits the matching
quantile of the query's distances to a sample of 4 000 items (exact_knn over the sample as candidates).
One warm-up of each call, then --repeat timed repetitions, alternating; medians.

Traffic model (an expectation, not a requirement): the count call is about one scan, the full call about two scans
plus the sort and the transfer of the hits.

  python scripts/exact_range_throughput.py --n 200000 --dim 768
  python scripts/exact_range_throughput.py --n 1000000 --dim 128
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "exact_range_throughput.json"
SAMPLE = 4000


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
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--hits", type=int, nargs="+", default=[10, 1000, 50000])
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
    sample = np.sort(rng.choice(a.n, min(SAMPLE, a.n), replace=False)).astype(np.uint32)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    def same(x, y):
        x, y = (x if isinstance(x, tuple) else (x,)), (y if isinstance(y, tuple) else (y,))
        return all(u.tobytes() == v.tobytes() for u, v in zip(x, y))

    res = {"n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "repeat": a.repeat,
           "device": torch.cuda.get_device_name(0), "radii": {}}
    ok = True
    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        near = b.exact_knn_f32(q, k=1000)[1]
        far = b.exact_knn_f32(q, k=len(sample), candidates=sample)[1]

        def knn():
            return b.exact_knn_f32(q, k=10)

        for hits in a.hits:
            if hits <= 1000:
                radius = near[:, hits - 1].copy()
            else:
                radius = far[:, min(len(sample) - 1, round(hits * len(sample) / a.n))].copy()

            def count():
                return b.exact_range_count_f32(q, radius)

            def full():
                return b.exact_range_f32(q, radius)

            calls = {"exact_knn_k10": knn, "exact_range_count": count, "exact_range": full}
            first = {name: timed(fn)[1] for name, fn in calls.items()}  # warm-up
            times = {name: [] for name in calls}
            identical = True
            for _ in range(a.repeat):
                for name, fn in calls.items():
                    t, r = timed(fn)
                    times[name].append(t)
                    identical = identical and same(r, first[name])
            sizes = np.diff(first["exact_range"][0])
            identical = identical and np.array_equal(sizes, first["exact_range_count"])
            ok = ok and identical
            med = {name: statistics.median(t) for name, t in times.items()}
            entry = {"wanted_hits_per_query": hits, "hits_per_query_mean": float(sizes.mean()),
                     "hits_per_query_min": int(sizes.min()), "hits_per_query_max": int(sizes.max()),
                     "hits_total": int(sizes.sum()), "identical_results": bool(identical)}
            for name, t in times.items():
                entry[name] = {"median_s": med[name], "min_s": min(t), "max_s": max(t),
                               "queries_per_s": a.queries / med[name]}
            entry["ratio_count_over_exact_knn"] = med["exact_range_count"] / med["exact_knn_k10"]
            entry["ratio_range_over_exact_knn"] = med["exact_range"] / med["exact_knn_k10"]
            res["radii"][f"about_{hits}"] = entry
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    runs[f"{a.n}x{a.dim}_{a.metric}_q{a.queries}"] = res
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    if not ok:
        raise SystemExit("repetitions of a call differ, or the counts are not the full call's row sizes")


if __name__ == "__main__":
    main()
