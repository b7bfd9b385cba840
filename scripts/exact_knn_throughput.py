#!/usr/bin/env python3
"""Exact k-NN throughput: hny_builder_exact_knn against the scan it replaces.

On ONE builder of n x dim items (loaded on a ring graph: neither scan reads the graph) and the same queries it times
  (a) Builder.nns with every id as candidates and linear_below = 2**32 - 1: k_nns_linear, one wave per query, every
      row fetched once per query;
  (b) Builder.exact_knn: k_exact_scores + k_exact_topk, every row fetched once per tile of queries,
checks that the two results are identical (ids, distance bits, counts), and writes queries/s, the row bytes each
traffic model says were read per second, and the ratio (a) / (b) to profiles/exact_knn_throughput.json (OUT=path
overrides; a run adds its shape to the file it finds).  One warm-up of each, then --repeat timed repetitions,
alternating; medians.

  python scripts/exact_knn_throughput.py --n 200000 --dim 768 --metric cosine --queries 1024 --k 10
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "exact_knn_throughput.json"


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
    ap.add_argument("--metric", default="cosine",
                    choices=["cosine", "euclidean", "manhattan", "hamming", "bq-cosine", "bq-euclidean", "bq-manhattan"])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hannoy_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    metric = ["cosine", "euclidean", "manhattan", "hamming", "bq-cosine", "bq-euclidean", "bq-manhattan"].index(a.metric)
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    items = H.F32ItemSet(metric, x)
    ids = np.arange(a.n, dtype=np.uint32)
    row_bytes = (H.vector_bytes(metric, a.dim) + 15) // 16 * 16  # as the builder stores them: 16-byte units
    qt = 32
    while qt > 4 and qt * row_bytes > 65536:
        qt //= 2
    with H.Builder(items, prev=Ring(np, a.n), load=True, M=2, M0=2, ef_construction=1) as b:
        def old():
            return b.nns_f32(q, k=a.k, candidates=ids, linear_below=2 ** 32 - 1)

        def new():
            return b.exact_knn_f32(q, k=a.k)

        def timed(fn):
            t0 = time.perf_counter()
            r = fn()
            return time.perf_counter() - t0, r

        _, want = timed(old)
        _, got = timed(new)
        identical = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
        t_old, t_new = [], []
        for _ in range(a.repeat):
            t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
    so, sn = statistics.median(t_old), statistics.median(t_new)
    pairs = a.queries * a.n
    res = {
        "n": a.n, "dim": a.dim, "metric": a.metric, "queries": a.queries, "k": a.k, "row_bytes": row_bytes,
        "queries_per_tile": qt, "repeat": a.repeat, "identical_results": bool(identical),
        "nns_linear": {"median_s": so, "min_s": min(t_old), "max_s": max(t_old), "queries_per_s": a.queries / so,
                       # model: every query reads every row
                       "model_row_bytes_per_s": pairs * row_bytes / so},
        "exact_knn": {"median_s": sn, "min_s": min(t_new), "max_s": max(t_new), "queries_per_s": a.queries / sn,
                      # model: every tile of queries reads every row once; 8 B of score traffic per pair on top
                      "model_row_bytes_per_s": -(-a.queries // qt) * a.n * row_bytes / sn,
                      "model_score_bytes_per_s": pairs * 8 / sn},
        "ratio_nns_linear_over_exact_knn": so / sn,
        "device": torch.cuda.get_device_name(0),
    }
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
    if not identical:
        raise SystemExit("exact_knn and the nns linear scan disagree")


if __name__ == "__main__":
    main()
