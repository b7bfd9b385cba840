#!/usr/bin/env python3
"""Batched search with one candidates filter per query: hny_builder_nns_filtered_f32 against the loop it replaces.

On ONE finished builder of n x dim items and the same f32 queries, for 1, 32 and 1 024 distinct filters of about
10 % of the items each (queries dealt round-robin to the filters), it times
  (a) the loop of Builder.nns_f32 calls, one per distinct filter on that filter's queries,
  (b) one Builder.nns_filtered_f32 call for the whole batch,
checks that both give identical rows (ids, distance bits, counts) and writes the median wall clock of each and the
ratio (a) / (b) to profiles/filtered_search_throughput.json (OUT=path overrides; a run adds its shape to the file it
finds).  One warm-up of each, then --repeat timed repetitions, alternating.

  python scripts/filtered_search_throughput.py --n 200000 --dim 768
  python scripts/filtered_search_throughput.py --n 1000000 --dim 128
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "filtered_search_throughput.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef-search", type=int, default=100)
    ap.add_argument("--filters", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hannoy_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    ids = np.arange(a.n, dtype=np.uint32)
    kw = dict(k=a.k, ef_search=a.ef_search)
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    failed = False
    with H.Builder(H.F32ItemSet(H.COSINE, x), M=16, M0=32, ef_construction=100) as b:
        b.run()
        b.finish()
        for nf in a.filters:
            filters = [ids[rng.random(a.n) < a.fraction] for _ in range(nf)]
            filter_of = np.arange(a.queries) % nf
            rows = [np.flatnonzero(filter_of == f) for f in range(nf)]
            sub = [np.ascontiguousarray(q[r]) for r in rows]

            def loop():
                got = (np.zeros((a.queries, a.k), np.uint32), np.zeros((a.queries, a.k), np.float32),
                       np.zeros(a.queries, np.uint32))
                for f in range(nf):
                    if len(rows[f]):
                        for dst, src in zip(got, b.nns_f32(sub[f], candidates=filters[f], **kw)):
                            dst[rows[f]] = src
                return got

            def batch():
                return b.nns_filtered_f32(q, filters, filter_of, **kw)

            def timed(fn):
                t0 = time.perf_counter()
                r = fn()
                return time.perf_counter() - t0, r

            _, want = timed(loop)
            _, got = timed(batch)
            identical = all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
            t_loop, t_batch = [], []
            for _ in range(a.repeat):
                t_loop.append(timed(loop)[0])
                t_batch.append(timed(batch)[0])
            sl, sb = statistics.median(t_loop), statistics.median(t_batch)
            res = {
                "n": a.n, "dim": a.dim, "metric": "cosine", "queries": a.queries, "k": a.k, "ef_search": a.ef_search,
                "distinct_filters": nf, "candidates_per_filter": float(np.mean([len(f) for f in filters])),
                "repeat": a.repeat, "identical_results": bool(identical),
                "loop_of_nns_f32": {"median_s": sl, "min_s": min(t_loop), "max_s": max(t_loop),
                                    "queries_per_s": a.queries / sl},
                "nns_filtered_f32": {"median_s": sb, "min_s": min(t_batch), "max_s": max(t_batch),
                                     "queries_per_s": a.queries / sb},
                "ratio_loop_over_batch": sl / sb,
                "device": torch.cuda.get_device_name(0),
            }
            runs = {}
            if os.path.exists(out):
                with open(out) as f:
                    runs = json.load(f)
            runs[f"{a.n}x{a.dim}_cosine_q{a.queries}_k{a.k}_ef{a.ef_search}_f{nf}"] = res
            with open(out, "w") as f:
                json.dump(runs, f, indent=1, sort_keys=True)
            print(json.dumps(res), flush=True)
            failed |= not identical
    if failed:
        raise SystemExit("nns_filtered_f32 and the loop of nns_f32 calls disagree")


if __name__ == "__main__":
    main()
