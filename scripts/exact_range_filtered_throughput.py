#!/usr/bin/env python3
"""Exact range search with a filter per query: hny_builder_exact_range_bitsets / _count_bitsets in one call against
the loop of one hny_builder_exact_range / _count call per distinct filter, the only way before these calls existed.

On ONE builder of n x dim items (loaded on a ring graph: the scan never reads the graph) and 1 024 f32 queries, for
filter densities 0.1 %, 10 % and 50 % and 1, 32 and 1 024 distinct filters (query i uses filter i % F), with a radius
per query of about 100 hits under its filter (a quantile of its distances to a sample of 4 000 items), it times

  --role branch   the single call, counts and hits (Builder.exact_range_count_bitsets_f32 / exact_range_bitsets_f32),
                  and the unfiltered Builder.exact_range_f32 / exact_range_count_f32 at the radius of the 10 % cells
  --role parent   the loop of Builder.exact_range_f32 / exact_range_count_f32 calls, one per distinct filter on its own
                  queries with candidates = the filter's ids (made from the bitset outside the timed region), and the
                  same unfiltered calls.  Run it from a checkout of the parent commit with its own build of the
                  library (this file copied into its scripts/: the binding of this commit does not load a library
                  without the new symbols), OUT naming the same JSON.

Both roles write into profiles/exact_range_filtered_throughput.json (OUT=path overrides) under the shape's key; the
role that finds the other's figures adds the comparison: the single call's median against the loop's minimum, and
the unfiltered medians of one against the min .. max spread of the other.  One warm-up, then --repeat timed
repetitions; median, min and max per cell.  The F filters of a cell are 32 drawn bitsets and their rotations by whole
words, which keeps the density.  Keys of the file that are no shape (`resource_usage`: the kernels' registers from
the compiler's remarks) are kept as they are.

  OUT=$PWD/profiles/exact_range_filtered_throughput.json python ../parent/scripts/exact_range_filtered_throughput.py \
      --role parent --n 200000 --dim 768
  python scripts/exact_range_filtered_throughput.py --role branch --n 200000 --dim 768
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "exact_range_filtered_throughput.json"
SAMPLE, HITS, DRAWN = 4000, 100, 32


class Ring:
    """every item linked to its two neighbours in id order on layer 0: a valid stored graph at no cost"""

    def __init__(self, np, n):
        ids = np.arange(n, dtype=np.uint32)
        self.rec_item, self.rec_layer = ids, np.zeros(n, np.uint8)
        self.offsets = np.arange(n + 1, dtype=np.uint64) * 2
        self.nbrs = np.sort(np.stack([np.roll(ids, 1), np.roll(ids, -1)], 1), 1).astype(np.uint32).ravel()
        self.entry_points, self.max_level = ids[:1].copy(), 0


def stats(times, nq):
    med = statistics.median(times)
    return {"median_s": med, "min_s": min(times), "max_s": max(times), "queries_per_s": nq / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", required=True, choices=["branch", "parent"])
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.001, 0.1, 0.5])
    ap.add_argument("--filters", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--unfiltered-only", action="store_true",
                    help="time the unfiltered calls alone and add the run to the shape's unfiltered_alternating list of "
                         "the role: for runs of the two libraries in turn, whose spread includes process to process")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hannoy_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    n, nq = a.n, a.queries
    assert n % 32 == 0
    rng = np.random.default_rng(42)
    x = rng.standard_normal((n, a.dim), dtype=np.float32)
    q = rng.standard_normal((nq, a.dim), dtype=np.float32)
    items = H.F32ItemSet(0, x)  # cosine
    sample = np.sort(rng.choice(n, min(SAMPLE, n), replace=False)).astype(np.uint32)
    res = {"n": n, "dim": a.dim, "metric": "cosine", "queries": nq, "repeat": a.repeat,
           "device": torch.cuda.get_device_name(0), "library": "HNY_LIB" if os.environ.get("HNY_LIB") else "the tree's own",
           "cells": {}}

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    with H.Builder(items, prev=Ring(np, n), load=True, M=2, M0=2, ef_construction=1) as b:
        far = b.exact_knn_f32(q, k=len(sample), candidates=sample)[1]

        def radius_for(density):
            rank = min(len(sample) - 1, max(1, round(HITS / (density * n) * len(sample))))
            return far[:, rank].copy()

        # the unchanged path: the unfiltered calls at the radius of the 10 % cells
        r10 = radius_for(0.1)
        calls = {"exact_range": lambda: b.exact_range_f32(q, r10), "exact_range_count": lambda: b.exact_range_count_f32(q, r10)}
        times = {k: [] for k in calls}
        for rep in range(a.repeat + 1):
            for k, fn in calls.items():
                t, r = timed(fn)
                if rep:
                    times[k].append(t)
        res["unfiltered"] = {k: stats(t, nq) for k, t in times.items()}
        res["unfiltered"]["hits_per_query_mean"] = float(b.exact_range_count_f32(q, r10).mean())

        for density in ([] if a.unfiltered_only else a.densities):
            drawn = np.stack([np.packbits(rng.random(n, dtype=np.float32) < density, bitorder="little").view("<u4")
                              for _ in range(DRAWN)])
            radius = radius_for(density)
            for F in a.filters:
                bits = np.stack([np.roll(drawn[f % DRAWN], 64 * (f // DRAWN)) for f in range(F)])
                fo = np.arange(nq) % F
                cell = {"density": density, "distinct_filters": F}
                if a.role == "branch":
                    calls = {"single_count": lambda: b.exact_range_count_bitsets_f32(q, radius, bits, n, fo),
                             "single_hits": lambda: b.exact_range_bitsets_f32(q, radius, bits, n, fo)}
                    times, first = {k: [] for k in calls}, {}
                    for rep in range(a.repeat + 1):
                        for k, fn in calls.items():
                            t, r = timed(fn)
                            if rep:
                                times[k].append(t)
                                same = all(u.tobytes() == v.tobytes() for u, v in zip(r, first[k])) \
                                    if isinstance(r, tuple) else r.tobytes() == first[k].tobytes()
                                if not same:
                                    raise SystemExit(f"{k}: repetitions differ")
                            else:
                                first[k] = r
                    cell["rows_read_both_passes"] = b.exact_rows_read()  # (the hits call ran last)
                    sizes = np.diff(first["single_hits"][0])
                    if not np.array_equal(sizes, first["single_count"]):
                        raise SystemExit("the counts are not the full call's row sizes")
                else:
                    groups = [np.flatnonzero(fo == f) for f in range(F)]
                    qg = [np.ascontiguousarray(q[g]) for g in groups]
                    times = {"loop_count": [], "loop_hits": []}
                    sizes = np.zeros(nq, np.int64)
                    for rep in range(a.repeat + 1):
                        tc = th = 0.0
                        for f, g in enumerate(groups):
                            ids = np.flatnonzero(np.unpackbits(bits[f].view(np.uint8), bitorder="little")).astype(np.uint32)
                            t, cnt = timed(lambda: b.exact_range_count_f32(qg[f], radius[g], candidates=ids))
                            tc += t
                            t, full = timed(lambda: b.exact_range_f32(qg[f], radius[g], candidates=ids))
                            th += t
                            sizes[g] = cnt
                            if not np.array_equal(np.diff(full[0]), cnt):
                                raise SystemExit("the counts are not the full call's row sizes")
                        if rep:
                            times["loop_count"].append(tc)
                            times["loop_hits"].append(th)
                cell.update({k: stats(t, nq) for k, t in times.items()})
                cell.update({"hits_per_query_mean": float(sizes.mean()), "hits_total": int(sizes.sum())})
                res["cells"][f"density_{density:g}_filters_{F}"] = cell
                print(json.dumps({f"density_{density:g}_filters_{F}": cell}), flush=True)

    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {}
    if os.path.exists(out):
        with open(out) as f:
            runs = json.load(f)
    shape = runs.setdefault(f"{n}x{a.dim}_cosine_q{nq}", {})
    if a.unfiltered_only:
        alt = shape.setdefault("unfiltered_alternating", {})
        alt.setdefault(a.role, []).append(res["unfiltered"])
        if "branch" in alt and "parent" in alt:
            alt["branch_medians_inside_parent_runs"] = {
                k: {"parent_min_s": min(r[k]["min_s"] for r in alt["parent"]),
                    "parent_max_s": max(r[k]["max_s"] for r in alt["parent"]),
                    "branch_medians_s": [r[k]["median_s"] for r in alt["branch"]],
                    "inside": all(min(p[k]["min_s"] for p in alt["parent"]) <= r[k]["median_s"] <=
                                  max(p[k]["max_s"] for p in alt["parent"]) for r in alt["branch"])}
                for k in ("exact_range", "exact_range_count")}
        with open(out, "w") as f:
            json.dump(runs, f, indent=1, sort_keys=True)
        print(json.dumps(res["unfiltered"]))
        return
    shape[a.role] = res
    if "branch" in shape and "parent" in shape:
        br, pa = shape["branch"], shape["parent"]
        cmp = {}
        for key, cell in br["cells"].items():
            if key not in pa["cells"]:
                continue
            p = pa["cells"][key]
            if cell["hits_total"] != p["hits_total"]:
                raise SystemExit(f"{key}: the single call found {cell['hits_total']} hits, the loop {p['hits_total']}")
            cmp[key] = {what: {"single_median_s": cell[f"single_{what}"]["median_s"],
                               "loop_min_s": p[f"loop_{what}"]["min_s"], "loop_median_s": p[f"loop_{what}"]["median_s"],
                               "single_median_below_loop_min": cell[f"single_{what}"]["median_s"] < p[f"loop_{what}"]["min_s"],
                               "loop_median_over_single_median": p[f"loop_{what}"]["median_s"] / cell[f"single_{what}"]["median_s"]}
                        for what in ("count", "hits")}
        shape["single_call_against_loop"] = cmp
        shape["unfiltered_branch_against_parent"] = {
            k: {"branch_median_s": br["unfiltered"][k]["median_s"], "parent_min_s": pa["unfiltered"][k]["min_s"],
                "parent_max_s": pa["unfiltered"][k]["max_s"],
                "inside_parent_spread": pa["unfiltered"][k]["min_s"] <= br["unfiltered"][k]["median_s"] <= pa["unfiltered"][k]["max_s"]}
            for k in ("exact_range", "exact_range_count")}
    with open(out, "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
