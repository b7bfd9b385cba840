#!/usr/bin/env python3
"""Filters as bitsets over item ids against the same filters as id lists.

On ONE finished builder of n x dim cosine items (ids 0 .. n-1) and the same 1 024 f32 queries, for F distinct filters
(queries dealt round-robin) of every density of --fractions, it times four calls on the same sets:
  hny_builder_nns_filtered_f32        and  hny_builder_nns_bitsets_f32,
  hny_builder_exact_knn_filtered_f32  and  hny_builder_exact_knn_bitsets_f32.
The id-list calls are the baseline: code that the bitset source does not touch.  Both forms are packed into their C
structs once, outside the timed region (concatenating 10^8 ids in numpy is not the library's time), so a figure is the
wall clock of the C call through ctypes plus the result arrays.  One warm-up of each, then --repeat repetitions,
alternating; median (min .. max).  Each pair is checked to be identical (ids, distance bits, counts, rows_read).
`upload_bytes` is what each form sends to the device for its filters per call: 4 B per live candidate and 8 B per
filter, or ceil(n_bits / 32) words per used filter.  Host and device time are not split: that would take tracing.

Writes profiles/bitset_filter_throughput.json (OUT=path overrides; a run adds its shape to the file it finds).

  python scripts/bitset_filter_throughput.py --n 200000 --dim 768
  python scripts/bitset_filter_throughput.py --n 1000000 --dim 128
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "bitset_filter_throughput.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef-search", type=int, default=100)
    ap.add_argument("--filters", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.5])
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hannoy_amd as H
    from hannoy_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    rng = np.random.default_rng(42)
    x = rng.standard_normal((a.n, a.dim), dtype=np.float32)
    q = rng.standard_normal((a.queries, a.dim), dtype=np.float32)
    out = os.environ.get("OUT") or os.path.join(ROOT, "profiles", NAME)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    failed = False

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    def stats(ts):
        return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}

    with H.Builder(H.F32ItemSet(H.COSINE, x), M=16, M0=32, ef_construction=100) as b:
        b.run()
        b.finish()
        src = _capi._query_source(None, _capi._f32_rows(q), None, None)
        for frac in a.fractions:
            for nf in a.filters:
                frng = np.random.default_rng(1000 * nf + int(frac * 100))
                mask = np.zeros((nf, (a.n + 31) // 32 * 32), bool)
                for f in range(nf):
                    mask[f, :a.n] = frng.random(a.n, dtype=np.float32) < frac
                bits = np.ascontiguousarray(np.packbits(mask, axis=1, bitorder="little").view("<u4"))
                lists = [np.flatnonzero(row).astype(np.uint32) for row in mask]
                del mask
                fo = np.arange(a.queries) % nf
                used = min(nf, a.queries)
                as_lists = _capi.QueryFilters.pack(lists, fo)
                as_bits = _capi.QueryBitsets.pack(bits, a.n, fo)
                n_ids = int(sum(len(s) for s in lists[:used]))
                rows_read = {}

                def call(name, packed, exact):
                    def run():
                        opts = _capi._query_opts(a.k, cancel=None) if exact else \
                            _capi._query_opts(a.k, a.ef_search, 1000, 1.0, cancel=None)
                        r = b._search(name, opts, src, True, packed)
                        rows_read[name] = b.exact_rows_read()
                        return r
                    return run
                runs = {"nns_filtered_f32": call("hny_builder_nns_filtered", as_lists, False),
                        "nns_bitsets_f32": call("hny_builder_nns_bitsets", as_bits, False),
                        "exact_knn_filtered_f32": call("hny_builder_exact_knn_filtered", as_lists, True),
                        "exact_knn_bitsets_f32": call("hny_builder_exact_knn_bitsets", as_bits, True)}
                first = {name: timed(fn)[1] for name, fn in runs.items()}  # the warm-up
                same = True
                for kind in ("nns", "exact_knn"):
                    same &= all(np.array_equal(g.view(np.uint32), w.view(np.uint32))
                                for g, w in zip(first[kind + "_bitsets_f32"], first[kind + "_filtered_f32"]))
                same &= rows_read["hny_builder_exact_knn_filtered"] == rows_read["hny_builder_exact_knn_bitsets"]
                ts = {name: [] for name in runs}
                for _ in range(a.repeat):
                    for name, fn in runs.items():
                        ts[name].append(timed(fn)[0])
                res = {"n": a.n, "dim": a.dim, "metric": "cosine", "queries": a.queries, "k": a.k,
                       "ef_search": a.ef_search, "distinct_filters": nf, "fraction": frac,
                       "candidates_per_filter": n_ids / used, "repeat": a.repeat, "identical_results": bool(same),
                       "upload_bytes": {"id_lists": 4 * n_ids + 8 * (used + 1), "bitsets": used * ((a.n + 31) // 32) * 4},
                       "device": torch.cuda.get_device_name(0)}
                for name, t in ts.items():
                    res[name] = stats(t)
                res["nns_lists_over_bitsets"] = res["nns_filtered_f32"]["median_s"] / res["nns_bitsets_f32"]["median_s"]
                res["exact_lists_over_bitsets"] = (res["exact_knn_filtered_f32"]["median_s"] /
                                                   res["exact_knn_bitsets_f32"]["median_s"])
                runs_file = {}
                if os.path.exists(out):
                    with open(out) as f:
                        runs_file = json.load(f)
                runs_file[f"{a.n}x{a.dim}_cosine_q{a.queries}_k{a.k}_ef{a.ef_search}_f{nf}_d{int(frac * 100)}"] = res
                with open(out, "w") as f:
                    json.dump(runs_file, f, indent=1, sort_keys=True)
                print(json.dumps(res), flush=True)
                failed |= not same
    if failed:
        raise SystemExit("the bitset calls and the id-list calls disagree")


if __name__ == "__main__":
    main()
