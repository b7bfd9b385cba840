"""Two-stage search: recall@10 and wall clock of hny_builder_nns_rescored.

Per dataset (200 000 x 768 and 1M x 128 Cosine, embedding-like synthetic rows, the BQ-Cosine successor made by create_changed_distance), 1 024 f32
queries, k = 10, n_rescore in {50, 200, 1 000}: recall against exact_knn on the f32 builder for the BQ index alone, the
rescored search and the f32 graph itself; the time of the fused call, and of the two-call route (nns on the BQ builder,
exact_knn_filtered on the f32 builder with one filter per query).  The two-call route exists on the parent commit
too: `--tree PATH` imports hannoy_amd from that (built) checkout, so that alternating processes on both give the
medians with their min ... max.  One JSON line per process; `--out FILE` appends it; `--aggregate FILE...` folds
such lines into the profile (per config, route and n_rescore: the median of the processes' medians, min ... max of
all their runs).

    python scripts/rescore_throughput.py --config 768 --route fused --commit THIS --out runs.jsonl
    python scripts/rescore_throughput.py --config 768 --route two-call --tree ../parent --commit PARENT --out runs.jsonl
    python scripts/rescore_throughput.py --aggregate runs.jsonl > profiles/rescore_throughput.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"768": (200_000, 768), "128": (1_000_000, 128)}
NQ, K, R_VALUES, EF = 1024, 10, (50, 200, 1000), 100


def recall(ids, counts, exact_ids):
    hit = sum(len(np.intersect1d(ids[i, :counts[i]], exact_ids[i])) for i in range(len(ids)))
    return hit / exact_ids.size


def data(n, dim, seed=7):
    """embedding-like rows and held-out queries of the same distribution (bench.py's `overlap`): 1 024 overlapping
    clusters on a 32-d manifold (latent centres N(0, 1), points centre + 0.5 N(0, 1)) embedded in `dim` dimensions,
    plus 0.05 isotropic noise"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((1024, 32), dtype=np.float32)
    basis = np.linalg.qr(rng.standard_normal((dim, 32)))[0].T.astype(np.float32)

    def draw(m):
        z = centres[rng.integers(0, 1024, m)] + 0.5 * rng.standard_normal((m, 32), dtype=np.float32)
        return z @ basis + 0.05 * rng.standard_normal((m, dim), dtype=np.float32)
    return draw(n), draw(NQ)


def timed(fn, repeat):
    out, ts = None, []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_s": float(np.median(ts)), "min_s": min(ts), "max_s": max(ts), "n": repeat}


def aggregate(files):
    runs = [json.loads(line) for f in files for line in open(f) if line.strip()]
    out = {"what": __doc__.split("\n\n")[0], "nq": NQ, "k": K, "configs": {}}
    for cfg in sorted({r["config"] for r in runs}):
        mine = [r for r in runs if r["config"] == cfg]
        c = {"n": mine[0]["n"], "dim": mine[0]["dim"], "ef_search": "max(%d, n_rescore)" % EF, "processes": len(mine),
             "recall_f32_graph": mine[0]["recall_f32_graph"], "recall_bq_alone": mine[0]["recall_bq_alone"], "points": []}
        for R in R_VALUES:
            pt = {"n_rescore": R}
            for route in ("fused", "two_call"):
                got = [(r["commit"], p) for r in mine for p in r["points"] if p["n_rescore"] == R and route in p]
                if got:
                    pt[route] = {"commit": sorted({g[0] for g in got}), "processes": len(got),
                                 "median_s": float(np.median([p[route]["median_s"] for _, p in got])),
                                 "min_s": min(p[route]["min_s"] for _, p in got),
                                 "max_s": max(p[route]["max_s"] for _, p in got)}
                    key = "recall_rescored" if route == "fused" else "recall_two_call"
                    pt[key] = got[0][1][key]
            c["points"].append(pt)
        out["configs"][cfg] = c
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="768")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--route", choices=["fused", "two-call", "both"], default="both")
    ap.add_argument("--tree", default=ROOT, help="the checkout hannoy_amd is imported from, e.g. the parent commit's")
    ap.add_argument("--commit", default="", help="the commit of that checkout's library, for the record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--aggregate", nargs="+", default=None)
    a = ap.parse_args()
    if a.aggregate:
        return aggregate(a.aggregate)
    sys.path.insert(0, os.path.abspath(a.tree))
    import hannoy_amd as H
    n, dim = CONFIGS[a.config]
    V, Q = data(n, dim)
    fine = H.Builder(H.F32ItemSet(H.COSINE, V), M=16, M0=32, ef_construction=100)
    fine.run()
    fine.finish()
    coarse = fine.create_changed_distance(H.BQ_COSINE)
    coarse.run()
    coarse.finish()
    exact = fine.exact_knn_f32(Q, k=K)[0]
    res = {"config": a.config, "n": n, "dim": dim, "nq": NQ, "k": K, "ef_search": EF, "commit": a.commit,
           "version": H.load_library().hny_version().decode(), "points": []}
    ids, _, c = fine.nns_f32(Q, k=K, ef_search=EF)
    res["recall_f32_graph"] = recall(ids, c, exact)
    ids, _, c = coarse.nns_f32(Q, k=K, ef_search=EF)
    res["recall_bq_alone"] = recall(ids, c, exact)
    for R in R_VALUES:
        pt = {"n_rescore": R}
        if a.route in ("fused", "both") and hasattr(coarse, "nns_rescored"):
            got, pt["fused"] = timed(lambda: coarse.nns_rescored(fine, qf32=Q, k=K, n_rescore=R, ef_search=max(EF, R)),
                                     a.repeat)
            pt["recall_rescored"] = recall(got[0], got[2], exact)
        if a.route in ("two-call", "both"):
            def two_calls():
                i1, _, c1 = coarse.nns_f32(Q, k=R, ef_search=max(EF, R))
                return fine.exact_knn_filtered_f32(Q, [i1[i, :c1[i]] for i in range(NQ)], np.arange(NQ), k=K)
            got, pt["two_call"] = timed(two_calls, a.repeat)
            pt["recall_two_call"] = recall(got[0], got[2], exact)
        res["points"].append(pt)
    coarse.close()
    fine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
