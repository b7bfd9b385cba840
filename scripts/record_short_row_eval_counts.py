#!/usr/bin/env python3
"""Records tests/golden/short_row_eval_counts.json: n_evals_prune / n_evals_apply of the short-row builds of
tests/test_gpu_short_row_counts.py, from a library that is NOT the code under test.

    git worktree add /tmp/parent <commit> && (cd /tmp/parent && python -m hannoy_amd.buildlib --out /tmp/parent.so)
    HNY_LIB=/tmp/parent.so python scripts/record_short_row_eval_counts.py --commit <commit>

A second run with a library built with HNY_CFLAGS=-DHNY_PRUNE_FILTER=0 and --filter-off adds, per build, the
prune count without the prefix filter and marks the cases in which it differs (the filter is engaged there):

    HNY_LIB=/tmp/parent_nofilter.so python scripts/record_short_row_eval_counts.py --commit <commit> --filter-off

Needs a GPU.  The counters are integer sums of per-member values: they do not depend on scheduling.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_short_row_counts as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit HNY_LIB was built at")
    ap.add_argument("--filter-off", action="store_true", help="HNY_LIB was built with -DHNY_PRUNE_FILTER=0")
    ap.add_argument("--out", default=T.FIXTURE)
    a = ap.parse_args()
    if not os.environ.get("HNY_LIB"):
        sys.exit("HNY_LIB must name a library built at --commit (python -m hannoy_amd.buildlib --out PATH)")
    import hannoy_amd as H
    from oracle import orc
    H.load_library()
    if a.filter_off:
        with open(a.out) as f:
            doc = json.load(f)
        assert doc["commit"] == a.commit, "the default build was recorded at another commit"
    else:
        doc = {"recorded_by": T.RECORDER, "commit": a.commit, "cases": {}}
    for case in T.CASES:
        metric, n, dim, M, M0, ef = case
        vecs, levels = T.make_inputs(case)
        ds = orc.Dataset.from_f32(metric, vecs, levels)
        items = H.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
        rec = doc["cases"].setdefault(T.case_key(case), {"input_sha1": T.input_sha1(vecs), "schedules": {}})
        assert rec["input_sha1"] == T.input_sha1(vecs)
        for kw in T.SCHEDULES:
            g = H.build(items, M=M, M0=M0, ef_construction=ef, **kw)
            s = rec["schedules"].setdefault(T.schedule_key(kw), {})
            if a.filter_off:
                s["n_evals_prune_filter_off"] = int(g.n_evals_prune)
            else:
                s["n_evals_prune"] = int(g.n_evals_prune)
                s["n_evals_apply"] = int(g.n_evals_apply)
            print(T.case_key(case), T.schedule_key(kw), s, flush=True)
        if a.filter_off:
            rec["filter_engaged"] = any(s["n_evals_prune_filter_off"] != s["n_evals_prune"]
                                        for s in rec["schedules"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
