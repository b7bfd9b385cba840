#!/usr/bin/env python3
"""Which kernels a build and a search launch, case by case: one tiny build plus one search_knn per case, each in a
child process of its own under `rocprofv3 --kernel-trace --stats`, and per case and kernel (demangled name with template
arguments, k_walk / k_prune / k_apply families) the sorted list of (dispatches, grid size, LDS bytes).

    python scripts/kernel_forms_trace.py OUT.json          # the library of the tree, or the one HNY_LIB names

Two runs - one with HNY_LIB naming a library built at the parent commit (python -m hannoy_amd.buildlib --out PATH),
one with the tree's - must give identical files: the definition of "the same kernels run" for a change of the launch
forms (profiles/kernel_forms_trace_*.json).  Stops at the first child that fails.  No test, no counters.

The LDS column proves nothing: it is the trace's `LDS_Block_Size`, which does not carry the dynamic LDS of a launch, and every
kernel of these families takes all of its LDS dynamically - the column is 0 for every dispatch of both
committed files, k_walk, k_prune_wg, k_prune_n8 and k_apply_wg with their kilobytes included.  What the two files
show equal is the kernel instance, the number of dispatches and the grid.  That the dynamic LDS of a launch is
unchanged rests on the launchers' size expressions (hnyk_walk_lds_bytes, wg_prune_lds_bytes, prune_n8_lds_bytes,
apply_n8_lds_bytes and the two one-wave sums in Hot<SP>), which a change of the launch forms must leave as they are."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (metric, n, dim, M, M0, ef, build keywords, environment, incremental round)
CASES = {
    "euclid_64d": (1, 3000, 64, 16, 32, 100, {}, {}, False),             # n8 prune, two-chunk beam
    "hamming_64b_ef40": (3, 3000, 64, 16, 32, 40, {}, {}, False),        # one-chunk beam, six waves
    "cosine_768d": (0, 3000, 768, 16, 32, 100, {}, {}, False),           # three chunks, workgroup prune
    "cosine_1100d": (0, 2000, 1100, 16, 32, 100, {}, {}, False),         # LDS beam by nch
    "euclid_64d_ef200": (1, 3000, 64, 16, 32, 200, {}, {}, False),       # LDS beam by size
    "cosine_3072d": (0, 1200, 3072, 8, 16, 40, {}, {}, False),           # wave prune
    "euclid_64d_strict": (1, 1500, 64, 16, 32, 100, {"x86_order": True}, {}, False),
    "euclid_64d_incremental": (1, 3000, 64, 16, 32, 100, {}, {}, True),
    "euclid_64d_M0_100": (1, 3000, 64, 16, 100, 100, {}, {}, False),
    "euclid_64d_no_fast": (1, 3000, 64, 16, 32, 100, {}, {"HNY_NO_FAST": "1"}, False),
    "euclid_64d_no_rb": (1, 3000, 64, 16, 32, 100, {}, {"HNY_NO_RB": "1"}, False),
    "hamming_64b_rb_one_0": (3, 3000, 64, 16, 32, 40, {}, {"HNY_RB_ONE": "0"}, False),
    "euclid_64d_prune_n8_0": (1, 3000, 64, 16, 32, 100, {}, {"HNY_PRUNE_N8": "0"}, False),
}
FAMILIES = ("k_walk", "k_prune", "k_apply")


def child(name):
    import numpy as np
    import hannoy_amd as H
    metric, n, dim, M, M0, ef, kw, _, inc = CASES[name]
    rng = np.random.default_rng(17)
    vecs = rng.uniform(-1, 1, (n + 64, dim)).astype(np.float32)
    items = H.F32ItemSet(metric, vecs[:n], levels=H.draw_levels(1, M, n))
    with H.Builder(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.25, batch_max=1024, **kw) as b:
        b.run()
        b.finish()
        if inc:  # one resident update: 64 new items, 16 deleted
            b.update(np.arange(n, n + 64, dtype=np.uint32), vectors=vecs[n:], delete_ids=np.arange(16, dtype=np.uint32),
                     levels=H.draw_levels(2, M, 64))
        qc, qh = H.encode_vectors(metric, vecs[100:164])
        b.search_knn(qc, qh, k=10, ef_search=50)


def trace(name, out_dir):
    env = dict(os.environ, **CASES[name][7])
    cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
           "--", sys.executable, os.path.abspath(__file__), "--child", name]
    rc = subprocess.call(cmd, env=env, stdout=subprocess.DEVNULL)
    if rc != 0:
        sys.exit(f"{name}: exit code {rc}")
    rows = {}
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if not any(fam in k for fam in FAMILIES):
                continue
            grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)
            key = (k, grid, int(r["LDS_Block_Size"]))
            rows[key] = rows.get(key, 0) + 1
    by_kernel = {}
    for (k, grid, lds), cnt in sorted(rows.items()):
        by_kernel.setdefault(k, []).append([cnt, grid, lds])
    return by_kernel


def dump(result, f):
    """one line per kernel: its [dispatches, grid size in threads, LDS bytes] triples, ascending by grid and LDS"""
    f.write('{"columns": ["dispatches", "grid size (threads)", "LDS bytes (LDS_Block_Size: without the dynamic LDS)"],\n'
            ' "cases": {\n')
    for ci, (name, kernels) in enumerate(result.items()):
        f.write(f'  {json.dumps(name)}: {{\n')
        lines = [f"   {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in kernels.items()]
        f.write(",\n".join(lines) + ("\n  }" if ci == len(result) - 1 else "\n  },") + "\n")
    f.write(" }\n}\n")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    out = sys.argv[1]
    result = {}
    for name in CASES:
        d = tempfile.mkdtemp(prefix="forms_trace_")
        try:
            result[name] = trace(name, d)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        print(name, len(result[name]), "kernels", flush=True)
    with open(out, "w") as f:
        dump(result, f)


if __name__ == "__main__":
    main()
