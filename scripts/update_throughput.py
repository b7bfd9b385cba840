#!/usr/bin/env python3
"""What an update costs end to end, through both ways into the incremental build.

For each shape (C2: 1M x 768 Cosine; S: 1M x 128 bits Hamming, a short-row shape) one finished builder, then an
update of 1 000 and of 100 000 items (10 % deletes, 10 % overwrites, the rest new ids),
  (a) through hny_build_incremental on the exported graph with every item uploaded again (today's path), and
  (b) through hny_builder_create_update on the resident builder (+ every batch, fill_gaps, finish / finish_delta).
Per path: state time (hny_graph.t_upload_s: the wall clock of the create call), build time, export time (full; for
(b) also the delta), and for k_move_rows the bytes moved / HIP-event time next to a hipMemcpyAsync device-to-device
copy of the same byte count in the same process.  One warm-up of each path, then --repeat (default 5) repetitions,
alternating (a) and (b); medians and min .. max go to bench_out/update_throughput.json (OUT=path overrides; the
committed copy is under profiles/).  Both graphs are compared once per update: they must be equal.

  python scripts/update_throughput.py [C2 S] [--scale 0.1] [--repeat 5]

Without --one the script is a driver: every shape runs in a child process of its own under `timeout`, and the
first failure stops the run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"C2": ("cosine", 1_000_000, 768, 16, 100), "S": ("hamming", 1_000_000, 128, 16, 64)}
STEP_TIMEOUT_S = {"C2": 900, "S": 600}
NAME = "update_throughput.json"


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def run_one(name, scale, repeat):
    import numpy as np
    import torch
    import hannoy_amd as H
    from bench import gen_data
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: these figures are measurements, not estimates")
    mname, n, dim, M, ef = CFG[name]
    n = max(20000, int(n * scale))
    metric = {"cosine": H.COSINE, "hamming": H.HAMMING}[mname]
    dev = torch.device("cuda", 0)
    big = max(1000, int(100_000 * scale))
    x = gen_data(torch, n + big, dim, "clustered", 42, dev).cpu().numpy()
    torch.cuda.empty_cache()
    codes, headers = H.encode_vectors(metric, x)
    ids0 = np.arange(n, dtype=np.uint32)
    kw = dict(M=M, M0=2 * M, ef_construction=ef, seed=42, device=0)
    items0 = H.ItemSet(metric, dim, ids0, codes[:n], headers[:n])
    L = H.load_library()
    L.hny_internal_builder_move_stats.restype = C.c_int
    L.hny_internal_builder_move_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    res = {"metric": mname, "n": n, "dim": dim, "repeat": repeat, "updates": {}}
    rng = np.random.default_rng(1)
    with H.Builder(items0, **kw) as src:
        src.run()
        g0 = src.finish()
        src.set_profiling(True)  # successors made from it time their k_move_rows
        for size in (max(100, int(1000 * scale)), big):
            n_del, n_over = size // 10, size // 10
            n_new = size - n_del - n_over
            touched = rng.choice(n, n_del + n_over, replace=False)
            to_delete = np.sort(touched[:n_del]).astype(np.uint32)
            over = touched[n_del:]
            to_insert = np.sort(np.concatenate([over, np.arange(n, n + n_new)])).astype(np.uint32)
            src_row = np.where(to_insert < n, (to_insert + 7) % n, to_insert)  # an overwrite takes another item's vector
            uc, uh = codes[src_row], headers[src_row]
            after = np.union1d(np.setdiff1d(ids0, to_delete), to_insert).astype(np.uint32)
            pos = np.searchsorted(to_insert, after)
            is_up = (pos < len(to_insert)) & (to_insert[np.minimum(pos, len(to_insert) - 1)] == after)
            rows_after = np.where(is_up, src_row[np.minimum(pos, len(to_insert) - 1)], after)
            lv = H.draw_levels(7, M, len(to_insert))

            def path_a():
                items = H.ItemSet(metric, dim, after, codes[rows_after], headers[rows_after], lv)
                t0 = time.perf_counter()
                g = H.build_incremental(items, g0, to_insert, to_delete, **kw)
                return g, time.perf_counter() - t0

            def path_b():
                t0 = time.perf_counter()
                with src.create_update(to_insert, codes=uc, headers=uh, delete_ids=to_delete, levels=lv) as s:
                    sec, nb = C.c_double(), C.c_uint64()
                    L.hny_internal_builder_move_stats(s._h, C.byref(sec), C.byref(nb))
                    s.run()
                    g = s.finish()
                    d = s.finish_delta()
                    wall = time.perf_counter() - t0
                    return g, d, wall, sec.value, nb.value

            ga, _ = path_a()
            gb, d, _, _, nbytes = path_b()  # warm-up, and the one comparison
            for f in ("rec_item", "rec_layer", "offsets", "nbrs", "entry_points"):
                assert np.array_equal(getattr(ga, f), getattr(gb, f)), f
            assert ga.n_links_added == gb.n_links_added and ga.n_evals_walk == gb.n_evals_walk
            n_delta, n_total = int(len(d.rec_item)), int(d.n_records_total)
            del ga, gb, d
            # the plain copy k_move_rows is set against: the same byte count (read + write), device to device
            half = max(16, nbytes // 2)
            a_buf = torch.empty(half, dtype=torch.uint8, device=dev)
            b_buf = torch.empty(half, dtype=torch.uint8, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t_copy = []
            for i in range(repeat + 1):
                e0.record()
                b_buf.copy_(a_buf, non_blocking=True)  # hipMemcpyAsync, device to device
                e1.record()
                torch.cuda.synchronize()
                if i:
                    t_copy.append(e0.elapsed_time(e1) * 1e-3)
            del a_buf, b_buf
            torch.cuda.empty_cache()
            A = {k: [] for k in ("state", "build", "export", "wall")}
            B = {k: [] for k in ("state", "build", "export", "export_delta", "wall", "move_rows")}
            for _ in range(repeat):
                g, wall = path_a()
                for k, v in (("state", g.t_upload_s), ("build", g.t_build_s), ("export", g.t_export_s), ("wall", wall)):
                    A[k].append(v)
                del g
                g, d, wall, t_mv, _ = path_b()
                for k, v in (("state", g.t_upload_s), ("build", g.t_build_s), ("export", g.t_export_s),
                             ("export_delta", d.t_export_s), ("wall", wall), ("move_rows", t_mv)):
                    B[k].append(v)
                del g, d
            r = {"n_upsert": int(len(to_insert)), "n_delete": int(len(to_delete)),
                 "a_build_incremental": {k: summary(v) for k, v in A.items()},
                 "b_builder_update": {k: summary(v) for k, v in B.items()},
                 "delta_records": n_delta, "records_total": n_total,
                 "move_rows_bytes": int(nbytes), "d2d_copy": summary(t_copy)}
            r["move_rows_gb_per_s"] = nbytes / r["b_builder_update"]["move_rows"]["median_s"] / 1e9
            r["d2d_copy_gb_per_s"] = nbytes / r["d2d_copy"]["median_s"] / 1e9
            r["state_b_over_a"] = r["b_builder_update"]["state"]["median_s"] / r["a_build_incremental"]["state"]["median_s"]
            res["updates"][str(size)] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=[])
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every shape's items and update sizes (rehearsals)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--one", help="(internal) run this shape in this process and print its JSON")
    a = ap.parse_args()
    if a.repeat < 5:
        raise SystemExit("--repeat: at least 5")
    if a.one:
        print("RESULT " + json.dumps(run_one(a.one, a.scale, a.repeat)), flush=True)
        return
    out_path = os.environ.get("OUT", os.path.join(ROOT, "bench_out", NAME))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    out = {}
    for src in (os.path.join(ROOT, "profiles", NAME), out_path):
        if os.path.exists(src):
            out.update(json.load(open(src)))
    for name in a.configs or list(CFG):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[name]), sys.executable, os.path.abspath(__file__), "--one", name,
               "--scale", str(a.scale), "--repeat", str(a.repeat)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-2000:])
            raise SystemExit(f"{name}: exit status {p.returncode}; stopping here")
        key = name if a.scale == 1.0 else f"{name}@{a.scale}"
        out[key] = json.loads(lines[-1][7:])
        for size, r in out[key]["updates"].items():
            A, B = r["a_build_incremental"], r["b_builder_update"]
            print(f"{key} update {size}: state (a) {A['state']['median_s']:.3f} s (b) {B['state']['median_s']:.3f} s | build (a) "
                  f"{A['build']['median_s']:.3f} (b) {B['build']['median_s']:.3f} | export full (a) {A['export']['median_s']:.3f} "
                  f"(b) {B['export']['median_s']:.3f} delta {B['export_delta']['median_s']:.4f} ({r['delta_records']} of "
                  f"{r['records_total']} records) | k_move_rows {r['move_rows_gb_per_s']:.0f} GB/s, d2d copy "
                  f"{r['d2d_copy_gb_per_s']:.0f} GB/s", flush=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
