#!/usr/bin/env python3
"""What a change of distance costs between "finished source builder" and "successor ready for its first batch".

C2 size (1M x 768 Cosine), to BQ Cosine (a kept-links pair: the lists move too) and to Euclidean (a fresh graph), in
one process:
  (a) hny_builder_create_changed_distance on the resident builder,
  (b) the host route for the same step: hny_builder_export_items -> hny_encode_vectors -> hny_builder_create
      (Euclidean) / hny_builder_create_incremental on the exported graph (BQ Cosine),
  (c) the re-encode kernel alone (HIP events around the k_ingest launch with the gathered source) next to a
      device-to-device hipMemcpyAsync of the source rows' bytes.
One warm-up of each path, then --repeat (default 5) repetitions, alternating (a) and (b); medians and min .. max go to
bench_out/change_distance_throughput.json (OUT=path overrides; the committed copy is under profiles/).  The rows of the
two successors are compared once per target: export_items must be equal.

  python scripts/change_distance_throughput.py [--scale 0.1] [--repeat 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = "change_distance_throughput.json"


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 1M items (rehearsals)")
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    if a.repeat < 5:
        raise SystemExit("--repeat: at least 5")
    import numpy as np
    import torch
    import hannoy_amd as H
    from bench import gen_data
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: these figures are measurements, not estimates")
    n, dim, M, ef = max(20000, int(1_000_000 * a.scale)), 768, 16, 100
    dev = torch.device("cuda", 0)
    x = gen_data(torch, n, dim, "clustered", 42, dev).cpu().numpy()
    torch.cuda.empty_cache()
    ids = np.arange(n, dtype=np.uint32)
    kw = dict(M=M, M0=2 * M, ef_construction=ef, seed=42, device=0)
    L = H.load_library()
    L.hny_internal_builder_move_stats.restype = C.c_int
    L.hny_internal_builder_move_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    res = {"n": n, "dim": dim, "repeat": a.repeat, "source": "cosine", "targets": {}}
    with H.Builder(H.F32ItemSet(H.COSINE, x, ids), **kw) as src:
        del x
        src.run()
        g0 = src.finish()
        src.set_profiling(True)  # successors made from it time their row kernel
        src_bytes = n * dim * 4
        a_buf = torch.empty(src_bytes, dtype=torch.uint8, device=dev)
        b_buf = torch.empty(src_bytes, dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_copy = []
        for i in range(a.repeat + 1):
            e0.record()
            b_buf.copy_(a_buf, non_blocking=True)  # hipMemcpyAsync, device to device
            e1.record()
            torch.cuda.synchronize()
            if i:
                t_copy.append(e0.elapsed_time(e1) * 1e-3)
        del a_buf, b_buf
        torch.cuda.empty_cache()
        for tname, new in (("bq_cosine", H.BQ_COSINE), ("euclidean", H.EUCLIDEAN)):
            keeps = H.distance_keeps_links(H.COSINE, new)
            lv = H.draw_levels(7, M, n)

            def path_a(keep=False):
                t0 = time.perf_counter()
                s = src.create_changed_distance(new, levels=lv)
                wall = time.perf_counter() - t0
                sec, nb = C.c_double(), C.c_uint64()
                L.hny_internal_builder_move_stats(s._h, C.byref(sec), C.byref(nb))
                out = s.export_items() if keep else None
                s.close()
                return wall, sec.value, nb.value, out

            def path_b(keep=False):
                t0 = time.perf_counter()
                codes, _ = src.export_items()
                t1 = time.perf_counter()
                c, h = H.encode_vectors(new, codes.view(np.float32))
                t2 = time.perf_counter()
                items = H.ItemSet(new, dim, ids, c, h, lv)
                s = H.Builder(items, prev=g0, to_insert=ids, to_delete=[], **kw) if keeps else H.Builder(items, **kw)
                t3 = time.perf_counter()
                out = s.export_items() if keep else None
                s.close()
                return t3 - t0, t1 - t0, t2 - t1, t3 - t2, out

            ra, rb = path_a(True), path_b(True)  # warm-up, and the one comparison
            assert np.array_equal(ra[3][0], rb[4][0]) and np.array_equal(ra[3][1], rb[4][1])
            del ra, rb
            A = {k: [] for k in ("wall", "kernel")}
            B = {k: [] for k in ("wall", "export", "encode", "create")}
            nbytes = 0
            for _ in range(a.repeat):
                wall, sec, nbytes, _o = path_a()
                A["wall"].append(wall)
                A["kernel"].append(sec)
                wall, te, tn, tc, _o = path_b()
                for k, v in (("wall", wall), ("export", te), ("encode", tn), ("create", tc)):
                    B[k].append(v)
            r = {"keeps_links": bool(keeps), "a_resident": {k: summary(v) for k, v in A.items()},
                 "b_host_route": {k: summary(v) for k, v in B.items()}, "kernel_bytes_read_written": int(nbytes),
                 "source_bytes": src_bytes, "d2d_copy_of_source_bytes": summary(t_copy)}
            r["a_over_b"] = r["a_resident"]["wall"]["median_s"] / r["b_host_route"]["wall"]["median_s"]
            r["kernel_over_d2d_copy"] = r["a_resident"]["kernel"]["median_s"] / r["d2d_copy_of_source_bytes"]["median_s"]
            res["targets"][tname] = r
            print(f"{tname}: (a) {r['a_resident']['wall']['median_s']:.3f} s  (b) {r['b_host_route']['wall']['median_s']:.3f} s "
                  f"(export {r['b_host_route']['export']['median_s']:.3f}, encode {r['b_host_route']['encode']['median_s']:.3f}, "
                  f"create {r['b_host_route']['create']['median_s']:.3f}) | kernel {r['a_resident']['kernel']['median_s'] * 1e3:.2f} ms, "
                  f"d2d copy {r['d2d_copy_of_source_bytes']['median_s'] * 1e3:.2f} ms", flush=True)
    out_path = os.environ.get("OUT", os.path.join(ROOT, "bench_out", NAME))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    key = "C2" if a.scale == 1.0 else f"C2@{a.scale}"
    out = {}
    for p in (os.path.join(ROOT, "profiles", NAME), out_path):
        if os.path.exists(p):
            out.update(json.load(open(p)))
    out[key] = res
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
