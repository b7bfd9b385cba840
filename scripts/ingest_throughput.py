#!/usr/bin/env python3
"""Ingest throughput: how fast f32 vectors become a resident, encoded builder.

For each config (C2 1M x 768 Cosine, C4 10M x 128 Cosine, C5 5M x 1024 bits Hamming from f32) it times, in ONE
process and on the same data,
  (a) a plain host-to-device copy of the f32 matrix from pinned memory: the ceiling (a pinned sample of at most
      --pinned-gib GiB of the matrix, copied as often as the matrix is long);
  (b) the two-call route: hny_encode_vectors_gpu followed by hny_builder_create on its output;
  (c) hny_builder_create_f32.
One warm-up, then --repeat (default 5) timed repetitions of each, alternating (b) and (c); the median and the
min .. max spread go to bench_out/ingest_throughput.json (OUT=path overrides; the committed copy is under profiles/,
and a run of some configs starts from it) as GB/s of f32 in, (c) as a fraction of (a), and the upload time of (b) and (c): the wall clock of the create
call, which is what hny_graph.t_upload_s records.

  python scripts/ingest_throughput.py [C2 C4 C5] [--scale 0.01] [--repeat 5]

Without --one the script is a driver: every config runs in a child process of its own under `timeout`, and the
first failure stops the run (nothing else is started on a GPU that may have faulted).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"C2": ("cosine", 1_000_000, 768, 16, 100), "C4": ("cosine", 10_000_000, 128, 16, 100),
       "C5": ("hamming", 5_000_000, 1024, 16, 64)}
STEP_TIMEOUT_S = {"C2": 300, "C4": 420, "C5": 480}
NAME = "ingest_throughput.json"


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def run_one(name, scale, repeat, pinned_gib):
    import numpy as np
    import torch
    import hannoy_amd as H
    from bench import gen_data
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a throughput figure is a measurement, not an estimate")
    mname, n, dim, M, ef = CFG[name]
    n = max(1000, int(n * scale))
    metric = {"cosine": H.COSINE, "hamming": H.HAMMING}[mname]
    dev = torch.device("cuda", 0)
    x = gen_data(torch, n, dim, "overlap" if name in ("C4", "C5") else "clustered", 42, dev).cpu().numpy()
    torch.cuda.empty_cache()
    nbytes = x.nbytes
    kw = dict(M=M, M0=2 * M, ef_construction=ef, seed=42)

    # (a) the ceiling
    rows = max(1, min(n, int(pinned_gib * 2 ** 30) // (dim * 4)))
    pinned = torch.from_numpy(x[:rows]).pin_memory()
    dst = torch.empty_like(pinned, device=dev)
    reps = -(-n // rows)

    def ceiling():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            dst.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * (n / (reps * rows))

    def two_calls():
        t0 = time.perf_counter()
        codes, headers = H.encode_vectors(metric, x, gpu=True, device=0)
        t1 = time.perf_counter()
        items = H.ItemSet(metric, dim, np.arange(n, dtype=np.uint32), codes, headers)
        with H.Builder(items, device=0, **kw) as b:
            b.sync()
            t2 = time.perf_counter()
        return t2 - t0, t2 - t1

    def fused():
        items = H.F32ItemSet(metric, x)
        t0 = time.perf_counter()
        with H.Builder(items, device=0, **kw) as b:
            b.sync()
            t1 = time.perf_counter()
        return t1 - t0, t1 - t0

    ceiling(), two_calls(), fused()  # warm-up: code objects, first pinned allocations
    ta, tb, tc, ub, uc = [], [], [], [], []
    for _ in range(repeat):
        ta.append(ceiling())
        t, u = two_calls()
        tb.append(t)
        ub.append(u)
        t, u = fused()
        tc.append(t)
        uc.append(u)
    del pinned, dst

    def rate(ts):
        s = summary(ts)
        s["gb_per_s"] = nbytes / s["median_s"] / 1e9
        s["gb_per_s_min"], s["gb_per_s_max"] = nbytes / s["max_s"] / 1e9, nbytes / s["min_s"] / 1e9
        return s
    res = {"metric": mname, "n": n, "dim": dim, "f32_bytes": nbytes, "repeat": repeat,
           "a_pinned_copy": rate(ta), "b_encode_gpu_then_create": rate(tb), "c_create_f32": rate(tc),
           "b_t_upload_s": summary(ub), "c_t_upload_s": summary(uc)}
    res["c_fraction_of_a"] = res["c_create_f32"]["gb_per_s"] / res["a_pinned_copy"]["gb_per_s"]
    res["c_over_b"] = res["c_create_f32"]["gb_per_s"] / res["b_encode_gpu_then_create"]["gb_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=[])
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every config's items (rehearsals)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--pinned-gib", type=float, default=2.0)
    ap.add_argument("--one", help="(internal) run this config in this process and print its JSON")
    a = ap.parse_args()
    if a.repeat < 5:
        raise SystemExit("--repeat: at least 5")
    if a.one:
        print("RESULT " + json.dumps(run_one(a.one, a.scale, a.repeat, a.pinned_gib)), flush=True)
        return
    out_path = os.environ.get("OUT", os.path.join(ROOT, "bench_out", NAME))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    out = {}
    for src in (os.path.join(ROOT, "profiles", NAME), out_path):  # a run of SOME configs adds to the earlier ones
        if os.path.exists(src):
            out.update(json.load(open(src)))
    for name in a.configs or list(CFG):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[name]), sys.executable, os.path.abspath(__file__), "--one", name,
               "--scale", str(a.scale), "--repeat", str(a.repeat), "--pinned-gib", str(a.pinned_gib)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-2000:])
            raise SystemExit(f"{name}: exit status {p.returncode}; stopping here")
        out[name if a.scale == 1.0 else f"{name}@{a.scale}"] = json.loads(lines[-1][7:])
        r = out[name if a.scale == 1.0 else f"{name}@{a.scale}"]
        print(f"{name}: (a) {r['a_pinned_copy']['gb_per_s']:.1f} GB/s  (b) {r['b_encode_gpu_then_create']['gb_per_s']:.2f} GB/s  "
              f"(c) {r['c_create_f32']['gb_per_s']:.2f} GB/s = {r['c_fraction_of_a']:.2f} of (a), {r['c_over_b']:.2f} x (b); "
              f"t_upload (b) {r['b_t_upload_s']['median_s']:.3f} s (c) {r['c_t_upload_s']['median_s']:.3f} s", flush=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
