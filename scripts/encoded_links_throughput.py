#!/usr/bin/env python3
"""From a finished builder to a closed data.mdb (with_items = 0), through both exports.

For each shape one built builder (Hamming rows of 128 bits, M 16 / M0 32: only the graph matters here), then
  (a) Builder.finish() + Graph.write_lmdb: lists padded to M0 downloaded, compacted and serialised on the host, and
  (b) Builder.finish_encoded() + EncodedLinks.write_lmdb: values serialised on the device (hny_export.hip).
One warm-up of each, then --repeat (default 3) alternating repetitions; medians and min .. max, the split of (b) into
device time, download and sink, the bytes each path downloads and `cmp` of the two files go to
bench_out/encoded_links_throughput.json (OUT=path overrides; the committed copy is under profiles/).

  python scripts/encoded_links_throughput.py [S1M S10M] [--repeat 3]

Without --one the script is a driver: every shape runs in a child process of its own under `timeout`, and the
first failure stops the run.
"""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"S1M": (1_000_000, 128, 16, 64), "S10M": (10_000_000, 128, 16, 64)}
STEP_TIMEOUT_S = {"S1M": 300, "S10M": 380}
NAME = "encoded_links_throughput.json"


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def run_one(name, repeat):
    import numpy as np
    import hannoy_amd as H
    n, bits, M, ef = CFG[name]
    rng = np.random.default_rng(42)
    codes = rng.integers(0, 256, (n, bits // 8), dtype=np.uint8)
    headers = np.zeros((n, H.header_bytes(H.HAMMING)), np.uint8)
    items = H.ItemSet(H.HAMMING, bits, np.arange(n, dtype=np.uint32), codes, headers)
    out = {"shape": name, "n": n, "bits": bits, "M": M, "M0": 2 * M, "ef_construction": ef}
    tmp = tempfile.mkdtemp(prefix="hny_enc_")
    fa, fb = os.path.join(tmp, "a.mdb"), os.path.join(tmp, "b.mdb")
    with H.Builder(items, M=M, M0=2 * M, ef_construction=ef, seed=42, device=0) as b:
        t = time.perf_counter()
        b.run()
        b.sync()
        out["build_s"] = time.perf_counter() - t

        def path_a():
            t0 = time.perf_counter()
            g = b.finish()
            t1 = time.perf_counter()
            g.write_lmdb(fa, with_items=False)
            t2 = time.perf_counter()
            return {"total_s": t2 - t0, "finish_s": t1 - t0, "sink_s": t2 - t1,
                    "records": len(g.rec_item), "links": int(g.offsets[-1])}

        def path_b():
            t0 = time.perf_counter()
            e = b.finish_encoded()
            t1 = time.perf_counter()
            e.write_lmdb(fb, with_items=False)
            t2 = time.perf_counter()
            return {"total_s": t2 - t0, "finish_s": t1 - t0, "sink_s": t2 - t1, "device_s": e.t_device_s,
                    "download_s": e.t_download_s, "bytes_downloaded": int(e.bytes_downloaded)}

        wa, wb = path_a(), path_b()  # warm-up (and the builder's record table on the device)
        out["records"], out["links"] = wa["records"], wa["links"]
        out["bytes_downloaded_a"] = 4 * n * 2 * M + 4 * n  # layer-0 slots and counts (the upper layers are small)
        out["bytes_downloaded_b"] = wb["bytes_downloaded"]
        ra, rb = [], []
        for _ in range(repeat):
            ra.append(path_a())
            rb.append(path_b())
        out["a"] = {k: summary([r[k] for r in ra]) for k in ("total_s", "finish_s", "sink_s")}
        out["b"] = {k: summary([r[k] for r in rb]) for k in ("total_s", "finish_s", "sink_s", "device_s", "download_s")}
        out["cmp_equal"] = bool(filecmp.cmp(fa, fb, shallow=False))
        out["data_mdb_bytes"] = os.path.getsize(fa)
    a, bb = out["a"]["total_s"], out["b"]["total_s"]
    out["b_faster_beyond_a_spread"] = bool(a["median_s"] - bb["median_s"] > a["max_s"] - a["min_s"])
    for f in (fa, fb):
        os.remove(f)
    os.rmdir(tmp)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["S1M", "S10M"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    if a.one:
        return run_one(a.shapes[0], a.repeat)
    results = []
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[name]), sys.executable, os.path.abspath(__file__), name, "--one",
               "--repeat", str(a.repeat)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"{name}: exit code {r.returncode}; stopping", file=sys.stderr)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    path = os.environ.get("OUT") or os.path.join(ROOT, "bench_out", NAME)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"results": results}, f, indent=1)
    print(json.dumps({"results": results}))
    return 0 if len(results) == len(a.shapes) else 1


if __name__ == "__main__":
    sys.exit(main())
