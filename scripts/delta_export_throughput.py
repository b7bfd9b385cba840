#!/usr/bin/env python3
"""From a finished successor builder to the records of its delta in a sink, through both delta exports.

One built index (Hamming rows of 128 bits, M 16 / M0 32: only the graph matters here), then for each update size a
successor (hny_builder_create_update: half of the upserts overwrite items, half are new ids, as many deletes; every
batch and fill_gaps run) and on it
  (old) hny_builder_finish_delta + hny_encode_kv: flags and counts downloaded, the changed records found on one host
        thread, their lists gathered, downloaded, mapped to ids and roaring-encoded on the host, and
  (new) hny_builder_finish_delta_encoded + hny_encode_kv_encoded: record table and values made on the device
        (hny_export.hip).
Both streams go into the same counting sink (a C function compiled on the spot; a ctypes callback if no C compiler is
found, which costs both paths the same time per record and is named in the result).  One warm-up of each, then
--repeat (default 5) alternating repetitions in the same process; medians and min .. max, the split of (new) into
device time and download, the bytes either path downloads and whether both sinks saw the same bytes go to
bench_out/encoded_delta_throughput.json (OUT=path overrides; the committed copy is under profiles/).

  python scripts/delta_export_throughput.py [U1 U10] [--repeat 5]

Without --one the script is a driver: every update size runs in a child process of its own under `timeout`, and the
first failure stops the run.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, BITS, M, EF = 1_000_000, 128, 16, 64
CFG = {"U1": 0.01, "U10": 0.10}  # upserts as a fraction of the items; as many deletes
STEP_TIMEOUT_S = 300
NAME = "encoded_delta_throughput.json"

SINK_C = """
#include <stddef.h>
#include <stdint.h>
typedef struct { uint64_t records, bytes, sum; } counts;
int counting_sink(void *ctx, const uint8_t *k, size_t kl, const uint8_t *v, size_t vl) {
  counts *c = (counts *)ctx;
  c->records++;
  c->bytes += kl + vl;
  for (size_t i = 0; i < kl; i++) c->sum = c->sum * 1099511628211ull + k[i];
  for (size_t i = 0; i < vl; i++) c->sum = c->sum * 1099511628211ull + v[i];
  return 0;
}
"""


class Counts(C.Structure):
    _fields_ = [("records", C.c_uint64), ("bytes", C.c_uint64), ("sum", C.c_uint64)]


def make_sink(capi, tmp):
    """(kind, sink, new_ctx, read_ctx)"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src, lib = os.path.join(tmp, "sink.c"), os.path.join(tmp, "libsink.so")
        with open(src, "w") as f:
            f.write(SINK_C)
        if subprocess.run([cc, "-O2", "-shared", "-fPIC", src, "-o", lib]).returncode == 0:
            fn = C.cast(C.CDLL(lib).counting_sink, capi.KV_SINK)
            box = []

            def new_ctx():
                box[:] = [Counts()]
                return C.byref(box[0])
            return "c", fn, new_ctx, lambda: (box[0].records, box[0].bytes, box[0].sum)
    acc = [0, 0, 0]

    def py_sink(_ctx, k, kl, v, vl):
        acc[0] += 1
        acc[1] += kl + vl
        acc[2] = zlib.crc32(C.string_at(v, vl), zlib.crc32(C.string_at(k, kl), acc[2]))
        return 0

    def new_ctx():
        acc[:] = [0, 0, 0]
        return None
    return "ctypes callback", capi.KV_SINK(py_sink), new_ctx, lambda: tuple(acc)


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def run_one(name, repeat):
    import numpy as np
    import hannoy_amd as H
    from hannoy_amd import _capi as capi
    L = H.load_library()
    frac = CFG[name]
    k = int(N * frac)
    rng = np.random.default_rng(42)
    codes = rng.integers(0, 256, (N + k, BITS // 8), dtype=np.uint8)
    headers = np.zeros((N + k, H.header_bytes(H.HAMMING)), np.uint8)
    items = H.ItemSet(H.HAMMING, BITS, np.arange(N, dtype=np.uint32), codes[:N], headers[:N])
    out = {"shape": name, "n": N, "bits": BITS, "M": M, "M0": 2 * M, "ef_construction": EF, "upserts": k, "deletes": k}
    tmp = tempfile.mkdtemp(prefix="hny_delta_")
    kind, sink, new_ctx, read_ctx = make_sink(capi, tmp)
    out["sink"] = kind
    pick = rng.permutation(N)
    dele = np.sort(pick[:k]).astype(np.uint32)
    over = np.sort(pick[k:k + k // 2]).astype(np.uint32)
    ups = np.concatenate([over, np.arange(N, N + k - len(over), dtype=np.uint32)])
    up_codes = np.concatenate([rng.integers(0, 256, (len(over), BITS // 8), dtype=np.uint8), codes[N:N + k - len(over)]])
    with H.Builder(items, M=M, M0=2 * M, ef_construction=EF, seed=42, device=0) as b:
        t = time.perf_counter()
        b.run()
        b.sync()
        out["build_s"] = time.perf_counter() - t
        with b.create_update(ups, codes=up_codes, headers=headers[:len(ups)], delete_ids=dele, seed=43) as s:
            t = time.perf_counter()
            s.run()
            s.sync()
            out["update_s"] = time.perf_counter() - t
            ids = np.ascontiguousarray(s.items.ids, np.uint32)
            it = capi.Items(len(ids), ids.ctypes.data, None, 0, None, 0, None)

            def path_old():
                ctx = new_ctx()
                t0 = time.perf_counter()
                dp = C.POINTER(capi.GraphDeltaStruct)()
                assert L.hny_builder_finish_delta(s._h, C.byref(dp)) == 0, L.hny_last_error()
                t1 = time.perf_counter()
                d = dp.contents
                g = capi.GraphStruct()
                g.n_records, g.rec_item, g.rec_layer, g.rec_offset = d.n_records, d.rec_item, d.rec_layer, d.rec_offset
                g.neighbours, g.entry_points = d.neighbours, d.entry_points
                g.n_entry_points, g.max_level = d.n_entry_points, d.max_level
                assert L.hny_encode_kv(C.byref(g), C.byref(s.opts), C.byref(it), 0, 0, sink, ctx) == 0
                t2 = time.perf_counter()
                r = {"total_s": t2 - t0, "finish_s": t1 - t0, "sink_s": t2 - t1, "records": int(d.n_records),
                     "removed": int(d.n_removed), "records_total": int(d.n_records_total),
                     "links": int(d.rec_offset[d.n_records]), "seen": read_ctx()}
                L.hny_graph_delta_free(dp)
                return r

            def path_new():
                ctx = new_ctx()
                t0 = time.perf_counter()
                dp = C.POINTER(capi.EncodedDeltaStruct)()
                assert L.hny_builder_finish_delta_encoded(s._h, C.byref(dp)) == 0, L.hny_last_error()
                t1 = time.perf_counter()
                e = dp.contents.links
                assert L.hny_encode_kv_encoded(C.byref(e), C.byref(s.opts), C.byref(it), 0, 0, sink, ctx) == 0
                t2 = time.perf_counter()
                r = {"total_s": t2 - t0, "finish_s": t1 - t0, "sink_s": t2 - t1, "device_s": e.t_device_s,
                     "download_s": e.t_download_s, "bytes_downloaded": int(e.bytes_downloaded),
                     "records": int(e.n_records), "removed": int(dp.contents.n_removed), "seen": read_ctx()}
                L.hny_encoded_delta_free(dp)
                return r

            wo, wn = path_old(), path_new()  # warm-up (and the successor's masks on the device)
            out["changed_records"], out["removed_keys"] = wo["records"], wo["removed"]
            out["records_total"], out["changed_links"] = wo["records_total"], wo["links"]
            # old: a flag byte and a count per list (at least one list per record), then the changed lists
            out["bytes_downloaded_old_at_least"] = 5 * wo["records_total"] + 4 * wo["links"]
            out["bytes_downloaded_new"] = wn["bytes_downloaded"]
            out["same_stream"] = bool(wo["seen"] == wn["seen"] and wo["records"] == wn["records"]
                                      and wo["removed"] == wn["removed"])
            out["stream_records"], out["stream_bytes"] = int(wo["seen"][0]), int(wo["seen"][1])
            ro, rn = [], []
            for _ in range(repeat):
                ro.append(path_old())
                rn.append(path_new())
            out["old"] = {f: summary([r[f] for r in ro]) for f in ("total_s", "finish_s", "sink_s")}
            out["new"] = {f: summary([r[f] for r in rn]) for f in ("total_s", "finish_s", "sink_s", "device_s", "download_s")}
    out["new_faster"] = bool(out["new"]["total_s"]["median_s"] < out["old"]["total_s"]["min_s"])  # the rule of §3c-3
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["U1", "U10"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    if a.one:
        return run_one(a.shapes[0], a.repeat)
    results = []
    for name in a.shapes:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), name, "--one",
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
