#!/usr/bin/env python3
"""From "the bytes of a data.mdb are in memory" to a loaded builder that has answered one search_knn query.

For each shape one built index (Hamming rows of 128 bits, M 16 / M0 32, ids 0 .. n-1: the graphs of
scripts/encoded_links_throughput.py), written to a data.mdb without items and read once so that it sits in the page
cache; the items stay in host memory for both paths.  Then
  (a) hny_lmdb_open + hny_lmdb_scan over the Links range into a compiled sink that decodes every roaring value into a
      CSR (C, built by this script with the system compiler: the library has no host decoder of its own), then
      hny_builder_load on that CSR — the path of the parent commit with its Python loop replaced by C; and
  (b) hny_lmdb_open + hny_lmdb_read_links + hny_builder_load_encoded (hny_import.hip).
Both end with one search_knn query.  One warm-up of each, then --repeat (default 3) alternating repetitions; median
and min .. max go to bench_out/load_encoded_throughput.json (OUT=path overrides; the committed copy is under
profiles/).  The Python decode of hannoy_amd.api (_StoredGraph) is timed once on the 1M shape and reported apart.

  python scripts/load_encoded_throughput.py [S1M S10M] [--repeat 3]

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
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"S1M": (1_000_000, 128, 16, 64), "S10M": (10_000_000, 128, 16, 64)}
STEP_TIMEOUT_S = {"S1M": 300, "S10M": 900}
NAME = "load_encoded_throughput.json"

DECODER_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
typedef struct {
  uint64_t n, cap_r, nl, cap_l;
  uint32_t *item; uint8_t *layer; uint64_t *off; uint32_t *nb;
} csr;
static uint32_t rd(const uint8_t *p, int b) { uint32_t v = 0; for (int k = 0; k < b; k++) v |= (uint32_t)p[k] << (8 * k); return v; }
int csr_sink(void *ctx, const uint8_t *key, size_t kl, const uint8_t *v, size_t vl) {
  csr *c = (csr *)ctx;
  if (kl != 8 || vl < 9 || v[0] != 1 || rd(v + 1, 4) != 12346) return -1;
  if (c->n + 1 >= c->cap_r) {
    c->cap_r = c->cap_r ? 2 * c->cap_r : 1 << 20;
    c->item = realloc(c->item, c->cap_r * 4); c->layer = realloc(c->layer, c->cap_r);
    c->off = realloc(c->off, (c->cap_r + 1) * 8);
    if (!c->n) c->off[0] = 0;
  }
  uint32_t nc = rd(v + 5, 4);
  const uint8_t *p = v + 9 + 8 * (size_t)nc;
  for (uint32_t k = 0; k < nc; k++) {
    uint32_t hi = rd(v + 9 + 4 * k, 2) << 16, card = rd(v + 11 + 4 * k, 2) + 1;
    if (c->nl + 65536 > c->cap_l) { c->cap_l = c->cap_l ? 2 * c->cap_l : 1 << 24; c->nb = realloc(c->nb, c->cap_l * 4); }
    if (card <= 4096) { for (uint32_t i = 0; i < card; i++) c->nb[c->nl++] = hi | rd(p + 2 * i, 2); p += 2 * card; }
    else { for (uint32_t i = 0; i < 65536; i++) if (p[i >> 3] >> (i & 7) & 1) c->nb[c->nl++] = hi | i; p += 8192; }
  }
  c->item[c->n] = (uint32_t)key[3] << 24 | (uint32_t)key[4] << 16 | (uint32_t)key[5] << 8 | key[6];
  c->layer[c->n] = key[7];
  c->off[++c->n] = c->nl;
  return 0;
}
void csr_free(csr *c) { free(c->item); free(c->layer); free(c->off); free(c->nb); memset(c, 0, sizeof *c); }
"""


class Csr(C.Structure):
    _fields_ = [("n", C.c_uint64), ("cap_r", C.c_uint64), ("nl", C.c_uint64), ("cap_l", C.c_uint64),
                ("item", C.c_void_p), ("layer", C.c_void_p), ("off", C.c_void_p), ("nb", C.c_void_p)]


def build_decoder(tmp):
    src, lib = os.path.join(tmp, "csr_sink.c"), os.path.join(tmp, "csr_sink.so")
    with open(src, "w") as f:
        f.write(DECODER_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", lib, src])
    return C.CDLL(lib)


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "n": len(ts)}


def run_one(name, repeat):
    import struct
    import numpy as np
    import hannoy_amd as H
    from hannoy_amd import _capi as capi
    n, bits, M, ef = CFG[name]
    rng = np.random.default_rng(42)
    codes = rng.integers(0, 256, (n, bits // 8), dtype=np.uint8)
    headers = np.zeros((n, H.header_bytes(H.HAMMING)), np.uint8)
    items = H.ItemSet(H.HAMMING, bits, np.arange(n, dtype=np.uint32), codes, headers)
    out = {"shape": name, "n": n, "bits": bits, "M": M, "M0": 2 * M, "ef_construction": ef}
    tmp = tempfile.mkdtemp(prefix="hny_load_")
    path = os.path.join(tmp, "data.mdb")
    kw = dict(M=M, M0=2 * M, ef_construction=ef, seed=42, device=0)
    with H.Builder(items, **kw) as b:
        b.run()
        e = b.finish_encoded()
        e.write_lmdb(path, with_items=False)
        out["records"], out["value_bytes"] = len(e.rec_item), int(e.val_offset[-1])
        eps, max_level = e.entry_points.copy(), e.max_level
        del e
    out["data_mdb_bytes"] = os.path.getsize(path)
    with open(path, "rb") as f:  # into the page cache
        while f.read(1 << 26):
            pass
    L, D = capi.load_library(), build_decoder(tmp)
    sink = C.cast(D.csr_sink, capi.KV_SINK)
    lo, hi = struct.pack(">HBIB", 0, 2, 0, 0), struct.pack(">HBIB", 0, 2, 0xFFFFFFFF, 0xFF)
    q = (codes[:1].copy(), headers[:1].copy())

    def path_a():
        t0 = time.perf_counter()
        csr = Csr()
        with capi.LmdbEnv(path) as env:
            capi._check(L.hny_lmdb_scan(env._e, lo, 8, hi, 8, sink, C.byref(csr)))
        t1 = time.perf_counter()
        pg = capi.PrevGraph(csr.n, csr.item, csr.layer, csr.off, csr.nb, capi._p(eps).value, len(eps), int(max_level))
        it, h = items.struct(), C.c_void_p()
        o = capi.make_opts(H.HAMMING, bits, **kw)
        capi._check(L.hny_builder_load(C.byref(o), C.byref(it), C.byref(pg), C.byref(h)))
        bl = capi.Builder.__new__(capi.Builder)
        bl.items, bl.opts, bl.incremental, bl._h = items, o, True, h
        t2 = time.perf_counter()
        hits = bl.search_knn(*q, k=10, ef_search=64)
        t3 = time.perf_counter()
        links = int(csr.nl)
        bl.close()
        D.csr_free(C.byref(csr))
        return {"total_s": t3 - t0, "read_s": t1 - t0, "load_s": t2 - t1, "query_s": t3 - t2, "links": links}, hits

    def path_b():
        t0 = time.perf_counter()
        with capi.LmdbEnv(path) as env:
            enc = env.read_links(0)
        t1 = time.perf_counter()
        bl = capi.Builder(items, stored=enc, load=True, **kw)
        t2 = time.perf_counter()
        hits = bl.search_knn(*q, k=10, ef_search=64)
        t3 = time.perf_counter()
        bl.close()
        return {"total_s": t3 - t0, "read_s": t1 - t0, "load_s": t2 - t1, "query_s": t3 - t2}, hits

    (wa, ha), (wb, hb) = path_a(), path_b()  # warm-up
    out["links"] = wa["links"]
    out["same_hits"] = bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ha, hb)))
    ra, rb = [], []
    for _ in range(repeat):
        ra.append(path_a()[0])
        rb.append(path_b()[0])
    keys = ("total_s", "read_s", "load_s", "query_s")
    out["a"] = {k: summary([r[k] for r in ra]) for k in keys}
    out["b"] = {k: summary([r[k] for r in rb]) for k in keys}
    out["b_median_below_a_min"] = bool(out["b"]["total_s"]["median_s"] < out["a"]["total_s"]["min_s"])
    if n <= 1_000_000:  # the Python decode of the default Reader, once: reported, not the yardstick
        from hannoy_amd import api
        t0 = time.perf_counter()
        db = api.Database.__new__(api.Database)
        with capi.LmdbEnv(path) as env:
            db.kv = dict(env.items())
        t1 = time.perf_counter()
        api._StoredGraph(db, 0)
        out["python_decode"] = {"scan_to_dict_s": t1 - t0, "stored_graph_s": time.perf_counter() - t1}
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
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
        print(json.dumps(results[-1]), flush=True)
    path = os.environ.get("OUT") or os.path.join(ROOT, "bench_out", NAME)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"results": results}, f, indent=1)
    return 0 if len(results) == len(a.shapes) else 1


if __name__ == "__main__":
    sys.exit(main())
