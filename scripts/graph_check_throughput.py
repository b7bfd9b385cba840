"""What the graph check costs on the device, next to the host route it replaces: finish() (every list to the host) plus
a numpy restatement of the two passes.  Writes profiles/graph_check_throughput.json.

    python scripts/graph_check_throughput.py [--sizes 1000000,10000000] [--reps 3]

Every figure comes from a process of its own that builds the index (Hamming, 128 bits, M 16, M0 32) and times one
route; the parent alternates device and host processes and records median and min .. max.  The device figures are the
wall time of Builder.check_graph (a synchronous call: workspace allocation, kernels, the reads of the frontier
lengths), taken on the second call of each kind."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "graph_check_throughput.json")
KW = dict(M=16, M0=32, ef_construction=48)


def host_check(g, n):
    """dead links and in-links on layer 0, then a level-synchronous BFS over layer 0 from the entry points (ids are
    0 .. n-1 here; the upper layers are a few percent of the links and are left out, in the host's favour)"""
    off = g.offsets.astype(np.int64)
    l0 = np.flatnonzero(g.rec_layer == 0)
    start, cnt = off[l0], off[l0 + 1] - off[l0]
    idx = np.repeat(start - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
    src, dst = np.repeat(g.rec_item[l0], cnt), g.nbrs[idx]
    named = np.zeros(n, bool)
    named[dst] = True
    order = np.argsort(src, kind="stable")
    dst, first = dst[order], np.searchsorted(src[order], np.arange(n + 1))
    seen = np.zeros(n, bool)
    front = np.asarray(g.entry_points, np.int64)
    seen[front] = True
    rounds = 0
    while len(front):
        rounds += 1
        lo, c = first[front], first[front + 1] - first[front]
        t = dst[np.repeat(lo - np.cumsum(c) + c, c) + np.arange(c.sum())]
        front = np.unique(t[~seen[t]]).astype(np.int64)
        seen[front] = True
    return int((~named).sum()), int((~seen).sum()), rounds


def child(route, n):
    import hannoy_amd as H
    rng, step = np.random.default_rng(5), 1 << 20
    parts = [H.encode_vectors(H.HAMMING, rng.uniform(-1, 1, (min(step, n - i), 128)).astype(np.float32))
             for i in range(0, n, step)]
    items = H.ItemSet(H.HAMMING, 128, np.arange(n, dtype=np.uint32), np.concatenate([p[0] for p in parts]),
                      np.concatenate([p[1] for p in parts]))
    out = dict(route=route, n=n)
    with H.Builder(items, **KW) as b:
        b.run()
        if route == "device":
            for name, kw in (("lists_s", dict(reach=False)), ("reach_s", dict(lists=False)), ("both_s", {})):
                b.check_graph(**kw)
                t = time.perf_counter()
                r = b.check_graph(**kw)
                out[name] = time.perf_counter() - t
            out.update(no_inlinks0=r["n_no_inlinks0"], unreachable=r["n_unreachable"], rounds=r["bfs_rounds"],
                       links=sum(r["n_links"]))
        else:
            t = time.perf_counter()
            g = b.finish()
            out["finish_s"] = time.perf_counter() - t
            t = time.perf_counter()
            out["no_inlinks0"], out["unreachable"], out["rounds_layer0"] = host_check(g, n)
            out["numpy_s"] = time.perf_counter() - t
    print(json.dumps(out))


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    arg = lambda name, d: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else d  # noqa: E731
    if "--child" in sys.argv:
        return child(arg("--child", "device"), int(arg("--n", "100000")))
    sizes, reps = [int(s) for s in arg("--sizes", "1000000,10000000").split(",")], int(arg("--reps", "3"))
    result = dict(what="Builder.check_graph against finish() + numpy on the host; Hamming 128 bits, M 16, M0 32",
                  commit=subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                        text=True).stdout.strip(), sizes={})
    for n in sizes:
        runs = dict(device=[], host=[])
        for _ in range(reps):
            for route in ("device", "host"):  # alternating processes
                p = subprocess.run([sys.executable, __file__, "--child", route, "--n", str(n)], capture_output=True,
                                   text=True, check=True)
                runs[route].append(json.loads(p.stdout.strip().splitlines()[-1]))
        d, h = runs["device"], runs["host"]
        assert all(x["unreachable"] == h[0]["unreachable"] and x["no_inlinks0"] == h[0]["no_inlinks0"] for x in d + h)
        result["sizes"][str(n)] = dict(
            links=d[0]["links"], bfs_rounds=d[0]["rounds"], unreachable=d[0]["unreachable"],
            no_inlinks0=d[0]["no_inlinks0"],
            device={k: spread([x[k] for x in d]) for k in ("lists_s", "reach_s", "both_s")},
            host={k: spread([x[k] for x in h]) for k in ("finish_s", "numpy_s")})
        print(n, json.dumps(result["sizes"][str(n)]), flush=True)
    if os.path.exists(OUT):  # keep what other runs recorded there (the bench lines)
        result = dict(json.load(open(OUT)), **result)
    json.dump(result, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
