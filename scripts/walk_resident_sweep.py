#!/usr/bin/env python3
"""Walk time of 1M x 768 builds against resident waves per CU (HNY_WALK_RESIDENT) x XCD tile (HNY_XCD_TILE): one
process, one data kind, a fresh builder per point -> profiles/walk_resident_sweep.json.
usage: walk_resident_sweep.py KIND OUT.json [points "r:t,r:t,..." (r = 0: switch unset)] [timed builds per point]
SWEEP_METRIC / SWEEP_M / SWEEP_EF select another configuration (C3: euclidean 32 200)."""
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import hannoy_amd as H  # noqa: E402

kind, out_path = sys.argv[1], sys.argv[2]
if len(sys.argv) > 3 and sys.argv[3]:
    points = [tuple(int(v) for v in p.split(":")) for p in sys.argv[3].split(",")]
else:
    points = []
    for r in (16, 12, 8, 6, 4):
        points.append((16, 512))  # the launch before the switch existed
        for t in (512, 256, 128, 64):
            if (r, t) != (16, 512):
                points.append((r, t))
    points.append((16, 512))
builds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
METRIC = os.environ.get("SWEEP_METRIC", "cosine")
MM = int(os.environ.get("SWEEP_M", "16"))
EFC = int(os.environ.get("SWEEP_EF", "100"))

H.load_library()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
x_dev = bench.gen_data(torch, 1_000_000, 768, kind, 42, dev)
x = x_dev.cpu().numpy()
del x_dev
torch.cuda.empty_cache()
items = H.ItemSet.from_f32({"cosine": H.COSINE, "euclidean": H.EUCLIDEAN}[METRIC], x)
H.set_graph_cache(8 << 30)
res = {"data": kind, "workload": f"1000000x768 {METRIC} M{MM} efC{EFC}", "builds_per_point": builds, "points": []}
for pt in points:
    r, t = pt[0], pt[1]
    for k in ("HNY_WALK_RESIDENT", "HNY_XCD_TILE"):
        os.environ.pop(k, None)
    if r:
        os.environ["HNY_WALK_RESIDENT"] = str(r)
    if t != 512:
        os.environ["HNY_XCD_TILE"] = str(t)
    b = H.Builder(items, device=0, M=MM, M0=2 * MM, ef_construction=EFC, seed=42)
    b.set_profiling(True)
    walks, prunes, steps = [], [], []
    g = None
    for i in range(builds + 1):
        g = None
        t0 = time.perf_counter()
        b.reset()
        b.run()
        g = b.finish()
        dt = time.perf_counter() - t0
        if i:  # the first build of a fresh builder is the warm-up
            walks.append(round(g.t_walk_kernels_s * 1e3, 2))
            prunes.append(round(g.t_prune_kernels_s * 1e3, 2))
            steps.append(round(dt * 1e3, 2))
    p = {"waves_per_cu": r or "default", "knob_set": bool(r), "xcd_tile": t, "k_walk_ms": walks, "k_prune_ms": prunes,
         "step_ms": steps, "evals_walk": int(g.n_evals_walk), "nbrs_crc32": zlib.crc32(g.nbrs.tobytes()),
         "n_walk_launches": int(g.n_walk_launches)}
    g = None
    b.close()
    res["points"].append(p)
    print(json.dumps(p), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
