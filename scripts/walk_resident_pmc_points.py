#!/usr/bin/env python3
"""Per-point sums of the k_walk dispatches in rocprofv3 --pmc counter_collection.csv files of a walk_resident_sweep.py run
(one build per point, points in order).  usage: walk_resident_pmc_points.py POINTS.json out.json csv [csv ...]"""
import collections
import csv
import json
import sys

pts = json.load(open(sys.argv[1]))["points"]
out = []
sums = collections.defaultdict(lambda: collections.defaultdict(float))
for path in sys.argv[3:]:
    per = collections.defaultdict(list)  # counter -> [(dispatch, value)]
    for r in csv.DictReader(open(path)):
        if "k_walk" in r["Kernel_Name"] and "k_walk_heap" not in r["Kernel_Name"]:
            per[r["Counter_Name"]].append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    for c, rows in per.items():
        rows.sort()
        at = 0
        for i, p in enumerate(pts):
            n = p["n_walk_launches"]
            sums[i][c] += sum(v for _, v in rows[at:at + n])
            sums[i][c + "_dispatches"] = len(rows[at:at + n])
            at += n
        if at != len(rows):
            print(f"{path}: {c}: {len(rows)} k_walk rows, points account for {at}", file=sys.stderr)
for i, p in enumerate(pts):
    s = dict(sums[i])
    o = {"waves_per_cu": p["waves_per_cu"], "xcd_tile": p["xcd_tile"], **s}
    if "FETCH_SIZE" in s:
        o["fabric_read_bytes_x2"] = 2.0 * s["FETCH_SIZE"] * 1024
    if "TCC_HIT_sum" in s:
        o["l2_hit_rate"] = s["TCC_HIT_sum"] / max(1.0, s["TCC_HIT_sum"] + s["TCC_MISS_sum"])
    out.append(o)
    print(json.dumps(o))
json.dump(out, open(sys.argv[2], "w"), indent=1)
