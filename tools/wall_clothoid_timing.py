#!/usr/bin/env python3
"""Cost of the clothoid instantiations of the wall map's add and check beside the straight and the arc ones, on one valid
cloud.

  python tools/wall_clothoid_timing.py --kernel [--points 1000000] [--frames 12]
        blocking frames; after each, an add_frame and a check_frame on a straight map, on a map whose design axis is a
        300 m-radius arc tangent to the same tunnel, and on a map whose axis is the clothoid that osculates that arc at
        chainage 0 and tightens by 1e-5 per metre (over the crop box the three axes part by 4 cm at most, the last two by
        0.2 mm, so the maps bin nearly the same points).  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_clothoid_timing.py --kernel
        in a run of its own, then
  python tools/wall_clothoid_timing.py --summarize OUT     per-kernel calls, median / min / max from the trace
On a commit without gm_wall_map_create_clothoid --kernel times the straight and the arc maps alone (tools/wall_arc_timing.py
does the same there)."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import synth  # noqa: E402

IDENT = np.eye(4)[:3]
NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel sits around chainage 0
ARC = dict(curvature=(0.0, 0.6 / 300.0, 0.8 / 300.0), point_chainage=0.0)
CLOTHOID = dict(normal=(0.0, 0.6, 0.8), curvature=1.0 / 300.0, rate=1.0e-5, point_chainage=0.0)
KERNELS = (("WallCheckPredClothoid", "check_clothoid"), ("WallCheckPredArc", "check_arc"), ("WallCheckPred", "check"),
           ("k_wall_add_clothoid_masked", "k_wall_add_clothoid_masked"), ("k_wall_add_clothoid", "k_wall_add_clothoid"),
           ("k_wall_add_arc_masked", "k_wall_add_arc_masked"), ("k_wall_add_arc", "k_wall_add_arc"),
           ("k_wall_add_masked", "k_wall_add_masked"), ("k_wall_add", "k_wall_add"))


def kernel(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        maps = dict(straight=c.wall_map(**NOMINAL), arc=c.wall_map(arc=ARC, **NOMINAL))
        if hasattr(c._L, "gm_wall_map_create_clothoid"):
            maps["clothoid"] = c.wall_map(clothoid=CLOTHOID, **NOMINAL)
        for _ in range(3 + a.frames):
            res = c.process_frame(xyz)
            for m in maps.values():
                m.add_frame(0, IDENT)
                m.check_frame(0, IDENT)
                m.sync()
        out = dict(points=len(xyz), n_valid=res["n_valid"], calls=3 + a.frames)
        for k, m in maps.items():
            i = m.info()
            out[k] = dict(mapped_per_frame=i["mapped"] // i["frames"], beyond_gate_per_frame=i["beyond_gate"] // i["frames"])
        print(json.dumps(out))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    by = {}
    for r in rows:
        for key, name in KERNELS:   # (the longer names first)
            if key in r["Kernel_Name"]:
                by.setdefault(name, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
                break
    out = {}
    for name, v in by.items():
        v = v[3:] if len(v) > 6 else v      # (the warm-up calls)
        out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernel:
        kernel(a)
    else:
        ap.error("--kernel or --summarize DIR")


if __name__ == "__main__":
    main()
