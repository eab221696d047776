#!/usr/bin/env python3
"""Cost of the wall deviation map (GM_CFG_SURFACE_MAP) on blocking frames: plane + cylinder RANSAC + cylinder fit with the
map flag off and on, alternated frame by frame on the same input, median wall time of gm_process_frame per leg, and the
map's class counts.

  python tools/surface_timing.py [--points 1000000] [--frames 30] [--lidar]

--lidar uses the 64-ring lidar frame (synth.velodyne_tunnel, ring by azimuth: long runs of one cell) instead of the
patch tunnel (synth.tunnel_patches, random order).  For the kernel time run it under rocprofv3 in a run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -o surf -- python tools/surface_timing.py --points 10000000 --frames 5 --only-on
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--lidar", action="store_true", help="the 64-ring lidar frame instead of the patch tunnel")
    ap.add_argument("--only-on", action="store_true", help="flag-on frames only (profiling)")
    a = ap.parse_args()
    if a.lidar:
        xyz = synth.velodyne_tunnel(rings=64)["xyz"]
        kw = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
    else:
        xyz = synth.tunnel_patches(a.points, seed=2)
        kw = dict(neighborRadius=synth.fixed_k_radius(a.points), ransac_hypotheses=1024, ransac_threshold=0.03,
                  ransac_seed=7, max_points=a.points)
    base = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER | _lib.GM_CFG_CYLINDER_FIT
    on = base | _lib.GM_CFG_SURFACE_MAP
    legs = {"on": on} if a.only_on else {"off": base, "on": on}
    ctxs = {k: g.GeometricMapping(flags=f, **kw) for k, f in legs.items()}
    times = {k: [] for k in legs}
    for c in ctxs.values():
        for _ in range(3):
            c.process_frame(xyz)
    for _ in range(a.frames):
        for k, c in ctxs.items():
            t0 = time.perf_counter()
            c.process_frame(xyz)
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
           for k, v in times.items()}
    if "off" in out:
        out["map_cost_ms"] = out["on"]["median_ms"] - out["off"]["median_ms"]
    res = ctxs["on"].process_frame(xyz)
    info = ctxs["on"].surface_map()[0]
    print(dict(frame="lidar" if a.lidar else "tunnel", points=len(xyz), n_valid=res["n_valid"], status=info["status"],
               mapped=info["mapped"], outside=info["outside"], beyond_gate=info["beyond_gate"], plane=info["plane"],
               cells_hit=info["cells_hit"], **out))
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
