#!/usr/bin/env python3
"""Cost of the cylinder regression (GM_CFG_CYLINDER_FIT) on blocking frames: plane + cylinder RANSAC with the flag off and
on, alternated frame by frame on the same input, median wall time of gm_process_frame per leg, and the fit's result.

  python tools/cylfit_timing.py [--points 1000000] [--frames 30]

With --group R: one sharded frame over R loopback ranks on device 0 (gm_group_process_frame, no fit flag), then
--frames calls of gm_group_fit_cylinder on it; median wall time of the call and the fit's result.

For the kernel times of the four passes run it under rocprofv3 in a run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -o fit -- python tools/cylfit_timing.py --points 10000000 --frames 5 --only-on
  rocprofv3 --kernel-trace --stats -d OUT -o grp -- python tools/cylfit_timing.py --points 10000000 --frames 5 --group 4
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
    ap.add_argument("--only-on", action="store_true", help="flag-on frames only (profiling)")
    ap.add_argument("--group", type=int, default=0, help="R > 0: gm_group_fit_cylinder over R loopback ranks")
    a = ap.parse_args()
    xyz = synth.tunnel_frame(a.points, seed=2, floor_z=-1.2, outlier_frac=0.01)
    base = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), ransac_hypotheses=1024, ransac_threshold=0.03,
              ransac_seed=7, max_points=a.points)
    if a.group > 0:
        group_timing(a, xyz, base, kw)
        return
    legs = {"on": base | _lib.GM_CFG_CYLINDER_FIT} if a.only_on else {"off": base, "on": base | _lib.GM_CFG_CYLINDER_FIT}
    ctxs = {k: g.GeometricMapping(flags=f, **kw) for k, f in legs.items()}
    times = {k: [] for k in legs}
    for k, c in ctxs.items():
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
        out["fit_cost_ms"] = out["on"]["median_ms"] - out["off"]["median_ms"]
    f = ctxs["on"].cylinder_fit()
    res = ctxs["on"].process_frame(xyz)
    n_el = int((ctxs["on"].labels() != 1).sum())
    print(dict(points=a.points, n_valid=res["n_valid"], eligible=n_el, status=f["status"], radius=f["radius"],
               axis=f["axis"].tolist(), point=f["point"].tolist(), inliers=f["inliers"], last_step=f["last_step"],
               rms=f["rms"], hypothesis=res["cylinder"].tolist(), **out))
    for c in ctxs.values():
        c.close()


def group_timing(a, xyz, base, kw):
    with g.GeometricMappingGroup([0] * a.group, loopback=True, flags=base, **kw) as grp:
        res = grp.process_frame(xyz)
        for _ in range(3):
            grp.fit_cylinder()
        times = []
        for _ in range(a.frames):
            t0 = time.perf_counter()
            f = grp.fit_cylinder()
            times.append((time.perf_counter() - t0) * 1e3)
        n_el = int((grp.labels() != 1).sum())
    print(dict(points=a.points, ranks=a.group, n_valid=res["n_valid"], eligible=n_el, status=f["status"],
               radius=f["radius"], axis=f["axis"].tolist(), point=f["point"].tolist(), inliers=f["inliers"],
               last_step=f["last_step"], rms=f["rms"], hypothesis=res["cylinder"].tolist(),
               fit_median_ms=float(np.median(times)), fit_p10_ms=float(np.percentile(times, 10)),
               fit_p90_ms=float(np.percentile(times, 90))))


if __name__ == "__main__":
    main()
