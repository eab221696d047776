#!/usr/bin/env python3
"""Cost of the persistent wall map (gm_wall_*): what an add_frame per frame adds to the pipeline, the time of a read, and
a driver for the kernel trace.

  python tools/wall_timing.py [--points 1000000] [--frames 40]    streaming loop (4 slots) and blocking frames, with and
                                                                  without an add_frame per frame, alternated in both
                                                                  orders in one call: medians and ratios
  python tools/wall_timing.py --read                              gm_wall_map_read of a 48-station window and of a whole
                                                                  2^24-cell map
  python tools/wall_timing.py --kernel [--points N | --lidar]     blocking frames with GM_CFG_SURFACE_MAP, each followed by
                                                                  an add_frame against the nominal design: k_surface_map
                                                                  and k_wall_add on the same valid cloud.  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_timing.py --kernel --points 10000000 --frames 8
                                                                  in a run of its own, then
  python tools/wall_timing.py --summarize OUT                     per-kernel calls, median / min / max from the trace

GM_WALL_POINTS_PER_BLOCK=N in the environment changes k_wall_add's grid (points per 1024-thread block; default 16384)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib, synth  # noqa: E402

IDENT = np.eye(4)[:3]
NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel and the lidar frame sit around chainage 0


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def pipeline(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    out = {}
    # four streaming slots: submit (+ add) into the slot whose frame was waited for, F frames per leg
    with g.GeometricMapping(n_slots=4, **kw) as c:
        m = c.wall_map(**NOMINAL)

        def leg(add):
            t0 = time.perf_counter()
            for k in range(a.frames):
                s = k % 4
                if k >= 4:
                    c.wait_frame(s)
                c.submit_frame(s, xyz)
                if add:
                    m.add_frame(s, IDENT)
            for s in range(4):
                c.wait_frame(s)
            if add:
                m.sync()
            return (time.perf_counter() - t0) * 1e3 / a.frames

        leg(False), leg(True)
        t = {False: [], True: []}
        for order in ((False, True), (True, False)) * a.rounds:
            for add in order:
                t[add].append(leg(add))
        out["streaming_ms_per_frame"] = dict(without=stats(t[False]), with_add=stats(t[True]),
                                             ratio=float(np.median(t[True]) / np.median(t[False])))
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)

        def frame(add):
            t0 = time.perf_counter()
            c.process_frame(xyz)
            if add:
                m.add_frame(0, IDENT)
                m.sync()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(3):
            frame(False), frame(True)
        t = {False: [], True: []}
        for k in range(a.frames):
            for add in ((False, True) if k % 2 else (True, False)):
                t[add].append(frame(add))
        out["blocking_ms"] = dict(without=stats(t[False]), with_add=stats(t[True]),
                                  ratio=float(np.median(t[True]) / np.median(t[False])),
                                  add_cost_ms=float(np.median(t[True]) - np.median(t[False])))
        out["info"] = {k: v for k, v in m.info().items() if isinstance(v, int)}
    print(json.dumps(dict(points=a.points, frames=a.frames, **out)))


def read(a):
    xyz = synth.tunnel_patches(200_000, seed=2)
    with g.GeometricMapping() as c:
        out = {}
        for name, prm, s0, n in (("window_48_stations", dict(NOMINAL), 1976, 48),
                                 ("whole_2^24_cells", dict(n_stations=(1 << 24) // 90, t_min=-500.0), 0, None)):
            m = c.wall_map(**prm)
            m.add_points(xyz, IDENT, outputs=False)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                cells = m.read(s0, n)
                t.append((time.perf_counter() - t0) * 1e3)
            out[name] = dict(cells=int(cells[0].size), hit=int((cells[0] > 0).sum()), **stats(t))
            m.close()
        print(json.dumps(out))


def kernel(a):
    if a.lidar:
        xyz = synth.velodyne_tunnel(rings=64)["xyz"]
        kw = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
    else:
        xyz = synth.tunnel_patches(a.points, seed=2)
        kw = dict(neighborRadius=synth.fixed_k_radius(a.points), ransac_hypotheses=1024, ransac_threshold=0.03,
                  ransac_seed=7, max_points=a.points)
    flags = (_lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER | _lib.GM_CFG_CYLINDER_FIT |
             _lib.GM_CFG_SURFACE_MAP)
    design = dict(point=(0.0, 0.3, 0.5)) if a.lidar else {}
    with g.GeometricMapping(flags=flags, **kw) as c:
        m = c.wall_map(**dict(NOMINAL, **design))
        for _ in range(3 + a.frames):
            res = c.process_frame(xyz)
            m.add_frame(0, IDENT)
            m.sync()
        s, w = c.surface_map()[0], m.info()
        print(json.dumps(dict(frame="lidar" if a.lidar else "tunnel", points=len(xyz), n_valid=res["n_valid"],
                              surface_mapped=s["mapped"], wall_mapped_per_frame=w["mapped"] // w["frames"],
                              wall_plane_per_frame=w["plane"] // w["frames"], calls=3 + a.frames)))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    by = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if "k_wall" in name or "k_surface_map" in name:
            by.setdefault(name, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, v in by.items():
        v = v[3:] if len(v) > 6 else v      # (the warm-up calls)
        out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the streaming legs (each in both orders)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lidar", action="store_true")
    ap.add_argument("--read", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.read:
        read(a)
    elif a.kernel:
        kernel(a)
    else:
        pipeline(a)


if __name__ == "__main__":
    main()
