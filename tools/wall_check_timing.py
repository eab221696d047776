#!/usr/bin/env python3
"""Cost of the wall-map check (gm_wall_map_check_*): what a check_frame per frame adds to a blocking frame that already
adds itself to the map, and a driver for the kernel trace.

  python tools/wall_check_timing.py [--points 1000000] [--frames 40]   blocking frames with add_frame only and with
                                                                       check_frame + check_result + add_frame, alternated
                                                                       in both orders in one process: medians, ratio, cost
  python tools/wall_check_timing.py --kernel [--points N | --lidar]    blocking frames, each followed by two checks -- one
                                                                       against the survey of the same wall (under 1 % of
                                                                       the points changed), one against the same survey
                                                                       moved by 0.3 m with a threshold of one unit (every
                                                                       usable point changed) -- and by an add_frame:
                                                                       k_wall_check and k_wall_add on the same valid
                                                                       cloud.  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_check_timing.py --kernel --frames 8
                                                                       in a run of its own, then
  python tools/wall_check_timing.py --summarize OUT                    per-kernel calls, median / min / max from the trace
                                                                       and the check's time as a ratio to the add's"""
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
from geometric_mapping_amd import synth  # noqa: E402

IDENT = np.eye(4)[:3]
NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel and the lidar frame sit around chainage 0
WARMUP = 3


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def pipeline(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)
        changed = []

        def frame(check):
            t0 = time.perf_counter()
            c.process_frame(xyz)
            if check:
                m.check_frame(0, IDENT)
                info, rec = m.check_result(0)
                changed.append(len(rec))
            m.add_frame(0, IDENT)
            m.sync()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(WARMUP):
            frame(False), frame(True)
        t = {False: [], True: []}
        for k in range(a.frames):
            for check in ((False, True) if k % 2 else (True, False)):
                t[check].append(frame(check))
        out = dict(add_only=stats(t[False]), check_and_add=stats(t[True]),
                   ratio=float(np.median(t[True]) / np.median(t[False])),
                   check_cost_ms=float(np.median(t[True]) - np.median(t[False])), changed_points_last=changed[-1])
    print(json.dumps(dict(points=a.points, frames=a.frames, blocking_ms=out)))


def kernel(a):
    if a.lidar:
        xyz = synth.velodyne_tunnel(rings=64)["xyz"]
        kw = {}
        design = dict(point=(0.0, 0.3, 0.5))
    else:
        xyz = synth.tunnel_patches(a.points, seed=2)
        kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
        design = {}
    with g.GeometricMapping(**kw) as c:
        p = dict(NOMINAL, **design)
        survey, moved, sink = c.wall_map(**p), c.wall_map(**p), c.wall_map(**p)
        c.process_frame(xyz)
        for _ in range(4):
            survey.add_frame(0, IDENT)
        survey.sync()
        raw = survey.read_raw()
        raw["sum"] += raw["count"].astype(np.int64) * int(0.3 * 2 ** 20)
        moved.add_raw(raw)
        for _ in range(WARMUP + a.frames):
            res = c.process_frame(xyz)
            survey.check_frame(0, IDENT, min_count=1)
            few, _ = survey.check_result(0)
            moved.check_frame(0, IDENT, min_count=1, threshold=2.0 ** -20, gate=0.25)
            every, _ = moved.check_result(0)
            sink.add_frame(0, IDENT)
            sink.sync()
        share = lambda i: (i["changed_pos"] + i["changed_neg"]) / max(i["n_points"], 1)  # noqa: E731
        print(json.dumps(dict(frame="lidar" if a.lidar else "tunnel", points=len(xyz), n_valid=res["n_valid"],
                              changed_share_low=share(few), changed_share_all=share(every),
                              usable_share_all=1.0 - (every["unsurveyed"] + every["beyond_gate"] + every["outside"]) / max(every["n_points"], 1),
                              calls=WARMUP + a.frames)))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: float(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        if "WallCheckPred" in name:
            by.setdefault("k_wall_check", []).append(us)
        elif "k_wall_add" in name:
            by.setdefault("k_wall_add", []).append(us)
    out = {}
    chk = by.get("k_wall_check", [])
    series = {"k_wall_check_low": chk[0::2], "k_wall_check_all": chk[1::2], "k_wall_add": by.get("k_wall_add", [])[4:]}
    for name, v in series.items():
        v = v[WARMUP:] if len(v) > 2 * WARMUP else v
        if v:
            out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    if "k_wall_add" in out:
        for k in ("k_wall_check_low", "k_wall_check_all"):
            if k in out:
                out[k]["ratio_to_add"] = round(out[k]["median_us"] / out["k_wall_add"]["median_us"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--lidar", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernel:
        kernel(a)
    else:
        pipeline(a)


if __name__ == "__main__":
    main()
