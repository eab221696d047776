#!/usr/bin/env python3
"""Cost of the wall-map align (gm_wall_map_align_*): what an align_frame per frame adds to a blocking frame that checks and
adds itself to the map, and a driver for the kernel trace.

  python tools/wall_align_timing.py [--points 1000000] [--frames 40]   blocking frames with check + add and with
                                                                      align + result + check + add under the aligned
                                                                      pose, alternated in both orders in one process:
                                                                      medians, ratio, cost
  python tools/wall_align_timing.py --kernel [--points N]              blocking frames, each followed by an align with the
                                                                      default parameters, an align with the widest search
                                                                      (A = 64, B = 15) and a locate against the map: the
                                                                      three kernels of an align beside the three passes of
                                                                      k_wall_locate on the same valid cloud.  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_align_timing.py --kernel --frames 8
                                                                      in a run of its own, then
  python tools/wall_align_timing.py --summarize OUT                    per-kernel calls, median / min / max from the trace"""
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

NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the frame sits around chainage 0
WARMUP = 3
TEX = dict(seed=5, amplitude=0.04, length=12.0)
WIDE = dict(max_station_shift=64, max_sector_shift=15)


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def textured_frame(n, seed=2, sigma=0.005):
    """n points of a textured tunnel wall of radius 2 around chainage 0 (the texture's own chainage runs 0 .. 12)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-6.0, 6.0, n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    rr = 2.0 + rng.normal(0.0, sigma, n) + synth.wall_texture(t + 6.0, phi, **TEX)
    return np.ascontiguousarray(np.stack([t, -rr * np.sin(phi), rr * np.cos(phi)], axis=1), dtype=np.float32)


TRUE = synth.pose_matrix((0.0, 0.0, 0.0))
OFF = synth.pose_matrix((-0.5, 0.0, 0.0), roll_deg=-4.0)   # the caller's pose: 2 stations and 1 sector (of 90) short


def pipeline(a):
    xyz = textured_frame(a.points)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)
        c.process_frame(xyz)
        m.add_frame(0, TRUE)                      # the survey the align and the check read
        m.sync()
        last = {}

        def frame(align):
            t0 = time.perf_counter()
            c.process_frame(xyz)
            pose = TRUE                           # (without an align: the pose a perfect odometry would hand over)
            if align:
                m.align_frame(0, OFF)
                r, _ = m.align_result(0)
                pose = r["pose"]
                last.update(status=r["status"], best=(r["best_station"], r["best_sector"]), distinction=r["distinction"],
                            shift_m=r["shift_m"], roll=r["roll"], overlap=r["overlap"])
            m.check_frame(0, pose)
            info, rec = m.check_result(0)
            last["changed_with" if align else "changed_without"] = len(rec)
            m.add_frame(0, pose)
            m.sync()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(WARMUP):
            frame(False), frame(True)
        t = {False: [], True: []}
        for k in range(a.frames):
            for align in ((False, True) if k % 2 else (True, False)):
                t[align].append(frame(align))
        out = dict(check_and_add=stats(t[False]), align_check_and_add=stats(t[True]),
                   ratio=float(np.median(t[True]) / np.median(t[False])),
                   align_cost_ms=float(np.median(t[True]) - np.median(t[False])), last=last)
    print(json.dumps(dict(points=a.points, frames=a.frames, blocking_ms=out)))


def kernel(a):
    xyz = textured_frame(a.points)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)
        c.process_frame(xyz)
        m.add_frame(0, TRUE)
        m.sync()
        for _ in range(WARMUP + a.frames):
            res = c.process_frame(xyz)
            m.align_frame(0, OFF)
            narrow, _ = m.align_result(0)
            m.align_frame(0, OFF, **WIDE)
            wide, _ = m.align_result(0)
            m.locate_frame(0, TRUE, reference=_lib.GM_WALL_LOCATE_MAP)
            m.locate_result(0)
        pick = lambda r: dict(status=r["status"], best=(r["best_station"], r["best_sector"]), overlap=r["overlap"],  # noqa: E731
                              distinction=r["distinction"], binned=r["binned"], usable=r["patch_cells_usable"])
        print(json.dumps(dict(points=len(xyz), n_valid=res["n_valid"], calls=WARMUP + a.frames, default=pick(narrow), wide=pick(wide))))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: float(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        for key in ("k_wall_align_bin", "k_wall_align_values", "k_wall_align_score", "k_wall_locate", "k_wall_add"):
            if key in name:
                by.setdefault(key, []).append(us)
    series = {}
    for key in ("k_wall_align_bin", "k_wall_align_values", "k_wall_align_score"):   # two aligns per frame: default, wide
        v = by.get(key, [])
        series[key + "_default"], series[key + "_wide"] = v[0::2], v[1::2]
    loc = by.get("k_wall_locate", [])
    series.update({f"k_wall_locate_map_pass{k}": loc[k::3] for k in range(3)})
    out = {}
    for name, v in series.items():
        v = v[WARMUP:] if len(v) > 2 * WARMUP else v
        if v:
            out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    for tag in ("default", "wide"):
        keys = [f"k_wall_align_{k}_{tag}" for k in ("bin", "values", "score")]
        if all(k in out for k in keys):
            out[f"align_{tag}_kernels_us"] = round(sum(out[k]["median_us"] for k in keys), 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=40)
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
