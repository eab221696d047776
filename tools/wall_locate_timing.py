#!/usr/bin/env python3
"""Cost of the wall-map locate (gm_wall_map_locate_*): what a locate_frame per frame adds to a blocking frame that checks
and adds itself to the map, and a driver for the kernel trace.

  python tools/wall_locate_timing.py [--points 1000000] [--frames 40]  blocking frames with check + add and with
                                                                       locate + result + check + add under the located
                                                                       pose, alternated in both orders in one process:
                                                                       medians, ratio, cost
  python tools/wall_locate_timing.py --kernel [--points N]             blocking frames with the plane and cylinder RANSAC
                                                                       and the cylinder regression, each followed by a
                                                                       locate against the design, a locate against the
                                                                       map and a check: the three passes of k_wall_locate
                                                                       in both references, k_wall_check and k_cylfit_gn
                                                                       on the same valid cloud.  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_locate_timing.py --kernel --frames 8
                                                                       in a run of its own, then
  python tools/wall_locate_timing.py --summarize OUT                   per-kernel calls, median / min / max from the trace
                                                                       and a locate pass as a ratio to a k_cylfit_gn pass"""
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

NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel sits around chainage 0
WARMUP = 3
TRUE = synth.pose_matrix((0.0, 0.0, 0.0))
OFF = synth.pose_matrix((0.0, 0.03, -0.02), yaw_deg=0.3, pitch_deg=-0.2)   # the caller's pose: 3.6 cm and 6 mrad off


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def pipeline(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)
        c.process_frame(xyz)
        m.add_frame(0, TRUE)                      # the survey the MAP locate and the check read
        m.sync()
        last = {}

        def frame(locate):
            t0 = time.perf_counter()
            c.process_frame(xyz)
            pose = TRUE                           # (without a locate: the pose a perfect odometry would hand over)
            if locate:
                m.locate_frame(0, OFF, reference=_lib.GM_WALL_LOCATE_MAP)
                r = m.locate_result(0)
                pose = r["pose"]
                last.update(status=r["status"], lateral=r["lateral"].tolist(), tilt=r["tilt"].tolist())
            m.check_frame(0, pose)
            info, rec = m.check_result(0)
            last["changed_with" if locate else "changed_without"] = len(rec)
            m.add_frame(0, pose)
            m.sync()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(WARMUP):
            frame(False), frame(True)
        t = {False: [], True: []}
        for k in range(a.frames):
            for locate in ((False, True) if k % 2 else (True, False)):
                t[locate].append(frame(locate))
        out = dict(check_and_add=stats(t[False]), locate_check_and_add=stats(t[True]),
                   ratio=float(np.median(t[True]) / np.median(t[False])),
                   locate_cost_ms=float(np.median(t[True]) - np.median(t[False])), last=last)
    print(json.dumps(dict(points=a.points, frames=a.frames, blocking_ms=out)))


def kernel(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    flags = (_lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER | _lib.GM_CFG_CYLINDER_FIT)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points, flags=flags, ransac_hypotheses=1024,
              ransac_threshold=0.03, ransac_seed=7)
    with g.GeometricMapping(**kw) as c:
        m = c.wall_map(**NOMINAL)
        c.process_frame(xyz)
        m.add_frame(0, TRUE)
        m.sync()
        for _ in range(WARMUP + a.frames):
            res = c.process_frame(xyz)
            m.locate_frame(0, OFF, reference=_lib.GM_WALL_LOCATE_DESIGN)
            design = m.locate_result(0)
            m.locate_frame(0, OFF, reference=_lib.GM_WALL_LOCATE_MAP)
            against_map = m.locate_result(0)
            m.check_frame(0, against_map["pose"])
            info, _ = m.check_result(0)
        print(json.dumps(dict(points=len(xyz), n_valid=res["n_valid"], calls=WARMUP + a.frames,
                              design=dict(status=design["status"], used=[q["used"] for q in design["pass"]],
                                          lateral=design["lateral"].tolist(), tilt=design["tilt"].tolist()),
                              map=dict(status=against_map["status"], used=[q["used"] for q in against_map["pass"]],
                                       unsurveyed=[q["unsurveyed"] for q in against_map["pass"]]),
                              check_changed=info["changed_pos"] + info["changed_neg"])))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: float(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        for key, tag in (("k_wall_locate", "k_wall_locate"), ("WallCheckPred", "k_wall_check"), ("k_cylfit_gn", "k_cylfit_gn"),
                         ("k_wall_add", "k_wall_add")):
            if key in name:
                by.setdefault(tag, []).append(us)
    loc = by.get("k_wall_locate", [])
    series = {f"k_wall_locate_design_pass{k}": loc[k::6] for k in range(3)}
    series.update({f"k_wall_locate_map_pass{k}": loc[3 + k::6] for k in range(3)})
    series["k_wall_check"] = by.get("k_wall_check", [])
    gn = by.get("k_cylfit_gn", [])
    series.update({f"k_cylfit_gn_pass{k}": gn[k::3] for k in range(3)})
    out = {}
    for name, v in series.items():
        v = v[WARMUP:] if len(v) > 2 * WARMUP else v
        if v:
            out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    if "k_cylfit_gn_pass0" in out:
        for k in list(out):
            if k.startswith("k_wall_locate"):
                out[k]["ratio_to_cylfit_gn_pass0"] = round(out[k]["median_us"] / out["k_cylfit_gn_pass0"]["median_us"], 3)
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
