#!/usr/bin/env python3
"""Cost of the three passes of the locate on a wall alignment (k_wall_locate_joint) beside the element map's own
(k_wall_locate), on one 1 M-point frame; tools/wall_arc_timing.py's protocol.

  python tools/wall_alignment_locate_timing.py --kernel --case CASE --order ORDER [--points 1000000] [--frames 8]
        CASE   straight   a plain straight wall map: gm_wall_map_locate_frame (k_wall_locate; runs on any commit that has it)
               arc        mid-arc of an alignment: one arc side
               clothoid   mid-clothoid: one clothoid side
               joint      1 m before the clothoid -> arc joint: two sides
        ORDER  frame      the points ring by ring along the axis, as a spinning sensor delivers them
               random     the same points shuffled
        Blocking frames; after each a locate_frame in DESIGN and one in MAP mode (min_count 1, against the same frame added
        once at its true pose) from a pose 3 cm and 5 mrad off, and locate_result.  The tube's points come from
        gm_wall_alignment_point, a quarter of them drawn and tiled four times (a library call per point).  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_alignment_locate_timing.py --kernel ...
        in a run of its own, then
  python tools/wall_alignment_locate_timing.py --summarize OUT     per kernel and mode: calls, median / min / max per pass"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import api, synth  # noqa: E402

DS, R, ARC_R = 0.25, 2.0, 80.0
LEFT = (0.0, -1.0)
GRID = dict(n_sectors=90, station_length=DS, radius=R)
N_EL = 160   # 40 m per element: mid-element frames see one side
ELEMENTS = [dict(kind="straight", n_stations=N_EL),
            dict(kind="clothoid", n_stations=N_EL, turn=LEFT, curvature=0.0, rate=1.0 / (ARC_R * N_EL * DS)),
            dict(kind="arc", n_stations=N_EL, turn=LEFT, curvature=1.0 / ARC_R)]
CHAINAGE = dict(straight=20.0, clothoid=60.0, arc=100.0, joint=79.0)
KERNELS = (("k_wall_locate_joint", "k_wall_locate_joint"), ("k_wall_locate", "k_wall_locate"))


def frame(rule, s, n, order, seed=1):
    """(cloud float32 [n, 3] in sensor coordinates, pose [3, 4]) of the design tube with 5 mm noise over chainages s +- 4.5."""
    rng = np.random.default_rng(seed)
    P, pu, pv = rule.point([s, s, s], [0.0, 0.0, 0.5 * np.pi], [0.0, 1.0, 1.0])
    u, v = pu - P, pv - P
    a = np.cross(u, v)
    Rm = np.stack([a, np.cross(u, a), u], axis=1)
    tr = P - 0.2 * v - 0.1 * u
    m = n // 4
    sp = np.sort(s + rng.uniform(-4.5, 4.5, m))                      # ring by ring along the axis
    phi = np.mod(np.arange(m) * (2.0 * np.pi / 1024.0), 2.0 * np.pi)  # 1024 points per turn
    x = rule.point(sp, phi, R + rng.normal(0.0, 0.005, m))
    cloud = ((x - tr) @ Rm).astype(np.float32)
    cloud = np.repeat(cloud, 4, axis=0)[:n]
    if order == "random":
        cloud = cloud[rng.permutation(len(cloud))]
    return np.ascontiguousarray(cloud), np.concatenate([Rm, tr.reshape(3, 1)], axis=1)


def kernel(a):
    rule = api.WallAlignmentRule(ELEMENTS, **GRID)
    xyz, pose = frame(rule, CHAINAGE[a.case], a.points, a.order)
    off = np.array(pose)
    off[:, :3] = off[:, :3] @ synth.pose_matrix((0, 0, 0), yaw_deg=0.29, pitch_deg=0.0)[:, :3]
    off[1, 3] += 0.03
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        if a.case == "straight":
            ep = rule.element_params(0)[0]
            vec = ("point", "direction", "up", "forward")
            target = c.wall_map(**{k: (list(getattr(ep, k)) if k in vec else getattr(ep, k))
                                   for k in ("n_stations", "n_sectors", "station_length", "t_min", "gate", "radius") + vec})
        else:
            target = c.wall_alignment(ELEMENTS, **GRID)
        res = c.process_frame(xyz)
        target.add_frame(0, pose)
        target.sync()
        infos = {}
        for _ in range(3 + a.frames):
            res = c.process_frame(xyz)
            for ref in (0, 1):
                target.locate_frame(0, off, reference=ref, min_count=1)
                infos[ref] = target.locate_result(0)
        out = dict(case=a.case, order=a.order, points=len(xyz), n_valid=res["n_valid"], calls=3 + a.frames)
        for ref, i in infos.items():
            out["design" if ref == 0 else "map"] = dict(status=i["status"], used=[q["used"] for q in i["pass"]], gated=[q["gated"] for q in i["pass"]],
                                                         unsurveyed=[q["unsurveyed"] for q in i["pass"]], n_sides=i.get("n_sides", 1))
        print(json.dumps(out))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    by = {}
    for r in rows:
        for key, name in KERNELS:   # (the longer name first)
            if key in r["Kernel_Name"]:
                by.setdefault(name, []).append((float(r["Start_Timestamp"]), (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
                break
    out = {}
    for name, v in by.items():
        v = [t for _, t in sorted(v)]
        v = v[18:] if len(v) > 36 else v      # (the warm-up frames: two locates of three passes each)
        # the launches alternate DESIGN (three passes) and MAP (three passes)
        for mode, first in (("design", 0), ("map", 3)):
            for k in range(3):
                w = v[first + k::6]
                if w:
                    out[f"{name}:{mode}:pass{k}"] = dict(calls=len(w), median_us=round(float(np.median(w)), 2), min_us=round(min(w), 2),
                                                        max_us=round(max(w), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--case", choices=sorted(CHAINAGE), default="joint")
    ap.add_argument("--order", choices=("frame", "random"), default="frame")
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
