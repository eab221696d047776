#!/usr/bin/env python3
"""Cost of the align through a wall alignment (k_wall_align_bin_joint, k_wall_align_values_joint, k_wall_align_score) beside
the same three launches on a straight map (k_wall_align_bin, k_wall_align_values, k_wall_align_score) and beside what a
caller had before it: the two element maps' own aligns, which refuse a curved map; on one 1 M-point frame 1 m before the
clothoid -> arc joint; tools/wall_alignment_check_timing.py's protocol.

  python tools/wall_alignment_align_timing.py --kernel --case CASE --order ORDER [--points 1000000] [--frames 8]
        CASE   joint      gm_wall_alignment_align_frame 1 m before the clothoid -> arc joint (two sides, two pieces)
               straight   gm_wall_alignment_align_frame in mid-straight, the image inside the element: the element map's own
                          align (k_wall_align_bin, k_wall_align_values, k_wall_align_score)
               elements   gm_wall_map_align_frame on the clothoid's and on the arc's element map at the joint: the status of
                          each (GM_ERR_UNSUPPORTED: nothing is launched)
        ORDER  frame      the points ring by ring along the axis, as a spinning sensor delivers them
               random     the same points shuffled
        Blocking frames, 3 warm-ups and --frames measured ones; the survey is the same frame added once at its pose; the
        align runs under a pose one station short (P 18, A 8, B 4, min_count 1, min_frame_count 1).  The tube's points come
        from gm_wall_alignment_point, a quarter of them drawn and repeated four times (a library call per point).  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_alignment_align_timing.py --kernel ...
        in a run of its own per case and order, then
  python tools/wall_alignment_align_timing.py --summarize OUT     per kernel: calls, median / min / max of the measured frames"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib, api, synth  # noqa: E402

DS, R, ARC_R = 0.25, 2.0, 80.0
LEFT = (0.0, -1.0)
GRID = dict(n_sectors=90, station_length=DS, radius=R)
N_EL = 160   # 40 m per element
ELEMENTS = [dict(kind="straight", n_stations=N_EL),
            dict(kind="clothoid", n_stations=N_EL, turn=LEFT, curvature=0.0, rate=1.0 / (ARC_R * N_EL * DS)),
            dict(kind="arc", n_stations=N_EL, turn=LEFT, curvature=1.0 / ARC_R)]
S_JOINT = 79.0   # 1 m before the clothoid -> arc joint
S_STRAIGHT = 20.0   # mid-straight
AP = dict(half_patch_stations=18, max_station_shift=8, max_sector_shift=4, min_count=1, min_frame_count=1)
WARM = 3
# (the longer names first: a kernel's name is matched by its first entry)
KERNELS = ("k_wall_align_bin_joint", "k_wall_align_values_joint", "k_wall_align_bin", "k_wall_align_values", "k_wall_align_score")


def frame(rule, s, n, order, seed=1):
    """(cloud float32 [n, 3] in sensor coordinates, pose [3, 4]) of the design tube with 5 mm noise over chainages s +- 4.5;
    a relief of 3 cm that no two stations share."""
    rng = np.random.default_rng(seed)
    P, pu, pv = rule.point([s, s, s], [0.0, 0.0, 0.5 * np.pi], [0.0, 1.0, 1.0])
    u, v = pu - P, pv - P
    a = np.cross(u, v)
    Rm = np.stack([a, np.cross(u, a), u], axis=1)
    tr = P - 0.2 * v - 0.1 * u
    m = n // 4
    sp = np.sort(s + rng.uniform(-4.5, 4.5, m))                      # ring by ring along the axis
    phi = np.mod(np.arange(m) * (2.0 * np.pi / 1024.0), 2.0 * np.pi)  # 1024 points per turn
    rho = R + rng.normal(0.0, 0.005, m) + 0.03 * np.sin(2.3 * sp + 0.7 * np.sin(1.1 * sp)) * np.cos(3.0 * phi + 0.9 * sp)
    x = rule.point(sp, phi, rho)
    cloud = ((x - tr) @ Rm).astype(np.float32)
    cloud = np.repeat(cloud, 4, axis=0)[:n]
    if order == "random":
        cloud = cloud[rng.permutation(len(cloud))]
    return np.ascontiguousarray(cloud), np.concatenate([Rm, tr.reshape(3, 1)], axis=1)


def kernel(a):
    rule = api.WallAlignmentRule(ELEMENTS, **GRID)
    s = S_STRAIGHT if a.case == "straight" else S_JOINT
    xyz, pose = frame(rule, s, a.points, a.order)
    _, short = frame(rule, s - DS, 4, a.order)   # the caller's pose: one station short
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        al = c.wall_alignment(ELEMENTS, **GRID)
        res = c.process_frame(xyz)
        al.add_frame(0, pose)
        al.sync()
        out = dict(case=a.case, order=a.order, points=len(xyz), calls=WARM + a.frames)
        for _ in range(WARM + a.frames):
            res = c.process_frame(xyz)
            if a.case == "elements":
                status = []
                for i in (1, 2):
                    try:
                        al.element(i).align_frame(0, short, **AP)
                        status.append(_lib.GM_OK)
                    except _lib.GmError as e:
                        status.append(e.status)
                out.update(status=status, unsupported=_lib.GM_ERR_UNSUPPORTED)
            else:
                plan = al.align_frame(0, short, **AP)
                info, _ = al.align_result(0)
                out.update(n_sides=plan["add"]["n_sides"], own=plan["own"], pieces=plan["n_pieces"], best=[info["best_station"], info["best_sector"]],
                           status=info["status"], side_class=info["side_class"].tolist(), overlap=info["overlap"])
            al.sync()
        out["n_valid"] = res["n_valid"]
        print(json.dumps(out))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    by = {}
    for r in rows:
        for key in KERNELS:
            if key in r["Kernel_Name"]:
                by.setdefault(key, []).append((float(r["Start_Timestamp"]),
                                                               (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
                break
    out = {}
    for name, v in by.items():
        v = [t for _, t in sorted(v)]
        v = v[WARM:] if len(v) > WARM else v
        if not v:
            continue
        out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--case", choices=("joint", "straight", "elements"), default="joint")
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
