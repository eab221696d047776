#!/usr/bin/env python3
"""Cost of a check's objects through a wall alignment (k_wall_object_bin_joint, _reduce_joint, _rows_joint beside the
kernels it shares with the map) next to gm_wall_map_check_objects (k_wall_object_bin, _reduce, _rows) on the same rows; on
one 1 M-point frame in which a strip of the wall lies 0.3 m inside the surveyed tube; tools/wall_alignment_align_timing.py's
frame and protocol.

  python tools/wall_alignment_objects_timing.py --case CASE [--points 1000000] [--calls 8]
        CASE   joint      the frame 1 m before the clothoid -> arc joint: a check of two sides, then
                          gm_wall_alignment_check_objects with object_of_row (the three joint kernels)
               element    the frame in mid-straight: a one-side check, whose rows lie in the element map's buffer; then on
                          the SAME staged rows gm_wall_alignment_check_objects (the joint kernels, one side) and the element
                          map's gm_wall_map_check_objects (the map's kernels), alternated
        One check, 3 warm-up calls and --calls measured ones of ONE sized ABI call each (not the binding, which calls twice);
        prints the wall time of the blocking calls.  Under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_alignment_objects_timing.py --case ...
        in a run of its own per case, then
  python tools/wall_alignment_objects_timing.py --summarize OUT     per k_wall_object_* kernel: calls, median / min / max"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib, api, synth  # noqa: E402
import wall_alignment_align_timing as at  # noqa: E402

WARM = 3
OP = dict(block_stations=2, block_sectors=2)
MAX_OBJECTS = 1 << 15
STRIP = (1.0, 1.6)   # rad
# (the longer names first: a kernel's name is matched by its first entry)
KERNELS = ("k_wall_object_bin_joint", "k_wall_object_reduce_joint", "k_wall_object_rows_joint", "k_wall_object_bin", "k_wall_object_reduce",
           "k_wall_object_rows", "k_wall_object_tiles", "k_wall_object_seams", "k_wall_object_flatten", "k_wall_object_blocks",
           "k_wall_object_select")


def moved(xyz, depth=0.3):
    """The frame with the strip of angles STRIP about the sensor's x axis moved `depth` toward it."""
    r = np.maximum(np.linalg.norm(xyz[:, 1:], axis=1), 1e-3)
    phi = np.mod(np.arctan2(xyz[:, 2], xyz[:, 1]), 2.0 * np.pi)
    k = np.where((phi >= STRIP[0]) & (phi < STRIP[1]), (r - depth) / r, 1.0)[:, None]
    out = xyz.copy()
    out[:, 1:] = (out[:, 1:] * k).astype(np.float32)
    return out


def stats(v):
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def run(a):
    rule = api.WallAlignmentRule(at.ELEMENTS, **at.GRID)
    s = at.S_STRAIGHT if a.case == "element" else at.S_JOINT
    xyz, pose = at.frame(rule, s, a.points, "frame")
    L = _lib.load()
    with g.GeometricMapping(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points) as c:
        al = c.wall_alignment(at.ELEMENTS, **at.GRID)
        c.process_frame(xyz)
        al.add_frame(0, pose)
        al.sync()
        c.process_frame(moved(xyz))
        plan = al.check_frame(0, pose, min_count=1)
        info, rows = al.check_result(0)
        n = len(rows)
        p = api.WallMap.object_params(**OP)
        objs = np.zeros(MAX_OBJECTS, api.WALL_OBJECT)
        of_row = np.zeros(max(n, 1), np.int32)
        op_, rp_ = objs.ctypes.data_as(C.POINTER(_lib.WallObject)), of_row.ctypes.data_as(C.POINTER(C.c_int32))
        ai, mi, got = _lib.WallAlignmentObjectsInfo(), _lib.WallObjectsInfo(), C.c_uint32(0)

        def alignment():
            assert L.gm_wall_alignment_check_objects(al._h(), 0, C.byref(p), C.byref(ai), op_, len(objs), C.byref(got), rp_, n) == 0

        calls = dict(alignment=alignment)
        if a.case == "element":
            m = al.element(plan["element"])

            def element_map():
                assert L.gm_wall_map_check_objects(m._map, 0, C.byref(p), C.byref(mi), op_, len(objs), C.byref(got), rp_, n) == 0
            calls["element_map"] = element_map
        t = {k: [] for k in calls}
        for it in range(WARM + a.calls):
            for k in (list(calls) if it % 2 else list(calls)[::-1]):
                t0 = time.perf_counter()
                calls[k]()
                if it >= WARM:
                    t[k].append((time.perf_counter() - t0) * 1e3)
        out = dict(case=a.case, points=len(xyz), calls=a.calls, n_sides=plan["n_sides"], changed_rows=n, objects=int(ai.objects),
                   components=int(ai.components), window_blocks=int(ai.blocks_stations) * int(ai.blocks_sectors),
                   side_rows=list(ai.side_rows)[:plan["n_sides"]], wall={k: stats(v) for k, v in t.items()})
        if a.case == "element":
            out["map_objects"] = int(mi.objects)
        print(json.dumps(out))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    by = {}
    for r in rows:
        for key in KERNELS:
            if key in r["Kernel_Name"]:
                by.setdefault(key, []).append((float(r["Start_Timestamp"]), (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
                break
    out = {}
    for name, v in by.items():
        v = [x for _, x in sorted(v)]
        v = v[WARM:] if len(v) > WARM else v
        out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--case", choices=("joint", "element"), default="joint")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        run(a)


if __name__ == "__main__":
    main()
