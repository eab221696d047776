#!/usr/bin/env python3
"""Cost of a check's objects (gm_wall_map_check_objects) on the 1 M-point tunnel frame, beside the path it replaces.

Two cases: the frame checked against the survey of the same wall (`low`: a few per cent of the points changed, the patches) and against
the same survey moved by 0.3 m with a threshold of one unit (`all`: every usable point changed).

  python tools/wall_objects_timing.py [--points 1000000] [--calls 30]
        per case, alternated in one process: the wall time of the blocking object call (ONE sized ABI call, the record
        buffer large enough -- not the Python binding, which calls twice), of the same call with object_of_row, and of
        gm_wall_map_get_check of all rows; then the path the call replaces: those rows are handed to
        host/gm_wall_objects_test --time (the host mirror's scalar C++ restatement, no device) and its median is added to
        get_check's: `replaced_path_ms`, beside `objects.median_ms`, with `device_wins`.
  python tools/wall_objects_timing.py --kernel --case low|all [--points N] [--calls 8]
        per iteration one frame, one check of that case and one sized object call, for
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_objects_timing.py --kernel --case low
        in a run of its own per case, then
  python tools/wall_objects_timing.py --summarize OUT
        from that trace: the median of every k_wall_object_* kernel, the median over the calls of their summed device time
        (`objects_sum_us`) and the median of that frame's check kernel beside it"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib, api, synth  # noqa: E402

IDENT = np.eye(4)[:3]
NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel sits around chainage 0
WARMUP = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTATE = os.path.join(ROOT, "host", "gm_wall_objects_test")
OP = dict(block_stations=2, block_sectors=2)
MAX_OBJECTS = 1 << 15   # above 2 planes x 128 x 45 window blocks of the default map under OP
CASES = (("low", dict(min_count=1)), ("all", dict(min_count=1, threshold=2.0 ** -20, gate=0.25)))


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def maps(c, xyz):
    survey, moved = c.wall_map(**NOMINAL), c.wall_map(**NOMINAL)
    c.process_frame(xyz)
    for _ in range(4):
        survey.add_frame(0, IDENT)
    survey.sync()
    raw = survey.read_raw()
    raw["sum"] += raw["count"].astype(np.int64) * int(0.3 * 2 ** 20)
    moved.add_raw(raw)
    return dict(low=survey, all=moved)


def restatement(rec, m, anchor, p, reps=5):
    """The host mirror's scalar C++ restatement on the rows of get_check (host/gm_wall_objects_test --time): wall times."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rows.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<qIIII", int(anchor), m.n_stations, m.n_sectors, len(rec), reps) + bytes(p) + rec.tobytes())
        r = subprocess.run([RESTATE, "--time", path], check=True, capture_output=True, text=True)
    got = json.loads(r.stdout.strip().splitlines()[-1])
    out = stats(got["restate_ms"])
    out.update(objects=got["objects"], components=got["components"])
    return out


def blocking(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    L = _lib.load()
    out = dict(points=a.points, calls=a.calls)
    with g.GeometricMapping(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points) as c:
        ms = maps(c, xyz)
        for name, ck in CASES:
            m = ms[name]
            c.process_frame(xyz)
            add = m.check_frame(0, IDENT, **ck)
            info, rec = m.check_result(0)
            n = len(rec)
            p = m.object_params(**OP)
            oinfo, got = _lib.WallObjectsInfo(), C.c_uint32(0)
            objs = np.zeros(MAX_OBJECTS, api.WALL_OBJECT)
            of_row = np.zeros(max(n, 1), np.int32)
            rows = np.zeros(max(n, 1), api.WALL_CHECK_POINT)
            op_, rp_ = objs.ctypes.data_as(C.POINTER(_lib.WallObject)), of_row.ctypes.data_as(C.POINTER(C.c_int32))
            kp_ = rows.ctypes.data_as(C.POINTER(_lib.WallCheckPoint))

            def objects():
                assert L.gm_wall_map_check_objects(m._map, 0, C.byref(p), C.byref(oinfo), op_, len(objs), C.byref(got), None, 0) == 0

            def objects_rows():
                assert L.gm_wall_map_check_objects(m._map, 0, C.byref(p), C.byref(oinfo), op_, len(objs), C.byref(got), rp_, n) == 0

            def get_check():
                assert L.gm_wall_map_get_check(m._map, 0, None, kp_, len(rows), C.byref(got)) == 0

            calls = dict(objects=objects, objects_with_rows=objects_rows, get_check=get_check)
            t = {k: [] for k in calls}
            for it in range(WARMUP + a.calls):
                for k in (list(calls) if it % 2 else list(calls)[::-1]):
                    t0 = time.perf_counter()
                    calls[k]()
                    if it >= WARMUP:
                        t[k].append((time.perf_counter() - t0) * 1e3)
            case = {k: stats(v) for k, v in t.items()}
            case.update(changed_rows=n, n_points=info["n_points"], n_objects=int(oinfo.objects), n_components=int(oinfo.components),
                        window_blocks=int(oinfo.blocks_stations) * int(oinfo.blocks_sectors), row_bytes=32 * n)
            case["restatement"] = restatement(rec, m, add["anchor_station"], p)
            case["replaced_path_ms"] = case["get_check"]["median_ms"] + case["restatement"]["median_ms"]
            case["device_wins"] = case["objects"]["median_ms"] < case["replaced_path_ms"]
            out[name] = case
    print(json.dumps(out))


def kernel(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    L = _lib.load()
    ck = dict(CASES)[a.case]
    with g.GeometricMapping(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points) as c:
        m = maps(c, xyz)[a.case]
        p = m.object_params(**OP)
        oinfo, got = _lib.WallObjectsInfo(), C.c_uint32(0)
        objs = np.zeros(MAX_OBJECTS, api.WALL_OBJECT)
        for _ in range(WARMUP + a.calls):
            c.process_frame(xyz)
            m.check_frame(0, IDENT, **ck)
            assert L.gm_wall_map_check_objects(m._map, 0, C.byref(p), C.byref(oinfo), objs.ctypes.data_as(C.POINTER(_lib.WallObject)),
                                               len(objs), C.byref(got), None, 0) == 0
        print(json.dumps(dict(case=a.case, points=len(xyz), calls=WARMUP + a.calls, changed_rows=int(oinfo.n_rows),
                              objects=int(oinfo.objects), components=int(oinfo.components))))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: float(r["Start_Timestamp"]))
    calls = []   # per check: [check us, {object kernel: us}] -- the object call's launches follow their check's
    for r in rows:
        name = r["Kernel_Name"]
        us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        if "WallCheckPred" in name:
            calls.append([us, {}])
        elif "k_wall_object_" in name and calls:
            k = name.split("(")[0].split("::")[-1]
            calls[-1][1][k] = calls[-1][1].get(k, 0.0) + us
    calls = calls[WARMUP:] if len(calls) > 2 * WARMUP else calls
    out = dict(calls=len(calls))
    if calls:
        med = lambda v: round(float(np.median(v)), 2)  # noqa: E731
        out["k_wall_check_us"] = med([c_[0] for c_ in calls])
        out["objects_sum_us"] = med([sum(c_[1].values()) for c_ in calls])
        out["kernels_us"] = {k: med([c_[1][k] for c_ in calls if k in c_[1]]) for k in sorted({k for c_ in calls for k in c_[1]})}
        out["ratio_to_check"] = round(out["objects_sum_us"] / out["k_wall_check_us"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--case", choices=("low", "all"), default="low")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernel:
        kernel(a)
    else:
        blocking(a)


if __name__ == "__main__":
    main()
