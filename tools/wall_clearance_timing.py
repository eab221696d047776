#!/usr/bin/env python3
"""Cost of gm_wall_map_clearance against gm_wall_map_read of the same window (what a host-side comparison pays first).

  python tools/wall_clearance_timing.py [--reps 15] [--out FILE]
        wall time of one sized call (stations and list), of a count query (the station pass alone) and of the read
        (medians after warm-up, alternated), for a 48-station window of the default map and the whole 4096 x 4096 map
        with ~1 % and with every cell short of the margin, in both references; merged into FILE (default
        profiles/r18_wall_clearance.json) under "wall"
  python tools/wall_clearance_timing.py --table [--out FILE]
        the DESIGN.md table from the json

The byte floor quoted beside the calls: count (4 B) of every cell and min_key (4 B) or sum (8 B) of the usable gauged
ones, once for the stations and once more for the list; 32 B per station and 16 B per list cell written and copied.
GM_WALL_CLEAR_CHUNK=<cells> in the environment changes the list's chunk (default 2^20 cells)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib  # noqa: E402
from geometric_mapping_amd.api import RAW_CELL, WALL_CLEARANCE_CELL, WALL_CLEARANCE_STATION  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r18_wall_clearance.json")
CELL = np.dtype([("count", "<u4"), ("mean", "<f4"), ("min", "<f4"), ("max", "<f4")])   # gm_surface_cell
# (name, n_stations, n_sectors, station0, n)
WINDOWS = (("48_stations", 4000, 90, 1976, 48), ("4096x4096", 4096, 4096, 0, 4096))
# (name, margin): the wall stands 0.10 m .. 0.30 m clear of the gauge, 1 % of the cells 0.05 m inside it
LISTS = (("1pct_listed", 0.05), ("all_listed", 0.5))
REFERENCES = (("min", _lib.GM_WALL_CLEAR_MIN), ("mean", _lib.GM_WALL_CLEAR_MEAN))


def ordered(e):
    b = np.asarray(e, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def field(n, ns, seed=1):
    """Raw cells holding 8-47 points each, every cell: means of 0 .. 0.2 m outside the design, 1 % of them 0.15 m inside."""
    rng = np.random.default_rng(seed)
    count = rng.integers(8, 48, (n, ns))
    mean = rng.uniform(0.0, 0.2, (n, ns))
    mean[rng.random((n, ns)) < 0.01] = -0.15
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = np.rint(mean * 2.0 ** 20).astype(np.int64) * count
    raw["min_key"] = ~ordered(mean - 0.005)
    raw["max_key"] = ordered(mean + 0.005)
    return raw


def merge(path, key, value):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def wall(a):
    out = {}
    i32p = C.POINTER(C.c_int32)
    with g.GeometricMapping() as c:
        for name, n, ns, s0, w in WINDOWS:
            m = c.wall_map(n_stations=n, n_sectors=ns)   # radius 2
            m.add_raw(field(n, ns))
            gauge = np.full(ns, int(round(1.9 * 2 ** 20)), np.int32)
            gauge[: ns // 10] = 0                        # the invert is not gauged
            gp = gauge.ctypes.data_as(i32p)
            for lname, margin in LISTS:
                for rname, ref in REFERENCES:
                    p = m.clearance_params(reference=ref, margin=margin)
                    info, got = _lib.WallClearanceInfo(), C.c_uint64(0)

                    def query():
                        c._check(c._L.gm_wall_map_clearance(m._h(), s0, w, gp, 1, None, C.byref(p), C.byref(info), None, 0, None, 0,
                                                            C.byref(got)))
                    query()
                    st = np.zeros(w, WALL_CLEARANCE_STATION)
                    cells = np.zeros(max(got.value, 1), WALL_CLEARANCE_CELL)

                    def call():
                        c._check(c._L.gm_wall_map_clearance(
                            m._h(), s0, w, gp, 1, None, C.byref(p), C.byref(info), st.ctypes.data_as(C.POINTER(_lib.WallClearanceStation)),
                            w, cells.ctypes.data_as(C.POINTER(_lib.WallClearanceCell)), len(cells), C.byref(got)))
                    rbuf, rgot = np.empty(w * ns, CELL), C.c_uint64(0)

                    def read():   # the C call into a buffer that is there already, as the two calls above
                        c._check(c._L.gm_wall_map_read(m._h(), s0, w, rbuf.ctypes.data_as(C.POINTER(_lib.SurfaceCell)), len(rbuf),
                                                       C.byref(rgot)))
                    t = {"call": [], "query": [], "read": []}
                    fns = {"call": call, "query": query, "read": read}
                    for rep in range(a.reps + 2):
                        for k, fn in fns.items():
                            t0 = time.perf_counter()
                            fn()
                            dt = (time.perf_counter() - t0) * 1e3
                            if rep >= 2:
                                t[k].append(dt)
                    row = {k + "_ms": med(v) for k, v in t.items()}
                    row.update(cells=w * ns, listed=int(got.value), reps=a.reps,
                               ratio_to_read=round(row["call_ms"] / row["read_ms"], 3))
                    out[f"{name}/{lname}/{rname}"] = row
                    print(f"{name}/{lname}/{rname}", row, flush=True)
            m.close()
    merge(a.out, "wall", out)


def table(a):
    data = json.load(open(a.out))["wall"]
    print("| window / list / reference | cells | listed | call ms | count query ms | gm_wall_map_read ms | call / read |")
    print("|---|---|---|---|---|---|---|")
    for k, r in data.items():
        print(f"| {k} | {r['cells']} | {r['listed']} | {r['call_ms']} | {r['query_ms']} | {r['read_ms']} | {r['ratio_to_read']} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    table(a) if a.table else wall(a)
