#!/usr/bin/env python3
"""Where gm_wall_map_quantities stands beside the three calls that read the same windows: gm_wall_map_read (what a
host-side reduction pays first), gm_wall_map_clearance (station records only: one pass of one wave per row over count
and sum or min_key) and gm_wall_map_sections (the same column merge, launched passes + 1 times).

  python tools/wall_quantities_timing.py [--reps 9] [--out FILE]
      wall time of one sized call of each (medians after two warm-up rounds, alternated in one process) for a 48-station
      window and the whole 2^24-cell map at 90 and at 4096 sectors, with S = 1 and 4, without and with a baseline; the
      rows go to profiles/r23_wall_quantities.json (or FILE) under "wall"
  python tools/wall_quantities_timing.py --table [--out FILE]   the DESIGN.md table from the json

Wall times of blocking calls: each ends in a device synchronise and includes its copies to the host.  The bytes a call's
kernels read from the table are computed from the shapes (12 B per cell for count and sum, 24 B with a baseline; the
clearance's station pass in the MEAN reference reads the same 12 B)."""
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
from geometric_mapping_amd.api import RAW_CELL, WALL_CLEARANCE_STATION, WALL_QUANTITY, WALL_SECTION  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r23_wall_quantities.json")
CELL = np.dtype([("count", "<u4"), ("mean", "<f4"), ("min", "<f4"), ("max", "<f4")])   # gm_surface_cell
# (n_stations, n_sectors) of the two 2^24-cell maps; each is timed on a 48-station window in its middle and as a whole
MAPS = ((2 ** 24 // 90, 90), (4096, 4096))
N_ZONES = 3


def field(n, ns, seed, offset=0.12):
    """Raw cells holding 8-47 points each: a tube excavated `offset` outside the design with 2 cm of roughness, 1 % of the
    cells in pockets 0.4 m further out and 1 % 0.15 m inside the design."""
    rng = np.random.default_rng(seed)
    mean = rng.normal(offset, 0.02, (n, ns)).astype(np.float32)
    u = rng.random((n, ns), dtype=np.float32)
    mean[u < 0.01] += 0.4
    mean[u > 0.99] = -0.15
    count = rng.integers(8, 48, (n, ns), dtype=np.int64)
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = np.rint(mean.astype(np.float64) * 2.0 ** 20).astype(np.int64) * count
    return raw


def med(v):
    return round(float(np.median(v)), 4)


def callers(c, m, base, ns, s0, w, S):
    """The four sized C calls on window [s0, s0 + w) into buffers that are there already."""
    L, h = c._L, m._h()
    i32 = C.POINTER(C.c_int32)
    NS = (w + S - 1) // S
    lo, hi = np.full(ns, 104858, np.int32), np.full(ns, 262144, np.int32)       # 0.10 m and 0.25 m outside the design
    zone = np.repeat(np.arange(N_ZONES, dtype=np.uint8), (ns + N_ZONES - 1) // N_ZONES)[:ns].copy()
    qp = m.quantity_params(section_stations=S)
    qrec, qinfo, qgot = np.zeros(NS * N_ZONES, WALL_QUANTITY), _lib.WallQuantitiesInfo(), C.c_uint32(0)
    bh = base._h() if base is not None else None

    def quantities():
        c._check(L.gm_wall_map_quantities(h, bh, s0, w, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32), 1, None,
                                          zone.ctypes.data_as(C.POINTER(C.c_uint8)), N_ZONES, C.byref(qp), C.byref(qinfo),
                                          qrec.ctypes.data_as(C.POINTER(_lib.WallQuantity)), len(qrec), C.byref(qgot), None))
    rbuf, rgot = np.empty(w * ns, CELL), C.c_uint64(0)

    def read():
        c._check(L.gm_wall_map_read(h, s0, w, rbuf.ctypes.data_as(C.POINTER(_lib.SurfaceCell)), len(rbuf), C.byref(rgot)))
    gauge = np.full(ns, (2 << 20) - 104858, np.int32)
    cp = m.clearance_params(reference=_lib.GM_WALL_CLEAR_MEAN)
    cst, cinfo, cgot = np.zeros(w, WALL_CLEARANCE_STATION), _lib.WallClearanceInfo(), C.c_uint64(0)

    def clearance():   # station records only: no list
        c._check(L.gm_wall_map_clearance(h, s0, w, gauge.ctypes.data_as(i32), 1, None, C.byref(cp), C.byref(cinfo),
                                         cst.ctypes.data_as(C.POINTER(_lib.WallClearanceStation)), w, None, 0, C.byref(cgot)))
    sp = m.section_params(section_stations=S)
    srec, sinfo, sgot = np.zeros(NS, WALL_SECTION), _lib.WallSectionsInfo(), C.c_uint32(0)

    def sections():
        c._check(L.gm_wall_map_sections(h, bh, s0, w, C.byref(sp), C.byref(sinfo), srec.ctypes.data_as(C.POINTER(_lib.WallSection)), NS,
                                        C.byref(sgot), None))
    return {"quantities": quantities, "read": read, "clearance_stations": clearance, "sections": sections}, qinfo


def wall(a):
    rows = []
    with g.GeometricMapping() as c:
        for n, ns in MAPS:
            m, base = c.wall_map(n_stations=n, n_sectors=ns), c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns, 1))
            base.add_raw(field(n, ns, 2, 0.20))
            for s0, w in ((n // 2 - 24, 48), (0, n)):
                for S in (1, 4):
                    for b in (None, base):
                        fns, qinfo = callers(c, m, b, ns, s0, w, S)
                        if b is not None:          # (read and the clearance take no baseline: timed once per window)
                            fns = {k: fns[k] for k in ("quantities", "sections")}
                        t = {k: [] for k in fns}
                        for rep in range(a.reps + 2):
                            for k, fn in fns.items():
                                t0 = time.perf_counter()
                                fn()
                                dt = (time.perf_counter() - t0) * 1e3
                                if rep >= 2:
                                    t[k].append(dt)
                        row = {"window": f"{w}x{ns}", "S": S, "baseline": b is not None, "cells": w * ns,
                               "sections": int(qinfo.sections), "under": int(qinfo.under), "over": int(qinfo.over),
                               "table_bytes": w * ns * (24 if b is not None else 12), "reps": a.reps}
                        row.update({k + "_ms": med(v) for k, v in t.items()})
                        rows.append(row)
                        print(row, flush=True)
            m.close()
            base.close()
    with open(a.out, "w") as f:
        json.dump({"wall": rows}, f, indent=1, sort_keys=True)
        f.write("\n")


def table(a):
    rows = json.load(open(a.out))["wall"]
    print("| window | S | baseline | sections | `quantities` ms | `read` ms | `clearance` (stations) ms | `sections` ms | "
          "quantities / clearance | bytes ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    stations = {}
    for r in rows:
        if "clearance_stations_ms" in r:
            stations[(r["window"], r["S"])] = (r["clearance_stations_ms"], r["read_ms"])
        cl, rd = stations[(r["window"], r["S"])]
        print(f"| {r['window']} | {r['S']} | {'yes' if r['baseline'] else 'no'} | {r['sections']} | {r['quantities_ms']} | {rd} | {cl} | "
              f"{r['sections_ms']} | {round(r['quantities_ms'] / cl, 2)} | {2 if r['baseline'] else 1} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    if a.table:
        table(a)
    else:
        wall(a)


if __name__ == "__main__":
    main()
