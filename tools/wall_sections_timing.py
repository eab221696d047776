#!/usr/bin/env python3
"""Cost of gm_wall_map_sections against gm_wall_map_read of the same window (what a host-side fit pays first).

  python tools/wall_sections_timing.py [--reps 15]   wall time of one call (records and sums) and of the read (medians
                                                      after warm-up, alternated) for 48 x 90, 4000 x 90 and 4096 x 4096
                                                      cells with S = 4 and the defaults; merged into
                                                      profiles/r19_wall_sections.json under "wall"
  python tools/wall_sections_timing.py --kernel       a few calls per window and nothing else: run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_sections_timing.py --kernel
                                                      in a run of its own, then
  python tools/wall_sections_timing.py --summarize OUT   k_wall_sections per launch of a call (the fitting passes, then
                                                      the evaluation), medians over the calls, merged under "kernels_us"
  python tools/wall_sections_timing.py --table        the DESIGN.md tables from the json

The split of the call: kernel (the trace) and what is left, the host side: the solves, the copies of the models and the
records between the launches and the waits for them.  The solves are not timed on their own: a ctypes loop over
gm_wall_section_solve costs more per call than the solve does."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib  # noqa: E402
from geometric_mapping_amd.api import RAW_CELL, WALL_SECTION, WALL_SECTION_SUMS  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r19_wall_sections.json")
CELL = np.dtype([("count", "<u4"), ("mean", "<f4"), ("min", "<f4"), ("max", "<f4")])   # gm_surface_cell
# (name, n_stations, n_sectors, station0, n)
WINDOWS = (("48x90", 4000, 90, 1976, 48), ("4000x90", 4000, 90, 0, 4000), ("4096x4096", 4096, 4096, 0, 4096))
KERNEL_CALLS = 6


def field(n, ns, seed=1):
    """Raw cells holding 8-47 points each: a tube closed by 8 mm, 5 mm off the axis, 4 mm oval, 2 mm of noise, and 1 % of
    the cells 0.3 m outside (niches, which the passes reject)."""
    rng = np.random.default_rng(seed)
    phi = 2 * np.pi * (np.arange(ns) + 0.5) / ns
    mean = -0.008 + 0.003 * np.cos(phi) - 0.004 * np.sin(phi) + 0.004 * np.cos(2 * phi) + rng.normal(0.0, 0.002, (n, ns))
    mean[rng.random((n, ns)) < 0.01] += 0.3
    count = rng.integers(8, 48, (n, ns))
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = np.rint(mean * 2.0 ** 20).astype(np.int64) * count
    return raw


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def caller(c, m, s0, w):
    p = m.section_params()
    ns_ = (w + 3) // 4
    rec, sums = np.zeros(ns_, WALL_SECTION), np.zeros(ns_, WALL_SECTION_SUMS)
    info, got = _lib.WallSectionsInfo(), C.c_uint32(0)

    def call():
        c._check(c._L.gm_wall_map_sections(m._h(), None, s0, w, C.byref(p), C.byref(info), rec.ctypes.data_as(C.POINTER(_lib.WallSection)),
                                           ns_, C.byref(got), sums.ctypes.data_as(C.POINTER(_lib.WallSectionSums))))
    return call, info, rec, sums


def wall(a):
    out = {}
    with g.GeometricMapping() as c:
        L = c._L
        for name, n, ns, s0, w in WINDOWS:
            m = c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns))
            call, info, rec, sums = caller(c, m, s0, w)
            rbuf, rgot = np.empty(w * ns, CELL), C.c_uint64(0)

            def read():   # the C call into a buffer that is there already, as the call above
                c._check(L.gm_wall_map_read(m._h(), s0, w, rbuf.ctypes.data_as(C.POINTER(_lib.SurfaceCell)), len(rbuf), C.byref(rgot)))
            t = {"call": [], "read": []}
            fns = {"call": call, "read": read}
            for rep in range(a.reps + 2):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= 2:
                        t[k].append(dt)
            row = {k + "_ms": med(v) for k, v in t.items()}
            row.update(cells=w * ns, sections=int(info.sections), ok=int(info.sections_ok), rejected=int(info.rejected), reps=a.reps,
                       ratio_to_read=round(row["call_ms"] / row["read_ms"], 3))
            out[name] = row
            print(name, row, flush=True)
            m.close()
    merge("wall", out)


def kernel(a):
    with g.GeometricMapping() as c:
        for name, n, ns, s0, w in WINDOWS:
            m = c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns))
            call, info, _, _ = caller(c, m, s0, w)
            for _ in range(KERNEL_CALLS):
                call()
            print(name, info.sections_ok, flush=True)
            m.close()


def summarize(d):
    """The trace holds KERNEL_CALLS x (passes + 1) launches of k_wall_sections per window, in window order."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for p in f for r in csv.DictReader(open(p))), key=lambda r: float(r["Start_Timestamp"]))
    v = [(float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3 for r in rows if "k_wall_sections" in r["Kernel_Name"]]
    per = len(v) // len(WINDOWS)
    launches = per // KERNEL_CALLS
    out = {}
    for i, (name, *_rest) in enumerate(WINDOWS):
        calls = np.array(v[i * per:(i + 1) * per]).reshape(KERNEL_CALLS, launches)[2:]   # (the first two calls: warm-up)
        out[name] = {"per_launch": [round(float(x), 2) for x in np.median(calls, axis=0)],
                     "sum": round(float(np.median(calls.sum(axis=1))), 2)}
    merge("kernels_us", out)
    print(json.dumps(out))


def table():
    data = json.load(open(OUT))
    ks = data.get("kernels_us", {})
    print("| window | sections | call ms | `gm_wall_map_read` ms | call / read | kernel ms | host solves, copies and waits ms |")
    print("|---|---|---|---|---|---|---|")
    for name, r in data.get("wall", {}).items():
        k = ks[name]["sum"] / 1e3 if name in ks else None
        rest = round(r["call_ms"] - k, 3) if k is not None else "not measured"
        print(f"| {name} | {r['sections']} | {r['call_ms']} | {r['read_ms']} | {r['ratio_to_read']} | "
              f"{round(k, 3) if k is not None else 'not measured'} | {rest} |")
    print("\n| window | " + " | ".join(f"pass {i + 1}" for i in range(3)) + " | evaluation | sum |")
    print("|---|---|---|---|---|---|")
    for name, r in ks.items():
        print(f"| {name} | " + " | ".join(f"{x}" for x in r["per_launch"]) + f" | {r['sum']} µs |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.table:
        table()
    elif a.kernel:
        kernel(a)
    else:
        wall(a)


if __name__ == "__main__":
    main()
