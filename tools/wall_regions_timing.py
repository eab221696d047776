#!/usr/bin/env python3
"""Cost of gm_wall_map_regions against gm_wall_map_read of the same window (the least any host-side labelling pays).

  python tools/wall_regions_timing.py [--reps 25]     wall time of one call with the list, of a count query and of the read
                                                      (medians after warm-up, alternated), for
                                                      windows of 48 and 4000 stations of the default map and the full
                                                      4096 x 4096 map, at ~1 % flagged in patches and 45 % random;
                                                      merged into profiles/r09_wall_regions.json under "wall"
  python tools/wall_regions_timing.py --kernel [--case NAME]
                                                      a few calls per case and nothing else: run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_regions_timing.py --kernel
                                                      in a run of its own, then
  python tools/wall_regions_timing.py --summarize OUT per-kernel medians of the trace, merged under "kernels_us"
  python tools/wall_regions_timing.py --table         the DESIGN.md tables from the json

GM_WALL_REGION_TILE=<stations>x<sectors> in the environment changes the labelling tile (default 64x64)."""
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
from geometric_mapping_amd.api import RAW_CELL, REGION  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r09_wall_regions.json")
T = int(np.rint(0.05 * 2.0 ** 20))
# (name, n_stations, n_sectors, station0, n)
WINDOWS = (("48_stations", 4000, 90, 1976, 48), ("4000_stations", 4000, 90, 0, 4000), ("4096x4096", 4096, 4096, 0, 4096))
KERNEL_CALLS = 6


def field(n, ns, kind, seed=1):
    """Raw cells: every cell holds 8-47 points; "patches": ~1 % of the cells flagged in 8 x 6 patches of either sign;
    "random": 45 % flagged, the sign drawn per block of 11 x 13 cells."""
    rng = np.random.default_rng(seed)
    count = rng.integers(8, 48, (n, ns))
    q = rng.integers(-T + 1, T, (n, ns))
    if kind == "patches":
        sg = np.zeros((n, ns), np.int64)
        for _ in range(max(1, n * ns // 4800)):
            j, k = rng.integers(0, n), rng.integers(0, ns)
            sg[j:j + 8, np.arange(k, k + 6) % ns] = rng.choice(np.array([-1, 1]))
    else:
        blocks = rng.choice(np.array([-1, 1]), (-(-n // 11), -(-ns // 13)))
        sg = np.where(rng.random((n, ns)) < 0.45, np.repeat(np.repeat(blocks, 11, axis=0), 13, axis=1)[:n, :ns], 0)
    q = np.where(sg != 0, sg * rng.integers(T, 3 * T, (n, ns)), q)
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = q * count
    return raw


def cases():
    for name, n, ns, s0, w in WINDOWS:
        for kind in ("patches", "random"):
            yield f"{name}/{kind}", n, ns, s0, w, kind


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def wall(a):
    out = {}
    with g.GeometricMapping() as c:
        for name, n, ns, s0, w, kind in cases():
            m = c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns, kind))
            p = m.region_params(min_cells=1)
            info, got = _lib.WallRegionsInfo(), C.c_uint32(0)
            buf = None

            def call():   # one call into a buffer that is large enough (sized by the first count query)
                nonlocal buf
                if buf is None:
                    c._check(c._L.gm_wall_map_regions(m._h(), None, s0, w, C.byref(p), C.byref(info), None, 0, C.byref(got), None))
                    buf = np.zeros(max(got.value, 1), dtype=REGION)
                c._check(c._L.gm_wall_map_regions(m._h(), None, s0, w, C.byref(p), C.byref(info),
                                                  buf.ctypes.data_as(C.POINTER(_lib.WallRegion)), len(buf), C.byref(got), None))

            def count_only():
                c._check(c._L.gm_wall_map_regions(m._h(), None, s0, w, C.byref(p), C.byref(info), None, 0, C.byref(got), None))

            t = {"list": [], "count": [], "read": []}
            for f, key in ((call, "list"), (count_only, "count"), (lambda: m.read(s0, w), "read")):
                for _ in range(3):
                    f()
            for _ in range(a.reps):   # alternated, so that drift hits all three alike
                for f, key in ((call, "list"), (count_only, "count"), (lambda: m.read(s0, w), "read")):
                    t0 = time.perf_counter()
                    f()
                    t[key].append((time.perf_counter() - t0) * 1e3)
            out[name] = dict(cells=w * ns, flagged=int(info.flagged_pos + info.flagged_neg), components=int(info.components),
                             regions=int(info.regions), regions_list_ms=med(t["list"]), regions_count_ms=med(t["count"]),
                             read_ms=med(t["read"]), ratio_count_to_read=round(med(t["count"]) / med(t["read"]), 3),
                             ratio_list_to_read=round(med(t["list"]) / med(t["read"]), 3), reps=a.reps)
            print(name, json.dumps(out[name]), flush=True)
            m.close()
    merge("wall", out)


def kernel(a):
    with g.GeometricMapping() as c:
        for name, n, ns, s0, w, kind in cases():
            if a.case and a.case != name:
                continue
            m = c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns, kind))
            for _ in range(KERNEL_CALLS):
                info = m.regions(s0, w, min_cells=1)[0]
            print(name, info["components"], flush=True)
            m.close()


def summarize(d):
    """The trace holds KERNEL_CALLS x 2 launches (count query + list) of every kernel per case, in case order."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for p in f for r in csv.DictReader(open(p))), key=lambda r: float(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if "k_wall_region" in name:
            by.setdefault(name, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    names = [c[0] for c in cases()]
    out = {}
    for name, v in by.items():
        per = len(v) // len(names)
        for i, case in enumerate(names):
            chunk = v[i * per:(i + 1) * per][2:]   # (the first call pair: warm-up)
            out.setdefault(case, {})[name] = round(float(np.median(chunk)), 2)
    merge("kernels_us", out)
    print(json.dumps(out))


def table():
    data = json.load(open(OUT))
    print("| window / flags | cells | components | count query | call with list | `gm_wall_map_read` | count / read | list / read |")
    print("|---|---|---|---|---|---|---|---|")
    for name, r in data.get("wall", {}).items():
        print(f"| {name} | {r['cells']} | {r['components']} | {r['regions_count_ms']} ms | {r['regions_list_ms']} ms | "
              f"{r['read_ms']} ms | {r['ratio_count_to_read']} | {r['ratio_list_to_read']} |")
    ks = ("k_wall_region_tiles", "k_wall_region_seams", "k_wall_region_flatten", "k_wall_region_reduce", "k_wall_region_select")
    print("\n| window / flags | " + " | ".join(k[len("k_wall_region_"):] for k in ks) + " | sum |")
    print("|---|" + "---|" * (len(ks) + 1))
    for name, r in data.get("kernels_us", {}).items():
        print(f"| {name} | " + " | ".join(f"{r.get(k, 0)}" for k in ks) + f" | {round(sum(r.get(k, 0) for k in ks), 1)} µs |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--case")
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
