#!/usr/bin/env python3
"""Cost of gm_wall_alignment_regions against gm_wall_map_regions on ONE straight map of the same window size and the same
cells, in the same session: what the piece table costs the two kernels that read a cell.

The alignment is straight - clothoid - arc - clothoid - straight at 400 stations each (ds 0.25 m, 90 sectors, arc radius
80 m); the window is the 512 stations around the clothoid -> arc joint at global station 800 (two pieces).  Beside it, 256
elements of two stations each (the same 512 stations: a piece every other row).  The straight map holds the same 512 x 90
cells.

  python tools/wall_alignment_regions_timing.py [--reps 25]   wall time of one blocking call with the list (medians after
                                                      warm-up, the three alternated) at ~1 % flagged in patches and 45 %
                                                      random; merged into profiles/r32_wall_alignment_regions.json under "wall"
  python tools/wall_alignment_regions_timing.py --kernel      a few calls per case and nothing else: run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_alignment_regions_timing.py --kernel
                                                      in a run of its own, then
  python tools/wall_alignment_regions_timing.py --summarize OUT   per-kernel medians of the trace, merged under "kernels_us"
  python tools/wall_alignment_regions_timing.py --table       the DESIGN.md tables from the json

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib  # noqa: E402
from geometric_mapping_amd.api import REGION  # noqa: E402
from wall_regions_timing import field  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r32_wall_alignment_regions.json")
NS, N, W = 90, 400, 512
LEFT = (0.0, -1.0)
FIVE = [dict(kind="straight", n_stations=N), dict(kind="clothoid", n_stations=N, turn=LEFT, curvature=0.0, rate=1.0 / (80.0 * N * 0.25)),
        dict(kind="arc", n_stations=N, turn=LEFT, curvature=1.0 / 80.0),
        dict(kind="clothoid", n_stations=N, turn=LEFT, curvature=1.0 / 80.0, rate=-1.0 / (80.0 * N * 0.25)), dict(kind="straight", n_stations=N)]
MANY = [dict(kind="arc", n_stations=2, turn=LEFT, curvature=1.0 / 80.0) if i % 2 else dict(kind="straight", n_stations=2) for i in range(256)]
KINDS = ("patches", "random")
KERNEL_CALLS = 6
# the order the callers of one case run in, here and in the trace
CALLERS = ("two_pieces", "256_pieces", "straight_map")


def rig(c, kind):
    """The three callers of one field: (name, handle's call, station0) on the same 512 x 90 cells."""
    raw = field(W, NS, kind)
    five = c.wall_alignment(FIVE, n_sectors=NS)
    s0 = 2 * N - W // 2
    for e, j0, part in ((1, N - W // 2, raw[:W // 2]), (2, 0, raw[W // 2:])):
        five.element(e).add_raw(part, j0)
    many = c.wall_alignment(MANY, n_sectors=NS)
    for e in range(256):
        many.element(e).add_raw(raw[2 * e:2 * e + 2])
    straight = c.wall_map(n_stations=W, n_sectors=NS)
    straight.add_raw(raw)
    L = c._L
    return ((five, L.gm_wall_alignment_regions, s0, _lib.WallAlignmentRegionsInfo), (many, L.gm_wall_alignment_regions, 0, _lib.WallAlignmentRegionsInfo),
            (straight, L.gm_wall_map_regions, 0, _lib.WallRegionsInfo))


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def caller(c, owner, fn, s0, Info):
    """One blocking call with the list into a buffer sized by a first count query; returns (call, info)."""
    p = owner.element(0).region_params(min_cells=1) if hasattr(owner, "element") else owner.region_params(min_cells=1)
    info, got = Info(), C.c_uint32(0)
    c._check(fn(owner._h(), None, s0, W, C.byref(p), C.byref(info), None, 0, C.byref(got), None))
    buf = np.zeros(max(got.value, 1), dtype=REGION)

    def call():
        c._check(fn(owner._h(), None, s0, W, C.byref(p), C.byref(info), buf.ctypes.data_as(C.POINTER(_lib.WallRegion)), len(buf), C.byref(got), None))
    return call, info, buf


def wall(a):
    out = {}
    with g.GeometricMapping() as c:
        for kind in KINDS:
            calls = [caller(c, *r) for r in rig(c, kind)]
            for call, _, _ in calls:
                for _ in range(3):
                    call()
            t = {k: [] for k in CALLERS}
            for _ in range(a.reps):   # alternated, so that drift hits all three alike
                for k, (call, _, _) in zip(CALLERS, calls):
                    t0 = time.perf_counter()
                    call()
                    t[k].append((time.perf_counter() - t0) * 1e3)
            info = calls[2][1]
            same = calls[1][2].tobytes() == calls[2][2].tobytes() and int(calls[0][1].regions) == int(info.regions)   # (the same cells)
            out[kind] = dict(cells=W * NS, flagged=int(info.flagged_pos + info.flagged_neg), components=int(info.components),
                             regions=int(info.regions), same_result=bool(same), reps=a.reps, **{f"{k}_ms": med(t[k]) for k in CALLERS})
            print(kind, json.dumps(out[kind]), flush=True)
    merge("wall", out)


def kernel(a):
    with g.GeometricMapping() as c:
        for kind in KINDS:
            for k, r in zip(CALLERS, rig(c, kind)):
                call, info, _ = caller(c, *r)   # (its count query: one run of the label kernels more, the warm-up)
                for _ in range(KERNEL_CALLS):
                    call()
                print(kind, k, int(info.components), flush=True)


def summarize(d):
    """Per (field, caller) the trace holds 1 + KERNEL_CALLS launches of tiles, seams and flatten and KERNEL_CALLS of reduce
    and select, in the order the callers ran; the joint kernels appear for the alignments only."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for p in f for r in csv.DictReader(open(p))), key=lambda r: float(r["Start_Timestamp"]))
    seq = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if "k_wall_region" in name:
            seq.setdefault(name.replace("_joint", ""), []).append((name, (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
    slots = [(kind, k) for kind in KINDS for k in CALLERS]
    out = {}
    for stage, v in seq.items():
        per = len(v) // len(slots)
        for i, (kind, k) in enumerate(slots):
            chunk = v[i * per:(i + 1) * per]
            out.setdefault(kind, {}).setdefault(k, {})[stage[len("k_wall_region_"):]] = round(float(np.median([x for _, x in chunk[1:]])), 2)
    merge("kernels_us", out)
    print(json.dumps(out))


def table():
    data = json.load(open(OUT))
    print("| field | cells | components | " + " | ".join(CALLERS) + " |")
    print("|---|---|---|" + "---|" * len(CALLERS))
    for kind, r in data.get("wall", {}).items():
        print(f"| {kind} | {r['cells']} | {r['components']} | " + " | ".join(f"{r[k + '_ms']} ms" for k in CALLERS) + " |")
    ks = ("tiles", "seams", "flatten", "reduce", "select")
    print("\n| field / caller | " + " | ".join(ks) + " | sum |")
    print("|---|" + "---|" * (len(ks) + 1))
    for kind, per in data.get("kernels_us", {}).items():
        for k in CALLERS:
            r = per.get(k, {})
            print(f"| {kind} / {k} | " + " | ".join(f"{r.get(s, 0)}" for s in ks) + f" | {round(sum(r.get(s, 0) for s in ks), 1)} µs |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
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
