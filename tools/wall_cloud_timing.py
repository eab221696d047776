#!/usr/bin/env python3
"""Cost of gm_wall_map_cloud against gm_wall_map_read of the same window (the least any host-side export pays).

  python tools/wall_cloud_timing.py [--reps 25]       wall time of one sized call, of a count query and of the read
                                                      (medians after warm-up, alternated), for a 48-station window of
                                                      the default map and the 4096 x 4096 map at 1 % filled in patches
                                                      and fully filled, at strides (1,1) and (16,16); merged into
                                                      profiles/r10_wall_cloud.json under "wall"
  python tools/wall_cloud_timing.py --kernel [--case NAME]
                                                      a few calls per case and nothing else: run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_cloud_timing.py --kernel
                                                      in a run of its own, then
  python tools/wall_cloud_timing.py --summarize OUT   per-kernel medians of the trace, merged under "kernels_us"
  python tools/wall_cloud_timing.py --table           the DESIGN.md tables from the json

The byte floor quoted beside the kernels: 20 B per source cell read, 40 B per point written and copied.
GM_WALL_CLOUD_CHUNK=<blocks> in the environment changes the chunk (default 2^20 blocks); --summarize must run with the
value the traced run had: it derives the launches per case from it and refuses a trace of another length."""
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
from geometric_mapping_amd.api import RAW_CELL, WALL_CLOUD_POINT  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r10_wall_cloud.json")
# (name, n_stations, n_sectors, station0, n, fill)
WINDOWS = (("48_stations", 4000, 90, 1976, 48, "full"), ("4096x4096/patches", 4096, 4096, 0, 4096, "patches"),
           ("4096x4096/full", 4096, 4096, 0, 4096, "full"))
STRIDES = ((1, 1), (16, 16))
KERNEL_CALLS = 6


def chunk_blocks():
    """The library's rule for GM_WALL_CLOUD_CHUNK: 0, unreadable or above 2^20 is the default."""
    try:
        v = int(os.environ.get("GM_WALL_CLOUD_CHUNK", "0"))
    except ValueError:
        v = 0
    return v if 0 < v < (1 << 20) else 1 << 20


def field(n, ns, kind, seed=1):
    """Raw cells holding 8-47 points each: "full": every cell; "patches": ~1 % of the cells, in 8 x 6 patches."""
    rng = np.random.default_rng(seed)
    hit = np.ones((n, ns), bool)
    if kind == "patches":
        hit[:] = False
        for _ in range(max(1, n * ns // 4800)):
            j, k = rng.integers(0, n), rng.integers(0, ns)
            hit[j:j + 8, np.arange(k, k + 6) % ns] = True
    count = np.where(hit, rng.integers(8, 48, (n, ns)), 0)
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = rng.integers(-50000, 50000, (n, ns)) * count
    raw["min_key"] = np.where(hit, 0x40000000, 0)
    raw["max_key"] = np.where(hit, 0xC0000000, 0)
    return raw


def cases():
    for name, n, ns, s0, w, kind in WINDOWS:
        for bs, bk in STRIDES:
            yield f"{name}/{bs}x{bk}", n, ns, s0, w, kind, bs, bk


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def maps(c, only=None):
    """(case, map, ...) with one map per window, shared by its strides."""
    m, held = None, None
    for name, n, ns, s0, w, kind, bs, bk in cases():
        if only and only != name:
            continue
        if held != (n, ns, kind):
            if m is not None:
                m.close()
            m = c.wall_map(n_stations=n, n_sectors=ns)
            m.add_raw(field(n, ns, kind))
            held = (n, ns, kind)
        yield name, m, ns, s0, w, bs, bk
    if m is not None:
        m.close()


def wall(a):
    out = {}
    with g.GeometricMapping() as c:
        for name, m, ns, s0, w, bs, bk in maps(c):
            p = m.cloud_params(block_stations=bs, block_sectors=bk)
            info, got = _lib.WallCloudInfo(), C.c_uint64(0)
            buf = None

            def call():   # one call into a buffer that is large enough (sized by the first count query)
                nonlocal buf
                if buf is None:
                    c._check(c._L.gm_wall_map_cloud(m._h(), s0, w, C.byref(p), C.byref(info), None, 0, C.byref(got)))
                    buf = np.zeros(max(got.value, 1), dtype=WALL_CLOUD_POINT)
                c._check(c._L.gm_wall_map_cloud(m._h(), s0, w, C.byref(p), C.byref(info),
                                                buf.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)), len(buf), C.byref(got)))

            def count_only():
                c._check(c._L.gm_wall_map_cloud(m._h(), s0, w, C.byref(p), C.byref(info), None, 0, C.byref(got)))

            fns = ((call, "cloud"), (count_only, "count"), (lambda: m.read(s0, w), "read"))
            t = {"cloud": [], "count": [], "read": []}
            for f, key in fns:
                for _ in range(3):
                    f()
            for _ in range(a.reps):   # alternated, so that drift hits all three alike
                for f, key in fns:
                    t0 = time.perf_counter()
                    f()
                    t[key].append((time.perf_counter() - t0) * 1e3)
            out[name] = dict(cells=w * ns, blocks=int(info.blocks), points=int(info.points), cloud_ms=med(t["cloud"]),
                             count_ms=med(t["count"]), read_ms=med(t["read"]),
                             ratio_cloud_to_read=round(med(t["cloud"]) / med(t["read"]), 3),
                             floor_bytes=20 * w * ns + 2 * 40 * int(info.points), reps=a.reps)
            print(name, json.dumps(out[name]), flush=True)
    merge("wall", out)


def kernel(a):
    with g.GeometricMapping() as c:
        for name, m, ns, s0, w, bs, bk in maps(c, a.case):
            for _ in range(KERNEL_CALLS):
                info = m.cloud(s0, w, block_stations=bs, block_sectors=bk)[0]
            print(name, info["points"], flush=True)


def summarize(d):
    """Per kernel and case: the median over the launches of the case (a call launches once per chunk, and WallMap.cloud
    calls twice), the number of launches per call, and the median per call (launch median x launches per call)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for p in f for r in csv.DictReader(open(p))), key=lambda r: float(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        name = r["Kernel_Name"]
        key = "k_wall_cloud_merge" if "k_wall_cloud_merge" in name else ("k_compact_cloud" if "WallCloudPred" in name else None)
        if key:
            seq.append((key, (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
    out, at = {}, 0
    for name, n, ns, s0, w, kind, bs, bk in cases():
        NJ, NK = -(-w // bs), -(-ns // bk)
        rows_per_chunk = max(chunk_blocks() // NK, 1)
        chunks = -(-NJ // rows_per_chunk)
        per_call = chunks * (2 if (bs, bk) != (1, 1) else 1)
        take = seq[at:at + per_call * 2 * KERNEL_CALLS]   # (every case holds points: WallMap.cloud calls twice)
        at += len(take)
        for key in ("k_wall_cloud_merge", "k_compact_cloud"):
            v = [t for k, t in take if k == key][2 * chunks:]   # (the first call pair: warm-up)
            if v:
                out.setdefault(name, {})[key] = dict(launch_us=round(float(np.median(v)), 2), launches_per_call=chunks)
    if at != len(seq):
        sys.exit(f"{len(seq)} launches in the trace, {at} expected: summarize with the GM_WALL_CLOUD_CHUNK the traced run had "
                 f"(now {chunk_blocks()} blocks) and trace every case")
    merge("kernels_us", dict(chunk_blocks=chunk_blocks(), **out))
    print(json.dumps(out))


def table():
    data = json.load(open(OUT))
    print("| window / fill / stride | cells | points | count query | sized call | `gm_wall_map_read` | call / read | byte floor |")
    print("|---|---|---|---|---|---|---|---|")
    for name, r in data.get("wall", {}).items():
        print(f"| {name} | {r['cells']} | {r['points']} | {r['count_ms']} ms | {r['cloud_ms']} ms | {r['read_ms']} ms | "
              f"{r['ratio_cloud_to_read']} | {r['floor_bytes'] / 1e6:.1f} MB |")
    print("\n| window / fill / stride | launches per call | merge, per launch | compact + emit, per launch |")
    print("|---|---|---|---|")
    for name, r in data.get("kernels_us", {}).items():
        if name == "chunk_blocks":
            continue
        mg, cp = r.get("k_wall_cloud_merge"), r.get("k_compact_cloud")
        print(f"| {name} | {cp['launches_per_call'] if cp else ''} | {str(mg['launch_us']) + ' µs' if mg else '-'} | "
              f"{str(cp['launch_us']) + ' µs' if cp else '-'} |")


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
