#!/usr/bin/env python3
"""Cost of the checked add (gm_wall_map_add_frame_checked) beside the plain add, and a driver for the kernel trace.

  python tools/wall_add_checked_timing.py [--points 1000000] [--frames 40]
        blocking frames that end in check_frame + add_frame and in check_frame + add_frame_checked (no row selected: a
        threshold of 8 m; the world-fixed patches selected: the default check), alternated in one process: medians and the
        checked add's cost per frame; then the same three variants through a four-slot pipeline: frames per second
  python tools/wall_add_checked_timing.py --kernel [--plain] [--points N] [--frames 12]
        blocking frames, each followed by a plain add_frame and (without --plain) by a check without rows and its checked
        add, then by the default check and its checked add, all on one map that holds the bare wall.  --plain is for a library built from a commit
        before the checked add existed: the same frames, the plain add only.  Run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_add_checked_timing.py --kernel
        in a run of its own, then
  python tools/wall_add_checked_timing.py --summarize OUT
        per-kernel calls, median / min / max from the trace"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import synth  # noqa: E402

IDENT = np.eye(4)[:3]
NOMINAL = dict(n_stations=4000, t_min=-500.0)   # the patch tunnel sits around chainage 0
NONE = dict(threshold=8.0, gate=8.0, min_count=1)   # a check without rows
PATCHES = dict(min_count=1)                          # the default check: the patches' points are rows
WARMUP = 3
VARIANTS = ("plain", "checked_none", "checked_patches")


def stats(v):
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def survey_of(c, xyz):
    """A map that holds the bare wall -- the patch tunnel's frame with its patch points left out -- at a weight of 4000
    frames, so that the frames the timed loops add (patch points included, in the plain variant) do not move its means."""
    bare = synth.tunnel_patches(len(xyz), seed=2, patches=())
    same = np.all(bare == xyz, axis=1)
    tmp = c.wall_map(**NOMINAL)
    for _ in range(4):
        tmp.add_points(xyz[same], IDENT, outputs=False)
    raw = tmp.read_raw()
    tmp.close()
    raw["sum"] *= 1000
    raw["count"] *= 1000
    m = c.wall_map(**NOMINAL)
    m.add_raw(raw)
    return m


def tail(m, slot, variant):
    """What follows a frame: the check, then the add into the same map."""
    m.check_frame(slot, IDENT, **(NONE if variant == "checked_none" else PATCHES))
    if variant == "plain":
        m.add_frame(slot, IDENT)
    else:
        m.add_frame_checked(slot, IDENT)


def pipeline(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    out = {}
    with g.GeometricMapping(**kw) as c:
        m = survey_of(c, xyz)

        def frame(variant):
            t0 = time.perf_counter()
            c.process_frame(xyz)
            tail(m, 0, variant)
            m.sync()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(WARMUP):
            for v in VARIANTS:
                frame(v)
        t = {v: [] for v in VARIANTS}
        for k in range(a.frames):
            for v in (VARIANTS if k % 2 else VARIANTS[::-1]):
                t[v].append(frame(v))
        out["blocking_ms"] = {v: stats(t[v]) for v in VARIANTS}
        for v in VARIANTS[1:]:
            out["blocking_ms"][v]["cost_ms"] = float(np.median(t[v]) - np.median(t["plain"]))
        out["skipped_last"] = m.add_checked_result(0)["skipped"]
    with g.GeometricMapping(n_slots=4, **kw) as c:
        m = survey_of(c, xyz)

        def run(variant, n):
            t0 = time.perf_counter()
            for k in range(n):
                if k >= 4:
                    c.wait_frame(k % 4)
                c.submit_frame(k % 4, xyz)
                tail(m, k % 4, variant)
            for k in range(4):
                c.wait_frame(k)
            m.sync()
            return n / (time.perf_counter() - t0)

        for v in VARIANTS:
            run(v, 8)
        fps = {v: [] for v in VARIANTS}
        for r in range(5):
            for v in (VARIANTS if r % 2 else VARIANTS[::-1]):
                fps[v].append(run(v, a.frames))
        out["four_slots_fps"] = {v: dict(median=float(np.median(fps[v])), min=float(min(fps[v])), max=float(max(fps[v]))) for v in VARIANTS}
    print(json.dumps(dict(points=a.points, frames=a.frames, **out)))


def kernel(a):
    xyz = synth.tunnel_patches(a.points, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(a.points), max_points=a.points)
    with g.GeometricMapping(**kw) as c:
        m = survey_of(c, xyz)
        info = {}
        for _ in range(WARMUP + a.frames):
            res = c.process_frame(xyz)
            m.add_frame(0, IDENT)
            if not a.plain:
                for name, ck in (("none", NONE), ("patches", PATCHES)):
                    m.check_frame(0, IDENT, **ck)
                    m.add_frame_checked(0, IDENT)
                    info[name] = m.add_checked_result(0)
            m.sync()
        print(json.dumps(dict(points=len(xyz), n_valid=res["n_valid"], calls=WARMUP + a.frames, plain_only=bool(a.plain),
                              **{k: dict(n_rows=v["n_rows"], skipped=v["skipped"]) for k, v in info.items()})))


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: float(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        if "k_wall_add" in name:
            masked = "k_wall_add_masked" in name
            by.setdefault("k_wall_add_masked" if masked else "k_wall_add", []).append(us)
        elif "k_wall_mark" in name:
            by.setdefault("k_wall_mark", []).append(us)
        elif "fillBuffer" in name:
            by.setdefault("fill_kernels_all", []).append(us)
    series = dict(by)
    if "k_wall_add" in series:
        series["k_wall_add"] = series["k_wall_add"][4:]   # (the survey's four stage adds)
    for k in ("k_wall_add_masked", "k_wall_mark"):   # alternating: the check without rows, the default check
        if k in by:
            series[k + "_none"], series[k + "_patches"] = by[k][0::2], by[k][1::2]
            del series[k]
    out = {}
    for name, v in series.items():
        v = v[WARMUP:] if len(v) > 2 * WARMUP else v
        if v:
            out[name] = dict(calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                             p10_us=round(float(np.percentile(v, 10)), 2), p90_us=round(float(np.percentile(v, 90)), 2))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernel:
        kernel(a)
    else:
        pipeline(a)


if __name__ == "__main__":
    main()
