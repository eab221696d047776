#!/usr/bin/env python3
"""Cost of gm_wall_map_mesh against gm_wall_map_cloud of the same window on the same build.

  python tools/wall_mesh_timing.py [--reps 25]        wall time of one sized mesh call and of one sized cloud call
                                                      (medians after warm-up, alternated) for a 48-station window of the
                                                      default map at the map's resolution and for the whole default map
                                                      with 4 x 4 blocks, with the bytes that crossed PCIe; merged into
                                                      profiles/r21_wall_mesh.json under "wall"
  python tools/wall_mesh_timing.py --kernel           a few calls per case and nothing else: run it under
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/wall_mesh_timing.py --kernel
                                                      in a run of its own, then
  python tools/wall_mesh_timing.py --summarize OUT    per-kernel medians of the trace, merged under "kernels_us"
  python tools/wall_mesh_timing.py --cloud-only [--reps 25]
                                                      gm_wall_map_cloud alone on the same cases: its median, its spread
                                                      and a digest of its output, printed as one json line -- for runs of
                                                      two builds alternated on one box (this file runs on a tree without
                                                      the mesh, too)"""
import argparse
import csv
import ctypes as C
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("GM_TIMING_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geometric_mapping_amd as g  # noqa: E402
from geometric_mapping_amd import _lib  # noqa: E402
from geometric_mapping_amd.api import RAW_CELL, WALL_CLOUD_POINT  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r21_wall_mesh.json")
# (name, station0, n, block_stations, block_sectors) on the default map (4000 x 90), every cell filled
CASES = (("48_stations/1x1", 1976, 48, 1, 1), ("whole_map/4x4", 0, 4000, 4, 4))
KERNEL_CALLS = 6
KERNELS = (("WallMeshVertexEmit", "k_compact_mesh_vertices"), ("WallMeshPred", "k_compact_mesh_triangles"),
           ("WallCloudEmit", "k_compact_cloud"), ("k_wall_cloud_merge", "k_wall_cloud_merge"))


def field(n, ns, seed=1):
    """Raw cells holding 8-47 points each, means within +-0.05 m."""
    rng = np.random.default_rng(seed)
    count = rng.integers(8, 48, (n, ns))
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = count
    raw["sum"] = rng.integers(-50000, 50000, (n, ns)) * count
    raw["min_key"] = 0x40000000
    raw["max_key"] = 0xC0000000
    return raw


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def med(v):
    return round(float(np.median(v)), 4)


def cloud_call(c, m, s0, w, bs, bk):
    """A sized gm_wall_map_cloud call into a buffer that is large enough; returns (call, buffer, info)."""
    p = m.cloud_params(block_stations=bs, block_sectors=bk)
    info, got = _lib.WallCloudInfo(), C.c_uint64(0)
    c._check(c._L.gm_wall_map_cloud(m._h(), s0, w, C.byref(p), C.byref(info), None, 0, C.byref(got)))
    buf = np.zeros(max(got.value, 1), dtype=WALL_CLOUD_POINT)

    def call():
        c._check(c._L.gm_wall_map_cloud(m._h(), s0, w, C.byref(p), C.byref(info),
                                        buf.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)), len(buf), C.byref(got)))
    return call, buf, info


def mesh_call(c, m, s0, w, bs, bk):
    p = _lib.WallMeshParams()
    c._L.gm_wall_mesh_default_params(C.byref(p))
    p.cloud = m.cloud_params(block_stations=bs, block_sectors=bk)
    info, nv, nt = _lib.WallMeshInfo(), C.c_uint64(0), C.c_uint64(0)
    c._check(c._L.gm_wall_map_mesh(m._h(), s0, w, C.byref(p), C.byref(info), None, 0, None, 0, C.byref(nv), C.byref(nt)))
    v = np.zeros(max(nv.value, 1), dtype=WALL_CLOUD_POINT)
    t = np.zeros((max(nt.value, 1), 3), dtype=np.uint32)

    def call():
        c._check(c._L.gm_wall_map_mesh(m._h(), s0, w, C.byref(p), C.byref(info), v.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)),
                                       len(v), t.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle)), len(t), C.byref(nv), C.byref(nt)))
    return call, info


def wall(a):
    out = {}
    with g.GeometricMapping() as c:
        m = c.wall_map()
        m.add_raw(field(m.n_stations, m.n_sectors))
        for name, s0, w, bs, bk in CASES:
            cloud, _, cinfo = cloud_call(c, m, s0, w, bs, bk)
            mesh, minfo = mesh_call(c, m, s0, w, bs, bk)
            fns = ((mesh, "mesh"), (cloud, "cloud"))
            t = {"mesh": [], "cloud": []}
            for f, _k in fns:
                for _ in range(3):
                    f()
            for _ in range(a.reps):   # alternated, so that drift hits both alike
                for f, key in fns:
                    t0 = time.perf_counter()
                    f()
                    t[key].append((time.perf_counter() - t0) * 1e3)
            nv, nt = int(minfo.cloud.points), int(minfo.triangles)
            out[name] = dict(blocks=int(cinfo.blocks), vertices=nv, triangles=nt, mesh_ms=med(t["mesh"]), cloud_ms=med(t["cloud"]),
                             mesh_minus_cloud_ms=round(med(t["mesh"]) - med(t["cloud"]), 4),
                             mesh_min_max_ms=[round(min(t["mesh"]), 4), round(max(t["mesh"]), 4)],
                             cloud_min_max_ms=[round(min(t["cloud"]), 4), round(max(t["cloud"]), 4)],
                             pcie_bytes_cloud=40 * nv + 32, pcie_bytes_mesh=40 * nv + 12 * nt + 32 + 48,
                             streamed_bytes_triangle_pass=4 * int(cinfo.blocks) + 12 * nt, reps=a.reps)
            print(name, json.dumps(out[name]), flush=True)
    merge("wall", out)


def cloud_only(a):
    out = {}
    with g.GeometricMapping() as c:
        m = c.wall_map()
        m.add_raw(field(m.n_stations, m.n_sectors))
        for name, s0, w, bs, bk in CASES:
            cloud, buf, info = cloud_call(c, m, s0, w, bs, bk)
            for _ in range(3):
                cloud()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                cloud()
                t.append((time.perf_counter() - t0) * 1e3)
            out[name] = dict(cloud_ms=med(t), min_ms=round(min(t), 4), max_ms=round(max(t), 4), points=int(info.points),
                             sha256=hashlib.sha256(buf[:int(info.points)].tobytes()).hexdigest()[:16])
    print(json.dumps(dict(root=ROOT, **out)), flush=True)


def kernel(a):
    with g.GeometricMapping() as c:
        m = c.wall_map()
        m.add_raw(field(m.n_stations, m.n_sectors))
        for name, s0, w, bs, bk in CASES:
            cloud, _, _ = cloud_call(c, m, s0, w, bs, bk)
            mesh, _ = mesh_call(c, m, s0, w, bs, bk)
            for _ in range(KERNEL_CALLS):
                mesh()
                cloud()
            print(name, flush=True)


def summarize(d):
    """Per case and kernel: the median over the case's launches (every case is one chunk: one launch per call and kernel;
    each case starts with one count query of the cloud and one of the mesh, dropped with the first timed call as warm-up)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for p in f for r in csv.DictReader(open(p))), key=lambda r: float(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        key = next((k for pat, k in KERNELS if pat in r["Kernel_Name"]), None)
        if key:
            seq.append((key, (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
    out, at = {}, 0
    for name, s0, w, bs, bk in CASES:
        merged = (bs, bk) != (1, 1)
        per_case = (KERNEL_CALLS + 1) * (3 + (2 if merged else 0))   # vertices, triangles, cloud (+ a merge for either)
        take = seq[at:at + per_case]
        at += len(take)
        for _pat, key in KERNELS:
            v = [t for k, t in take if k == key][2:]
            if v:
                out.setdefault(name, {})[key] = round(float(np.median(v)), 2)
    if at != len(seq):
        sys.exit(f"{len(seq)} launches in the trace, {at} expected")
    merge("kernels_us", out)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--cloud-only", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernel:
        kernel(a)
    elif a.cloud_only:
        cloud_only(a)
    else:
        wall(a)


if __name__ == "__main__":
    main()
