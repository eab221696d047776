"""Persistent wall map (gm_wall_*) checks that need no GPU: the entry points are exported, declared and prototyped, the
new structs' layout from a C99 compile matches the ctypes mirrors, the defaults, NULL arguments are refused before a
device is touched, and the numpy twin's own arithmetic (tests/wall_np.py): the anchor makes the frame-local map frame
independent of the chainage, bad poses are refused, cells_from() sums over several adds and bins the drive's patches."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gm_wall_default_params", "gm_wall_map_create", "gm_wall_map_destroy", "gm_wall_map_add_frame",
       "gm_wall_map_add_points", "gm_wall_map_sync", "gm_wall_map_info", "gm_wall_map_read", "gm_wall_map_read_raw",
       "gm_wall_map_add_raw", "gm_wall_map_clear")


def test_wall_entry_points_are_exported_declared_and_prototyped():
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    assert _lib.GM_WALL_MAX_CELLS == 1 << 24 and _lib.GM_WALL_MAX_SECTORS == 4096
    assert L.gm_abi_version() == 3


def test_wall_struct_layouts_match_ctypes():
    fields = {
        "gm_wall_params": (_lib.WallParams, ("struct_size", "n_stations", "n_sectors", "reserved", "station_length", "t_min",
                                             "gate", "point", "direction", "radius", "up", "forward")),
        "gm_wall_raw_cell": (_lib.WallRawCell, ("sum", "count", "min_key", "max_key", "reserved")),
        "gm_wall_add_info": (_lib.WallAddInfo, ("struct_size", "status", "anchor_station", "o", "a", "u", "v", "R",
                                                "station_length", "sector_angle", "gate")),
        "gm_wall_info": (_lib.WallInfo, ("struct_size", "status", "n_stations", "n_sectors", "frames", "mapped", "outside",
                                         "beyond_gate", "plane", "cells_hit", "o", "a", "u", "v", "R")),
    }
    lines = []
    for name, (_, fs) in fields.items():
        lines.append(f'printf("%zu ", sizeof({name}));')
        lines += [f'printf("%zu ", offsetof({name}, {f}));' for f in fs]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gm_hip.h"\nint main(void) {\n' + "\n".join(lines) +
           '\nprintf("%u %u %zu %zu %zu\\n", GM_WALL_MAX_CELLS, GM_WALL_MAX_SECTORS, sizeof(gm_config), sizeof(gm_surface_cell),'
           ' sizeof(gm_surface_info));\nreturn 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = []
    for _, (T, fs) in fields.items():
        want.append(C.sizeof(T))
        want += [getattr(T, f).offset for f in fs]
    want += [_lib.GM_WALL_MAX_CELLS, _lib.GM_WALL_MAX_SECTORS, C.sizeof(_lib.Config), C.sizeof(_lib.SurfaceCell),
             C.sizeof(_lib.SurfaceInfo)]
    assert out == want
    assert C.sizeof(_lib.WallRawCell) == 24 == api.RAW_CELL.itemsize == wn.RAW_CELL.itemsize
    assert [api.RAW_CELL.fields[f][1] for f in ("sum", "count", "min_key", "max_key", "reserved")] == [0, 8, 12, 16, 20]


def test_default_wall_params():
    L = _lib.load()
    p = _lib.WallParams()
    L.gm_wall_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallParams) and p.reserved == 0
    assert (p.n_stations, p.n_sectors, p.station_length, p.t_min, p.gate, p.radius) == (4000, 90, 0.25, 0.0, 0.25, 2.0)
    assert list(p.point) == [0.0, 0.0, 0.0] and list(p.direction) == [1.0, 0.0, 0.0]
    assert list(p.up) == [0.0, 0.0, 1.0] and list(p.forward) == [1.0, 0.0, 0.0]
    assert p.n_stations * p.n_sectors <= _lib.GM_WALL_MAX_CELLS
    d = wn.params()
    for k in ("n_stations", "n_sectors", "station_length", "t_min", "gate", "radius"):
        assert getattr(p, k) == d[k]
    L.gm_wall_default_params(None)   # (a NULL is ignored)
    q = api.WallMap.params(n_sectors=360, direction=(0, 1, 0))
    assert q.n_sectors == 360 and list(q.direction) == [0.0, 1.0, 0.0] and q.n_stations == 4000


def test_null_arguments_are_refused():
    L = _lib.load()
    p = _lib.WallParams()
    L.gm_wall_default_params(C.byref(p))
    h = C.c_void_p()
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    xyz = (C.c_float * 3)(2, 0, 0)
    n = C.c_uint64(0)
    bad = _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_map_create(None, C.byref(p), C.byref(h)) == bad and not h.value
    assert L.gm_wall_map_add_frame(None, None, 0, pose, None) == bad
    assert L.gm_wall_map_add_points(None, xyz, 1, None, pose, None, None, None) == bad
    for fn in (L.gm_wall_map_sync,):
        assert fn(None) == bad
    assert L.gm_wall_map_info(None, C.byref(_lib.WallInfo())) == bad
    assert L.gm_wall_map_read(None, 0, 0, None, 0, C.byref(n)) == bad
    assert L.gm_wall_map_read_raw(None, 0, 0, None, 0, C.byref(n)) == bad
    assert L.gm_wall_map_add_raw(None, 0, 0, None) == bad
    assert L.gm_wall_map_clear(None, 0, 0) == bad
    L.gm_wall_map_destroy(None)   # (a NULL is ignored)


def test_twin_design_frame():
    f = wn.design_frame(wn.params(point=(3, 1, -1), direction=(-2, 0, 0)))   # pointing backwards: flipped forward
    assert f["status"] == wn.SURF_OK and np.allclose(f["a"], [1, 0, 0]) and np.allclose(f["u"], [0, 0, 1])
    assert np.allclose(f["v"], [0, -1, 0]) and np.allclose(f["o"], [0, 1, -1]) and f["R"] == 2.0
    g = wn.design_frame(wn.params(direction=(0, 0, 1), forward=(0, 0, 1)))
    assert g["status"] == wn.SURF_UP_FALLBACK and abs(g["u"] @ g["a"]) < 1e-15


def test_twin_anchor_makes_the_frame_independent_of_chainage():
    p, p0, p1 = wn.chainage_pair()
    D = wn.design_frame(p)
    f0, f1 = wn.add_frame(D, p, p0), wn.add_frame(D, p, p1)
    assert f1["anchor"] - f0["anchor"] == 20000 and f0["anchor"] == int(np.floor((1.375 + 8.0) / 0.25))
    for k in ("o", "a", "u", "v"):
        assert np.array_equal(f0[k].view(np.uint64), f1[k].view(np.uint64)), k
    # an oblique axis: o' may move by one fp32 ulp, nothing else
    q = wn.params(n_stations=20100, point=(1.0, 2.0, 0.5), direction=(1.0, 0.05, 0.02))
    D = wn.design_frame(q)
    g0 = wn.add_frame(D, q, p0)
    p2 = p0.copy()
    p2[:, 3] += 20000 * 0.25 * D["a"]
    g1 = wn.add_frame(D, q, p2)
    assert g1["anchor"] - g0["anchor"] in (19999, 20000, 20001)
    if g1["anchor"] - g0["anchor"] == 20000:
        ulp = np.spacing(np.abs(g0["o"]).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(g0["o"] - g1["o"]) <= ulp)
    for k in ("a", "u", "v"):
        assert np.array_equal(g0[k], g1[k])


def test_twin_refuses_bad_poses():
    good = synth.pose_matrix((1, 2, 3), yaw_deg=10, roll_deg=-4, pitch_deg=2)
    assert wn.pose_ok(good) and wn.pose_ok(np.vstack([good, [0, 0, 0, 1]]))
    scaled = good.copy()
    scaled[:, :3] *= 1.001
    mirrored = good.copy()
    mirrored[:, 0] *= -1
    nan = good.copy()
    nan[1, 3] = np.nan
    sheared = good.copy()
    sheared[0, 1] += 1e-4
    for bad in (scaled, mirrored, nan, sheared, good[:, :3]):
        assert not wn.pose_ok(bad)
    almost = good.copy()
    almost[0, 0] += 1e-8
    assert wn.pose_ok(almost)


def test_twin_bins_the_drive_onto_its_patches():
    d = synth.tunnel_drive(8, 60_000, seed=4, sigma=0.01)
    p = wn.params(n_stations=192, **d["design"])
    D = wn.design_frame(p)
    es, cs, per_frame = [], [], []
    for cloud, pose in d["frames"]:
        keep = np.all(np.abs(cloud) <= 5.0, axis=1)
        r = wn.points(cloud[keep], None, wn.add_frame(D, p, pose), p)
        assert 1.0 - r["ambiguous"].mean() > 0.99
        assert np.bincount(r["cls"], minlength=4).sum() == keep.sum()
        es.append(r["e"].astype(np.float32))
        cs.append(r["cell"])
        per_frame.append(wn.cells_from(es[-1], cs[-1], 192 * 90))
    raw = wn.cells_from(np.concatenate(es), np.concatenate(cs), 192 * 90)
    merged = per_frame[0]
    for r in per_frame[1:]:
        merged = wn.merge_raw(merged, r)
    assert raw.tobytes() == merged.tobytes()          # the rule is a function of the multiset: adds in any grouping
    count, mean, mn, mx = (x.reshape(192, 90) for x in wn.records_from(raw))
    seen = 0
    for t0, t1, p0, p1, dr in d["patches"]:
        js, ks = slice(int(t0 / 0.25), int(t1 / 0.25)), slice(int(p0 / 4), int(p1 / 4))
        c, m = count[js, ks].astype(np.float64), mean[js, ks].astype(np.float64)
        ok = c > 0
        seen += int(ok.sum())
        assert np.all(np.abs(m[ok] - dr) <= 4 * 0.01 / np.sqrt(c[ok]) + 2e-4), (dr, m)
    assert seen == 2 * 48 + 40   # every cell of the three patches was seen
    assert np.all(count[int(40 / 0.25):] == 0) and np.all(np.isnan(mean[int(40 / 0.25):]))   # nobody drove there
