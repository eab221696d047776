"""Wall deviation map (GM_CFG_SURFACE_MAP) checks that need no GPU: the entry points are exported, declared and
prototyped, the new structs' layout from a C99 compile matches the ctypes mirrors, the default parameters, gm_create
refuses the flag without the cylinder regression before it touches a device, NULL arguments are refused, and the numpy
twin (tests/surface_np.py) bins the analytic patch tunnel onto its patches."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_np as sn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gm_surface_default_params", "gm_set_surface_params", "gm_get_surface_map", "gm_get_surface_points",
       "gm_surface_map")


def test_surface_entry_points_are_exported_declared_and_prototyped():
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    assert _lib.GM_CFG_SURFACE_MAP == 1 << 8 and _lib.GM_SURF_MAX_CELLS >= 4096
    assert L.gm_abi_version() == 3


def test_surface_struct_layouts_match_ctypes():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "gm_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gm_surface_params), offsetof(gm_surface_params, n_stations),
         offsetof(gm_surface_params, n_sectors), offsetof(gm_surface_params, station_length),
         offsetof(gm_surface_params, t_min), offsetof(gm_surface_params, gate), offsetof(gm_surface_params, up),
         offsetof(gm_surface_params, forward));
  printf("%zu %zu %zu %zu\n", sizeof(gm_surface_cell), offsetof(gm_surface_cell, mean), offsetof(gm_surface_cell, min),
         offsetof(gm_surface_cell, max));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gm_surface_info), offsetof(gm_surface_info, status),
         offsetof(gm_surface_info, mapped), offsetof(gm_surface_info, plane), offsetof(gm_surface_info, cells_hit),
         offsetof(gm_surface_info, o), offsetof(gm_surface_info, v), offsetof(gm_surface_info, R),
         offsetof(gm_surface_info, t_min), offsetof(gm_surface_info, sector_angle));
  printf("%u %u %u %u %u\n", GM_CFG_SURFACE_MAP, GM_SURF_MAX_CELLS, GM_SURF_OK, GM_SURF_NO_MODEL, GM_SURF_UP_FALLBACK);
  printf("%zu %zu %zu\n", sizeof(gm_config), sizeof(gm_frame_result), sizeof(gm_cylinder_fit));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    P, Q, I = _lib.SurfaceParams, _lib.SurfaceCell, _lib.SurfaceInfo
    assert out[0:8] == [C.sizeof(P), P.n_stations.offset, P.n_sectors.offset, P.station_length.offset, P.t_min.offset,
                        P.gate.offset, P.up.offset, P.forward.offset]
    assert out[8:12] == [C.sizeof(Q), Q.mean.offset, Q.min.offset, Q.max.offset] and out[8] == 16
    assert out[12:22] == [C.sizeof(I), I.status.offset, I.mapped.offset, I.plane.offset, I.cells_hit.offset, I.o.offset,
                          I.v.offset, I.R.offset, I.t_min.offset, I.sector_angle.offset]
    assert out[22:27] == [_lib.GM_CFG_SURFACE_MAP, _lib.GM_SURF_MAX_CELLS, _lib.GM_SURF_OK, _lib.GM_SURF_NO_MODEL,
                          _lib.GM_SURF_UP_FALLBACK]
    # the existing structs did not change
    assert out[27:30] == [C.sizeof(_lib.Config), C.sizeof(_lib.FrameResult), C.sizeof(_lib.CylinderFit)]


def test_default_surface_params():
    L = _lib.load()
    p = _lib.SurfaceParams()
    L.gm_surface_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.SurfaceParams)
    assert (p.n_stations, p.n_sectors, p.station_length, p.t_min, p.gate) == (40, 90, 0.25, -5.0, 0.25)
    assert list(p.up) == [0.0, 0.0, 1.0] and list(p.forward) == [1.0, 0.0, 0.0]
    assert p.n_stations * p.n_sectors <= _lib.GM_SURF_MAX_CELLS
    L.gm_surface_default_params(None)   # (a NULL is ignored)


def test_create_rejects_surface_map_without_cylinder_fit():
    L = _lib.load()
    ctx = C.c_void_p()
    cfg = _lib.Config()
    for extra in (0, _lib.GM_CFG_RANSAC_CYLINDER, _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER):
        L.gm_default_config(C.byref(cfg))
        cfg.flags |= _lib.GM_CFG_SURFACE_MAP | extra
        assert L.gm_create(C.byref(cfg), C.byref(ctx)) == _lib.GM_ERR_INVALID_ARG   # not GM_ERR_DEVICE: no device touched
        assert not ctx.value
        assert b"GM_CFG_SURFACE_MAP" in L.gm_last_error(None)


def test_null_arguments_are_refused():
    L = _lib.load()
    p = _lib.SurfaceParams()
    L.gm_surface_default_params(C.byref(p))
    info = _lib.SurfaceInfo()
    cells = (_lib.SurfaceCell * 3600)()
    n = C.c_uint32(0)
    m = (C.c_float * 7)(0, 0, 0, 1, 0, 0, 2)
    xyz = (C.c_float * 3)(2, 0, 0)
    assert L.gm_set_surface_params(None, C.byref(p)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_get_surface_map(None, 0, C.byref(info), cells, 3600, C.byref(n)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_get_surface_points(None, 0, None, None, 0, C.byref(n)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_surface_map(None, xyz, 1, None, m, C.byref(p), C.byref(info), cells, 3600, None, None) == _lib.GM_ERR_INVALID_ARG


def test_twin_frame_and_bins_on_the_patch_tunnel():
    xyz = synth.tunnel_patches(200_000, seed=3)
    xyz = xyz[np.all(np.abs(xyz) <= 5.0, axis=1)]
    f = sn.map_frame([0, 0, 0, -1, 0, 0, 2.0])            # a fit that points backwards: a is flipped forward
    assert f["status"] == sn.SURF_OK and np.allclose(f["a"], [1, 0, 0]) and np.allclose(f["u"], [0, 0, 1])
    assert np.allclose(f["v"], [0, -1, 0]) and np.allclose(f["o"], 0)
    assert sn.map_frame([0, 0, 0, 0, 0, 1, 2.0])["status"] == sn.SURF_UP_FALLBACK
    assert sn.map_frame([math.nan, 0, 0, 1, 0, 0, 2.0]) is None
    p = sn.params()
    lab = (np.abs(xyz[:, 2] + 1.2) < 0.05).astype(np.uint8)   # the floor as the plane would take it
    r = sn.points(xyz, lab, f["o"], f["a"], f["u"], f["v"], f["R"], p)
    assert np.bincount(r["cls"], minlength=4).sum() == len(xyz) and (r["cls"] == sn.PLANE).sum() == lab.sum()
    count, mean, _, _ = sn.cells_from(r["e"].astype(np.float32), r["cell"], 3600)
    count, mean = count.reshape(40, 90), mean.reshape(40, 90)
    for t0, t1, p0, p1, dr in synth.SURFACE_PATCHES:
        js, ks = slice(int((t0 + 5) / 0.25), int((t1 + 5) / 0.25)), slice(int(p0 / 4), int(p1 / 4))
        c, m = count[js, ks], mean[js, ks]
        assert np.all(np.abs(m - dr) <= 4 * 0.01 / np.sqrt(c) + 2e-4), (dr, m)
