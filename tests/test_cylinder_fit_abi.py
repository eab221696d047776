"""Cylinder regression (GM_CFG_CYLINDER_FIT) checks that need no GPU: the entry points are exported, gm_cylinder_fit's
layout from a C99 compile matches the ctypes mirror, gm_create refuses the flag without the cylinder RANSAC, and the fp64
numpy twin (tests/cylfit_np.py) reaches the analytic truth of the synthetic frames from a perturbed start."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cylfit_np as cf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, B, FLOOR = 0.03, 5.0, -1.2


def test_fit_entry_points_are_exported_and_declared():
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in ("gm_get_cylinder_fit", "gm_fit_cylinder"):
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    assert _lib.GM_CFG_CYLINDER_FIT == 1 << 7
    import geometric_mapping_amd as g
    assert g.GM_CFG_CYLINDER_FIT == _lib.GM_CFG_CYLINDER_FIT
    assert L.gm_abi_version() == 3


def test_cylinder_fit_struct_layout_matches_ctypes():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "gm_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gm_cylinder_fit), offsetof(gm_cylinder_fit, status),
         offsetof(gm_cylinder_fit, inliers), offsetof(gm_cylinder_fit, passes), offsetof(gm_cylinder_fit, point),
         offsetof(gm_cylinder_fit, axis), offsetof(gm_cylinder_fit, radius), offsetof(gm_cylinder_fit, rms),
         offsetof(gm_cylinder_fit, last_step), offsetof(gm_cylinder_fit, model));
  printf("%u %u %u %u %u %u\n", GM_CFG_CYLINDER_FIT, GM_FIT_OK, GM_FIT_NO_MODEL, GM_FIT_DEGENERATE, GM_FIT_SINGULAR,
         GM_FIT_NOT_CONVERGED);
  printf("%zu %zu\n", sizeof(gm_config), sizeof(gm_frame_result));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    F = _lib.CylinderFit
    assert out[0] == C.sizeof(F)
    assert out[1:10] == [F.status.offset, F.inliers.offset, F.passes.offset, F.point.offset, F.axis.offset,
                         F.radius.offset, F.rms.offset, F.last_step.offset, F.model.offset]
    assert out[10:16] == [_lib.GM_CFG_CYLINDER_FIT, _lib.GM_FIT_OK, _lib.GM_FIT_NO_MODEL, _lib.GM_FIT_DEGENERATE,
                          _lib.GM_FIT_SINGULAR, _lib.GM_FIT_NOT_CONVERGED]
    assert out[16] == C.sizeof(_lib.Config) and out[17] == C.sizeof(_lib.FrameResult)   # existing structs did not grow


def test_create_rejects_fit_without_cylinder_ransac():
    L = _lib.load()
    ctx = C.c_void_p()
    cfg = _lib.Config()
    for extra in (0, _lib.GM_CFG_RANSAC_PLANE):
        L.gm_default_config(C.byref(cfg))
        cfg.flags |= _lib.GM_CFG_CYLINDER_FIT | extra
        assert L.gm_create(C.byref(cfg), C.byref(ctx)) == _lib.GM_ERR_INVALID_ARG
        assert not ctx.value
        assert b"cylinder" in L.gm_last_error(None).lower()


def _crop(p):
    p = p[np.all(np.isfinite(p), axis=1)]
    return p[np.all(np.abs(p) <= B, axis=1)]


def _check_twin(xyz, origin, start_err):
    el = ~(np.abs(xyz[:, 2] - FLOOR) < 3 * TAU)   # the floor band, as the plane RANSAC would take it
    init = cf.perturbed_init(origin, [1, 0, 0], 2.0)
    f = cf.fit_cylinder(xyz, init, TAU, el)
    assert f["status"] == cf.FIT_OK and f["passes"] == 3
    err = (abs(f["radius"] - 2.0), cf.axis_angle(f["axis"], [1, 0, 0]), cf.line_distance(f["point"], origin, [1, 0, 0]))
    assert err[0] < 1e-3 and err[1] < 1e-3 and err[2] < 2e-3, err
    assert err[0] < start_err[0] and err[1] < start_err[1]
    assert f["last_step"] < cf.STEP_BOUND and f["axis"] @ init[3:6] > 0
    # the true wall (|rho_true - 2| < tau, off the floor band) is inside the fitted band
    rho = np.linalg.norm(xyz[:, 1:].astype(np.float64) - np.asarray(origin[1:]), axis=1)
    wall = el & (np.abs(rho - 2.0) < TAU)
    assert f["inliers"][wall].mean() >= 0.95
    return f


def test_twin_meets_analytic_bounds_on_tunnel_frame():
    xyz = _crop(synth.tunnel_frame(200_000, seed=2, floor_z=FLOOR, outlier_frac=0.01))
    _check_twin(xyz, (0.0, 0.0, 0.0), (0.05, 0.04))


def test_twin_meets_analytic_bounds_on_velodyne_partial_arc():
    xyz = _crop(synth.velodyne_tunnel(rings=64)["xyz"])
    _check_twin(xyz, (0.0, 0.3, 0.5), (0.05, 0.04))


def test_twin_failure_modes():
    xyz = _crop(synth.tunnel_frame(20_000, seed=1))
    assert cf.fit_cylinder(xyz, np.full(7, np.nan, np.float32), TAU)["status"] == cf.FIT_NO_MODEL
    el = np.zeros(len(xyz), bool)
    el[:4] = True
    f = cf.fit_cylinder(xyz, cf.perturbed_init([0, 0, 0], [1, 0, 0], 2.0), TAU, el)
    assert f["status"] == cf.FIT_DEGENERATE and np.isnan(f["radius"]) and np.isnan(f["model"]).all()
