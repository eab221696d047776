"""GPU tests of the cylinder regression's failure and edge paths (csrc/k_cylfit.hip) through the stage call getCylinder:
GM_FIT_SINGULAR and GM_FIT_NOT_CONVERGED, which no other test reaches, rows that are not finite and points on the axis,
labels that make wall-like points ineligible, and the state a failed fit leaves for the next call on the context.  The
references are the fp64 twin (tests/cylfit_np.py) and the oracle's fp32 inlier predicate on the published row."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cylfit_np as cf  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0.03
GOOD_INIT = cf.perturbed_init([0, 0, 0], [1, 0, 0], 2.0, dr=0.02, tilt=0.01, shift=0.02)
RING_INIT = [0, 0, 0, 1, 0, 0, 2.01]


def _ring(x=0.0, n=2000):
    th = np.arange(n) * (2 * np.pi / n)
    return np.stack([np.full(n, x), 2 * np.cos(th), 2 * np.sin(th)], axis=1).astype(np.float32)


def _arc():
    """A 10-degree arc of the tube around +z, |x| < 2: about 1900 points that hardly constrain the axis."""
    xyz = synth.cylinder_frame(200_000, seed=9)
    phi = np.degrees(np.arctan2(xyz[:, 2], xyz[:, 1]))
    return xyz[(phi >= 85.0) & (phi < 95.0) & (np.abs(xyz[:, 0]) < 2.0)]


def _bad_rows():
    """A 20 k tube with NaN rows, rows with an infinite coordinate and points on the axis."""
    xyz = synth.cylinder_frame(20_000, seed=3)
    i = np.arange(len(xyz))
    xyz[i % 97 == 0] = np.nan
    xyz[i % 389 == 1, 0] = np.inf
    xyz[i % 397 == 2, 1] = -np.inf
    xyz[i % 101 == 5] = [1.0, 0.0, 0.0]
    return xyz


@pytest.fixture(scope="module")
def ctx(gm):
    with gm.GeometricMapping() as c:
        yield c


def _failed(f, mask, status, passes):
    assert f["status"] == status and f["passes"] == passes and not f["ok"] and f["inliers"] == 0
    assert np.isnan(f["radius"]) and np.isnan(f["rms"]) and np.isnan(f["last_step"])
    assert np.isnan(f["point"]).all() and np.isnan(f["axis"]).all() and np.isnan(f["model"]).all()
    assert not mask.any()


def _oracle_mask(oc, xyz, model, eligible=None):
    """The oracle's fp32 predicate on the published row, over the finite rows (a row that is not finite is no inlier)."""
    fin = np.isfinite(xyz).all(axis=1) if eligible is None else np.isfinite(xyz).all(axis=1) & eligible
    ref = np.zeros(int(fin.sum()), np.uint8)
    n = oc.label_cylinder(xyz[fin], ref, 0, 1, model, TAU)
    out = np.zeros(len(xyz), bool)
    out[fin] = ref == 1
    assert n == int(out.sum())
    return out


@pytest.mark.parametrize("x", [0.0, 0.5])
def test_singular(ctx, x):
    """One ring across the axis: t is the same for every point, the tilt columns of J vanish after the re-centring, the
    third Cholesky pivot is 0 in the first pass."""
    xyz = _ring(x)
    tw = cf.fit_cylinder(xyz, RING_INIT, TAU)
    assert (tw["status"], tw["passes"]) == (cf.FIT_SINGULAR, 0)
    f, mask = ctx.getCylinder(xyz, RING_INIT, TAU)
    _failed(f, mask, _lib.GM_FIT_SINGULAR, 0)
    assert _lib.GM_FIT_SINGULAR == cf.FIT_SINGULAR == 3


def test_not_converged(ctx, oc):
    """A 10-degree arc from a start 0.05 m and 0.04 rad off: the third step is still 0.053, five times
    GM_FIT_STEP_BOUND, so rounding cannot flip the flag; the parameters are published all the same.

    The geometry is ill-conditioned, so the bound on the parameters is measured, not fixed: the twin run again on the
    cloud with every coordinate moved by one fp32 ulp (seeded signs) moves the radius by 5.3e-6 m and the axis by
    3.9e-8 rad (measured on the CPU).  Allowed: ten times the larger of that spread and the 1e-5 of the well-conditioned
    edge sizes (test_stage_call_edge_sizes), i.e. 1e-4 m and 1e-4 rad."""
    xyz = _arc()
    assert 1800 < len(xyz) < 2000
    init = cf.perturbed_init([0, 0, 0], [1, 0, 0], 2.0, dr=0.05, tilt=0.04, shift=0.05)
    tw = cf.fit_cylinder(xyz, init, TAU)
    assert tw["status"] == cf.FIT_OK | cf.FIT_NOT_CONVERGED and tw["passes"] == 3
    assert 0.045 < tw["last_step"] < 0.06 and tw["last_step"] > 4 * cf.STEP_BOUND
    up = np.random.default_rng(100).integers(0, 2, xyz.shape).astype(bool)
    moved = np.where(up, np.nextafter(xyz, np.float32(np.inf)), np.nextafter(xyz, np.float32(-np.inf))).astype(np.float32)
    tw2 = cf.fit_cylinder(moved, init, TAU)
    spread_r, spread_a = abs(tw2["radius"] - tw["radius"]), cf.axis_angle(tw2["axis"], tw["axis"])
    print(f"ulp spread of the twin: radius {spread_r:.3e} m, axis {spread_a:.3e} rad")
    assert tw2["status"] == tw["status"] and spread_r < 1e-5 and spread_a < 1e-5
    f, mask = ctx.getCylinder(xyz, init, TAU)
    print(f"device against the twin: radius {abs(f['radius'] - tw['radius']):.3e} m, "
          f"axis {cf.axis_angle(f['axis'], tw['axis']):.3e} rad, last_step {f['last_step']:.6f} / {tw['last_step']:.6f}")
    assert f["status"] == _lib.GM_FIT_OK | _lib.GM_FIT_NOT_CONVERGED and f["passes"] == 3
    assert f["ok"] and not f["converged"] and f["last_step"] > 4 * _lib.GM_FIT_STEP_BOUND
    assert abs(f["radius"] - tw["radius"]) <= 10 * max(spread_r, 1e-5)
    assert cf.axis_angle(f["axis"], tw["axis"]) <= 10 * max(spread_a, 1e-5) and np.dot(f["axis"], tw["axis"]) > 0
    assert np.array_equal(mask, _oracle_mask(oc, xyz, f["model"])) and f["inliers"] == int(mask.sum()) > 0


def test_rows_that_are_not_finite_and_points_on_the_axis(ctx, oc):
    xyz = _bad_rows()
    fin = np.isfinite(xyz).all(axis=1)
    on_axis = fin & (xyz[:, 1] == 0) & (xyz[:, 2] == 0)
    assert (~fin).sum() > 250 and np.isinf(xyz).any() and on_axis.sum() > 150
    with np.errstate(invalid="ignore"):
        tw = cf.fit_cylinder(xyz, GOOD_INIT, TAU)
    assert tw["status"] == cf.FIT_OK and abs(tw["radius"] - 2.0) < 1e-3
    f, mask = ctx.getCylinder(xyz, GOOD_INIT, TAU)
    assert f["status"] == _lib.GM_FIT_OK and f["passes"] == 3
    assert abs(f["radius"] - tw["radius"]) < 1e-5 and cf.axis_angle(f["axis"], tw["axis"]) < 1e-5
    assert not mask[~fin].any() and not mask[on_axis].any()
    assert np.array_equal(mask, _oracle_mask(oc, xyz, f["model"])) and f["inliers"] == int(mask.sum()) > 18_000
    assert np.isfinite(f["rms"]) and f["rms"] < 0.02


def test_ineligible_shell(ctx, oc):
    """A second shell 0.02 m outside the tube, labelled 1, and want = 0: the shell takes no part in the sums (the fit
    over all points has a radius 5 mm larger) and no shell point is marked, although most lie inside tau of the fit."""
    tube, shell = synth.cylinder_frame(20_000, seed=3), synth.cylinder_frame(8_000, seed=4, radius=2.02)
    xyz, lab = np.concatenate([tube, shell]), np.r_[np.zeros(20_000, np.uint8), np.ones(8_000, np.uint8)]
    p = np.random.default_rng(1).permutation(len(xyz))
    xyz, lab = xyz[p], lab[p]
    tw, tw_all = cf.fit_cylinder(xyz, GOOD_INIT, TAU, lab == 0), cf.fit_cylinder(xyz, GOOD_INIT, TAU)
    assert tw["status"] == cf.FIT_OK and tw_all["radius"] - tw["radius"] > 3e-3
    f, mask = ctx.getCylinder(xyz, GOOD_INIT, TAU, lab, 0)
    assert f["status"] == _lib.GM_FIT_OK
    assert abs(f["radius"] - tw["radius"]) < 1e-5 and cf.axis_angle(f["axis"], tw["axis"]) < 1e-5
    assert not mask[lab == 1].any()
    everyone = _oracle_mask(oc, xyz, f["model"])
    assert everyone[lab == 1].mean() > 0.8                                # most of the shell: geometric inliers
    assert np.array_equal(mask, everyone & (lab == 0)) and f["inliers"] == int(mask.sum())


def _same_fit(a, b):
    for k in ("status", "inliers", "passes", "radius", "rms", "last_step"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in ("point", "axis", "model"):
        assert np.array_equal(a[k], b[k]), k


def test_a_failed_fit_leaves_the_context_fit_for_the_next(gm):
    """good, NO_MODEL, good, SINGULAR, good, DEGENERATE, good on one context: CylFitWork, the partial rows and the
    ticket carry nothing over, the four good calls are the fresh context's call byte for byte."""
    good = synth.cylinder_frame(30_000, seed=5)
    with gm.GeometricMapping() as c:
        ref, ref_mask = c.getCylinder(good, GOOD_INIT, TAU)
    assert ref["status"] == _lib.GM_FIT_OK and ref["passes"] == 3 and ref_mask.sum() > 25_000
    with gm.GeometricMapping() as c:
        def again():
            f, mask = c.getCylinder(good, GOOD_INIT, TAU)
            _same_fit(ref, f)
            assert np.array_equal(mask, ref_mask)
        again()
        f, mask = c.getCylinder(good, [np.nan] * 7, TAU)
        _failed(f, mask, _lib.GM_FIT_NO_MODEL, 0)
        again()
        f, mask = c.getCylinder(_ring(), RING_INIT, TAU)
        _failed(f, mask, _lib.GM_FIT_SINGULAR, 0)
        again()
        f, mask = c.getCylinder(good[:4], GOOD_INIT, TAU)
        _failed(f, mask, _lib.GM_FIT_DEGENERATE, 0)
        again()
