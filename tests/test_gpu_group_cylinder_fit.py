"""GPU tests of gm_group_fit_cylinder: the cylinder regression over a sharded frame, its ranks' sums merged on the device.

A 1-rank group over real RCCL reproduces the single-device fit (GM_CFG_CYLINDER_FIT) bit for bit, labels included.
Loopback groups of 2 and 4 ranks agree with the fp64 numpy twin (tests/cylfit_np.py) on the merged cloud, their labels
are the oracle's fp32 predicates on the published plane and the fitted row, and the 1 M-point tunnel meets the analytic
truth.  Edge cases: a caller start, a plane-only cloud, repeat calls, NOT_READY before a sharded frame and after a
streamed submit."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cylfit_np as cf  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, FLOOR, H, SEED = 0.03, -1.2, 1024, 7
BASE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER
KW = dict(ransac_hypotheses=H, ransac_threshold=TAU, ransac_seed=SEED)


def _same_fit(a, b):
    for k in ("status", "inliers", "passes", "radius", "rms", "last_step"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    for k in ("point", "axis", "model"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _errors(point, axis, radius, origin):
    return (abs(radius - 2.0), cf.axis_angle(axis, [1, 0, 0]), cf.line_distance(point, origin, [1, 0, 0]))


def _plane_labels(oc, cloud, res):
    lab = np.zeros(len(cloud), np.uint8)
    oc.label_plane(cloud, lab, 0, 1, res["plane"], TAU)
    return lab


def _check_against_twin(oc, cloud, res, labels, f, init):
    """item 2 of the issue: the twin on the merged cloud, the oracle's labels bit for bit, inliers = count of label 2"""
    ref = _plane_labels(oc, cloud, res)
    tw = cf.fit_cylinder(cloud, init, TAU, ref != 1)
    assert tw["status"] == f["status"], (tw["status"], f["status"])
    assert abs(f["radius"] - tw["radius"]) < 1e-6 * tw["radius"]
    assert np.abs(f["point"] - tw["point"]).max() < 1e-6 * max(1.0, np.abs(tw["point"]).max())
    assert cf.axis_angle(f["axis"], tw["axis"]) < 1e-7 and np.dot(f["axis"], tw["axis"]) > 0
    n = oc.label_cylinder(cloud, ref, 0, 2, f["model"], TAU)
    assert n == f["inliers"] == int((labels == 2).sum())
    assert np.array_equal(labels, ref)


def test_one_rank_group_over_rccl_equals_the_single_device_fit(gm):
    xyz = synth.tunnel_frame(150_000, seed=5, floor_z=FLOOR, outlier_frac=0.01)
    kw = dict(KW, neighborRadius=0.3)
    with gm.GeometricMapping(flags=BASE | _lib.GM_CFG_CYLINDER_FIT, **kw) as c:
        ref_res = c.process_frame(xyz)
        ref, ref_lab = c.cylinder_fit(), c.labels()
    assert ref["ok"]
    with gm.GeometricMappingGroup([0], flags=BASE, **kw) as g:        # distinct devices: the RCCL path
        res = g.process_frame(xyz)
        assert np.array_equal(res["cylinder"], ref_res["cylinder"]) and np.array_equal(res["plane"], ref_res["plane"])
        f = g.fit_cylinder()
        _same_fit(ref, f)
        assert np.array_equal(g.labels(), ref_lab)
        _same_fit(f, g.last_cylinder_fit())


def _frames():
    return {"tunnel": (synth.tunnel_frame(150_000, seed=2, floor_z=FLOOR, outlier_frac=0.01), (0.0, 0.0, 0.0), 0.3),
            "velodyne": (synth.velodyne_tunnel(rings=64)["xyz"], (0.0, 0.3, 0.5), None)}


@pytest.fixture(scope="module")
def sharded(gm):
    out = {}
    for name, (xyz, origin, nr) in _frames().items():
        kw = dict(KW, neighborRadius=nr) if nr else dict(KW)
        for n_ranks in (2, 4):
            with gm.GeometricMappingGroup([0] * n_ranks, loopback=True, flags=BASE, **kw) as g:
                res = g.process_frame(xyz)
                cloud, rows = g.cropped_cloud()
                f = g.fit_cylinder()
                lab = g.labels()
                got = g.last_cylinder_fit()
                init = cf.perturbed_init(origin, [1, 0, 0], 2.0)
                fp = g.fit_cylinder(init)
                lab_p = g.labels()
                again = g.fit_cylinder()
                lab_again = g.labels()
            out[(name, n_ranks)] = dict(xyz=xyz, origin=origin, res=res, cloud=cloud, rows=rows, fit=f, labels=lab,
                                        got=got, init=init, fit_p=fp, labels_p=lab_p, again=again, labels_again=lab_again)
    return out


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_loopback_fit_matches_twin_and_oracle_labels(sharded, oc, name, n_ranks):
    r = sharded[(name, n_ranks)]
    f = r["fit"]
    assert f["ok"] and f["passes"] == 3, f
    _check_against_twin(oc, r["cloud"], r["res"], r["labels"], f, r["res"]["cylinder"])
    assert np.dot(f["axis"], r["res"]["cylinder"][3:6]) > 0
    _same_fit(f, r["got"])                                             # gm_group_get_cylinder_fit returns the call's


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_loopback_fit_from_a_caller_start(sharded, oc, name, n_ranks):
    r = sharded[(name, n_ranks)]
    assert r["fit_p"]["ok"], r["fit_p"]
    _check_against_twin(oc, r["cloud"], r["res"], r["labels_p"], r["fit_p"], r["init"])


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_second_call_gives_the_same_bits(sharded, name, n_ranks):
    r = sharded[(name, n_ranks)]
    _same_fit(r["fit"], r["again"])                                    # (a caller-start fit ran in between)
    assert np.array_equal(r["labels"], r["labels_again"])


def test_sharded_fit_meets_analytic_truth(gm):
    xyz = synth.tunnel_frame(1_000_000, seed=2, floor_z=FLOOR, outlier_frac=0.01)
    kw = dict(KW, neighborRadius=synth.fixed_k_radius(len(xyz)))
    with gm.GeometricMappingGroup([0] * 4, loopback=True, flags=BASE, **kw) as g:
        res = g.process_frame(xyz)
        f = g.fit_cylinder()
        cloud, rows = g.cropped_cloud()
        lab = g.labels()
    assert f["ok"] and f["converged"] and f["passes"] == 3, f
    assert f["status"] == _lib.GM_FIT_OK
    origin = (0.0, 0.0, 0.0)
    err = _errors(f["point"], f["axis"], f["radius"], origin)
    assert err[0] < 1e-3 and err[1] < 1e-3 and err[2] < 2e-3, err
    hyp = res["cylinder"].astype(np.float64)
    herr = _errors(hyp[:3], hyp[3:6], hyp[6], origin)
    assert all(e < h for e, h in zip(err, herr)), (err, herr)          # better than the voted hypothesis on every count
    assert np.array_equal(xyz[rows], cloud)
    rho = np.linalg.norm(cloud[:, 1:].astype(np.float64) - np.asarray(origin[1:]), axis=1)
    wall = (np.abs(rho - 2.0) < TAU) & (lab != 1)
    assert wall.sum() > 1000 and (lab[wall] == 2).mean() >= 0.95, (lab[wall] == 2).mean()
    assert f["inliers"] == int((lab == 2).sum())


def test_plane_only_cloud_has_no_model_and_plane_labels(gm, oc):
    xyz = synth.plane_patch(30_000, seed=3, normal=(0, 0, 1), offset=-1.2, half=3.0)
    with gm.GeometricMappingGroup([0, 0], loopback=True, flags=BASE, **KW) as g:
        res = g.process_frame(xyz)
        f = g.fit_cylinder()
        cloud, _ = g.cropped_cloud()
        lab = g.labels()
        _same_fit(f, g.last_cylinder_fit())
    assert f["status"] == _lib.GM_FIT_NO_MODEL and not f["ok"] and f["passes"] == 0 and f["inliers"] == 0
    assert np.isnan(f["radius"]) and np.isnan(f["point"]).all() and np.isnan(f["model"]).all()
    assert res["plane_inliers"] > 0
    assert np.array_equal(lab, _plane_labels(oc, cloud, res))


def test_not_ready_without_a_sharded_frame(gm):
    xyz = synth.tunnel_frame(60_000, seed=11, floor_z=FLOOR, outlier_frac=0.01)
    with gm.GeometricMappingGroup([0, 0], loopback=True, flags=BASE, neighborRadius=0.4, **KW) as g:
        for call in (g.fit_cylinder, g.last_cylinder_fit, g.labels):
            with pytest.raises(gm.GmError) as e:
                call()
            assert e.value.status == _lib.GM_ERR_NOT_READY
        g.process_frame(xyz)
        with pytest.raises(gm.GmError) as e:
            g.last_cylinder_fit()                                      # no fit of this frame yet
        assert e.value.status == _lib.GM_ERR_NOT_READY
        assert g.fit_cylinder()["ok"]
        g.submit_frame(xyz)                                            # a streamed frame takes slot 0 of a rank
        for call in (g.fit_cylinder, g.last_cylinder_fit, g.labels):
            with pytest.raises(gm.GmError) as e:
                call()
            assert e.value.status == _lib.GM_ERR_NOT_READY
        g.wait_frame()
