"""GPU tests of the cylinder regression (GM_CFG_CYLINDER_FIT, csrc/k_cylfit.hip): analytic truth of the synthetic
frames, agreement with the fp64 numpy twin (tests/cylfit_np.py) on the device's own cloud, labels bit for bit against the
oracle's fp32 predicate on the published row, nothing else of the frame changed, determinism over every pipeline path,
the gm_fit_cylinder stage call, edge cases.  The reference's getCylinder is an empty stub
(/root/reference src/tunnel_processing.cpp:149-154): truth here is the generator's, never "vs reference"."""
import ctypes as C
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
FIT = _lib.GM_CFG_CYLINDER_FIT


def _run(gm, xyz, flags, **kw):
    with gm.GeometricMapping(flags=flags, ransac_hypotheses=H, ransac_threshold=TAU, ransac_seed=SEED, **kw) as c:
        res = c.process_frame(xyz)
        out = dict(res=res, cloud=c.cropped_cloud(), normals=c.normals(), labels=c.labels(), map=c.compressed_map())
        if flags & _lib.GM_CFG_VOXEL_GRID:
            out["voxels"] = c.voxel_centroids()
        if flags & _lib.GM_CFG_NEAREST:
            out["nearest"] = c.voxel_nearest()
        if flags & FIT:
            out["fit"] = c.cylinder_fit()
        else:
            with pytest.raises(gm.GmError) as e:
                c.cylinder_fit()
            assert e.value.status == _lib.GM_ERR_UNSUPPORTED
    return out


def _frames():
    tun = synth.tunnel_frame(1_000_000, seed=2, floor_z=FLOOR, outlier_frac=0.01)
    vel = synth.velodyne_tunnel(rings=64)["xyz"]
    return {"tunnel": (tun, (0.0, 0.0, 0.0)), "velodyne": (vel, (0.0, 0.3, 0.5))}


@pytest.fixture(scope="module")
def runs(gm):
    out = {}
    for name, (xyz, origin) in _frames().items():
        kw = dict(neighborRadius=synth.fixed_k_radius(len(xyz))) if name == "tunnel" else {}
        on = _run(gm, xyz, BASE | _lib.GM_CFG_NEAREST | FIT, **kw)
        off = _run(gm, xyz, BASE | _lib.GM_CFG_NEAREST, **kw)
        out[name] = (xyz, origin, on, off)
    return out


def _errors(point, axis, radius, origin):
    return (abs(radius - 2.0), cf.axis_angle(axis, [1, 0, 0]), cf.line_distance(point, origin, [1, 0, 0]))


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
def test_fit_meets_analytic_truth(runs, name):
    xyz, origin, on, _ = runs[name]
    f, res = on["fit"], on["res"]
    assert f["ok"] and f["converged"] and f["passes"] == 3, f
    err = _errors(f["point"], f["axis"], f["radius"], origin)
    assert err[0] < 1e-3 and err[1] < 1e-3 and err[2] < 2e-3, err
    hyp = res["cylinder"].astype(np.float64)
    herr = _errors(hyp[:3], hyp[3:6], hyp[6], origin)
    assert all(e < h for e, h in zip(err, herr)), (err, herr)        # better than the hypothesis on every count
    assert np.dot(f["axis"], hyp[3:6]) > 0
    # the true wall inside the crop box: |rho_true - 2| < tau, not taken by the plane -> labelled 2
    cloud, rows = on["cloud"]
    assert np.array_equal(xyz[rows], cloud)                            # (pad row index maps back to the input)
    lab = on["labels"]
    rho = np.linalg.norm(xyz[rows][:, 1:].astype(np.float64) - np.asarray(origin[1:]), axis=1)
    wall = (np.abs(rho - 2.0) < TAU) & (lab != 1)
    assert wall.sum() > 1000 and (lab[wall] == 2).mean() >= 0.95, (lab[wall] == 2).mean()
    assert f["inliers"] == int((lab == 2).sum())


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
def test_fit_matches_numpy_twin_and_oracle_labels(runs, oc, name):
    _, _, on, off = runs[name]
    f = on["fit"]
    cloud = off["cloud"][0]
    pre = off["labels"]
    tw = cf.fit_cylinder(cloud, off["res"]["cylinder"], TAU, pre != 1)
    assert tw["status"] == f["status"]
    assert abs(f["radius"] - tw["radius"]) < 1e-6 * tw["radius"]
    assert np.abs(f["point"] - tw["point"]).max() < 1e-6 * max(1.0, np.abs(tw["point"]).max())
    assert cf.axis_angle(f["axis"], tw["axis"]) < 1e-7 and np.dot(f["axis"], tw["axis"]) > 0
    # labels: the oracle's fp32 predicate on the published row, bit for bit
    ref = pre.copy()
    ref[ref == 2] = 0
    n = oc.label_cylinder(cloud, ref, 0, 2, f["model"], TAU)
    assert n == f["inliers"] and np.array_equal(on["labels"], ref)
    m = np.asarray(f["model"], np.float64)
    assert abs(np.linalg.norm(m[3:6]) - 1) < 1e-6 and np.abs(m[:3] - np.asarray(f["point"])).max() < 10.0


@pytest.mark.parametrize("name", ["tunnel", "velodyne"])
def test_flag_changes_nothing_else(runs, gm, name):
    _, _, on, off = runs[name]
    a, b = on["res"], off["res"]
    for k in a:
        if k in ("stage_ms", "normals_kernel_ms"):
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    for k in ("cloud", "voxels"):
        for x, y in zip(on[k], off[k]):
            assert np.array_equal(x, y), k
    assert np.array_equal(on["normals"], off["normals"], equal_nan=True)
    assert np.array_equal(on["nearest"], off["nearest"])
    assert np.array_equal(on["labels"] == 1, off["labels"] == 1)
    ma, mb = gm.decode_compressed_map(on["map"]), gm.decode_compressed_map(off["map"])
    assert len(on["map"]) == len(off["map"])
    assert ma["n_points"] == mb["n_points"] and np.array_equal(ma["voxels"], mb["voxels"])
    assert np.array_equal(ma["eigenvalues"], mb["eigenvalues"]) and np.array_equal(ma["center_axis"], mb["center_axis"])
    assert [p["type"] for p in ma["primitives"]] == [p["type"] for p in mb["primitives"]] == [1, 2]
    p1a, p1b = ma["primitives"][0], mb["primitives"][0]
    assert p1a["inliers"] == p1b["inliers"] and np.array_equal(p1a["params"], p1b["params"])
    p2a, p2b = ma["primitives"][1], mb["primitives"][1]
    assert np.array_equal(p2a["params"], on["fit"]["model"]) and p2a["inliers"] == on["fit"]["inliers"]
    assert np.array_equal(p2b["params"], off["res"]["cylinder"]) and p2b["inliers"] == off["res"]["cylinder_inliers"]
    # the rest of the map bytes are the same
    hdr = 56 + 40
    assert np.array_equal(on["map"][:hdr], off["map"][:hdr]) and np.array_equal(on["map"][hdr + 40:], off["map"][hdr + 40:])


def _same_fit(a, b):
    for k in ("status", "inliers", "passes", "radius", "rms", "last_step"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in ("point", "axis", "model"):
        assert np.array_equal(a[k], b[k]), k


def test_fit_is_bit_identical_across_pipeline_paths(gm):
    xyz = synth.tunnel_frame(200_000, seed=5, floor_z=FLOOR, outlier_frac=0.01)
    kw = dict(ransac_hypotheses=256, ransac_threshold=TAU, ransac_seed=SEED)
    flags = BASE | FIT
    with gm.GeometricMapping(flags=flags, **kw) as c:
        c.process_frame(xyz)
        ref, ref_lab = c.cylinder_fit(), c.labels()
        c.process_frame(xyz)
        _same_fit(ref, c.cylinder_fit())
        assert np.array_equal(ref_lab, c.labels())
    assert ref["ok"]
    with gm.GeometricMapping(flags=flags | _lib.GM_CFG_GRAPH, **kw) as c:
        for _ in range(3):                                            # capture, then replays
            c.process_frame(xyz)
            _same_fit(ref, c.cylinder_fit())
            assert np.array_equal(ref_lab, c.labels())
    with gm.GeometricMapping(flags=flags, n_slots=4, **kw) as c:
        for s in range(4):
            c.submit_frame(s, xyz)
        for s in range(4):
            c.wait_frame(s)
            _same_fit(ref, c.cylinder_fit(s))
            assert np.array_equal(ref_lab, c.labels(s))
    with gm.GeometricMappingGroup([0, 0], loopback=True, n_slots=2, flags=flags, **kw) as g:
        for _ in range(4):
            g.submit_frame(xyz)
        seen = set()
        while g.in_flight():
            _, rank, slot = g.wait_frame()
            seen.add(rank)
            if rank == 0:                                             # rank r draws with seed + r
                _same_fit(ref, g.cylinder_fit(rank, slot))
        assert seen == {0, 1}
        with pytest.raises(gm.GmError) as e:
            g.process_frame(xyz)
        assert e.value.status == _lib.GM_ERR_UNSUPPORTED


def test_stage_call_reproduces_the_frame_fit(gm, runs):
    _, _, on, off = runs["velodyne"]
    cloud = off["cloud"][0]
    lab = off["labels"].copy()
    lab[lab == 2] = 0
    with gm.GeometricMapping() as c:
        f, mask = c.getCylinder(cloud, off["res"]["cylinder"], TAU, lab, 0)
    _same_fit(on["fit"], f)
    assert np.array_equal(mask, on["labels"] == 2)


def test_stage_call_from_a_perturbed_start_on_a_half_arc(gm, oc):
    xyz = synth.cylinder_frame(120_000, seed=9)
    xyz = xyz[(xyz[:, 2] > 0) & (np.abs(xyz[:, 0]) < 5.0)]            # the upper half of the tube only
    init = cf.perturbed_init([0, 0, 0], [1, 0, 0], 2.0, dr=0.05, tilt=0.04, shift=0.05)
    with gm.GeometricMapping() as c:
        f, mask = c.getCylinder(xyz, init, TAU)
    assert f["ok"] and f["converged"], f
    err = _errors(f["point"], f["axis"], f["radius"], (0, 0, 0))
    assert err[0] < 1e-3 and err[1] < 1e-3 and err[2] < 2e-3, err
    ref = np.zeros(len(xyz), np.uint8)
    assert oc.label_cylinder(xyz, ref, 0, 1, f["model"], TAU) == f["inliers"] == int(mask.sum())
    assert np.array_equal(mask, ref == 1)
    tw = cf.fit_cylinder(xyz, init, TAU)
    assert abs(f["radius"] - tw["radius"]) < 1e-6 * 2 and cf.axis_angle(f["axis"], tw["axis"]) < 1e-6


def test_plane_only_cloud_has_no_model_and_keeps_labels(gm):
    xyz = synth.plane_patch(30_000, seed=3, normal=(0, 0, 1), offset=-1.2, half=3.0)
    on = _run(gm, xyz, BASE | FIT)
    off = _run(gm, xyz, BASE)
    f = on["fit"]
    assert f["status"] == _lib.GM_FIT_NO_MODEL and not f["ok"] and f["passes"] == 0
    assert np.isnan(f["radius"]) and np.isnan(f["point"]).all() and np.isnan(f["model"]).all()
    assert np.array_equal(on["labels"], off["labels"]) and np.array_equal(on["map"], off["map"])


def test_stage_call_edge_sizes(gm, oc):
    base = synth.cylinder_frame(600_000, seed=4)
    init = cf.perturbed_init([0, 0, 0], [1, 0, 0], 2.0, dr=0.02, tilt=0.01, shift=0.02)
    with gm.GeometricMapping() as c:
        # fewer than 5 eligible points: degenerate, nothing marked
        lab = np.ones(5000, np.uint8)
        lab[[3, 100, 2000, 4999]] = 0
        f, mask = c.getCylinder(base[:5000], init, TAU, lab, 0)
        assert f["status"] == _lib.GM_FIT_DEGENERATE and np.isnan(f["radius"]) and not mask.any()
        for n in (0, 1, 4):
            f, mask = c.getCylinder(base[:n], init, TAU)
            assert f["status"] == _lib.GM_FIT_DEGENERATE and len(mask) == n and not mask.any()
        # around a block (256), the fixed grid's row (512 * 256 points) and its four-point trip
        for n in (255, 256, 257, 131_071, 131_072, 131_073, 524_289):
            xyz = base[:n]
            f, mask = c.getCylinder(xyz, init, TAU)
            tw = cf.fit_cylinder(xyz, init, TAU)
            assert f["ok"] and tw["status"] == cf.FIT_OK, n
            assert abs(f["radius"] - tw["radius"]) < 1e-5 and cf.axis_angle(f["axis"], tw["axis"]) < 1e-5, n
            ref = np.zeros(n, np.uint8)
            assert oc.label_cylinder(xyz, ref, 0, 1, f["model"], TAU) == f["inliers"] == int(mask.sum()), n
            assert np.array_equal(mask, ref == 1), n
        with pytest.raises(gm.GmError):
            c.getCylinder(base[:100], init, 0.0)
