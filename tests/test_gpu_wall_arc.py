"""GPU tests of the wall map on a circular-arc design axis (gm_wall_map_create_arc): add, checked add, check, cloud and
mesh against the twin tests/wall_arc_np.py, and the integer rule of tests/wall_np.py byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_wall_map as twm  # noqa: E402  (GRIDS and the rebuild rule)
import wall_add_checked_np as an  # noqa: E402
import wall_arc_np as wa  # noqa: E402
import wall_check_np as kn  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
OBLIQUE = (0.0, 0.6, 0.8)
CURVES = {
    "horizontal_80": dict(arc_radius=80.0, toward=(0.0, 1.0, 0.0)),
    "vertical_300": dict(arc_radius=300.0, toward=(0.0, 0.0, -1.0)),
    "oblique": dict(arc_radius=120.0, toward=OBLIQUE, yaw_deg=8.0, roll_deg=6.0, lateral=0.4),
}


def _arc_frame(m, pose):
    """The frame the library reports for this map and pose (gm_wall_arc_add_frame), as the twin's points() takes it."""
    return api.wall_arc_add_frame(m.prm, m.arc_struct(), pose)


def _against_twin(m, info, res, cell, xyz, labels, pose, p, arc):
    f = _arc_frame(m, pose)
    w = wa.add_frame(wa.design(p, arc), p, pose)
    assert info["anchor_station"] == f["anchor_station"] == w["anchor"]
    for k in ("o", "a"):
        assert np.array_equal(info[k].view(np.uint32), f[k].view(np.uint32)), k
    for k in ("o", "a", "u", "v"):
        assert np.abs(info[k].astype(np.float64) - w[k]).max() <= 1e-6, k
    assert float(info["R"]) == w["R"] and float(info["station_length"]) == w["ds"] and float(info["gate"]) == w["gate"]
    r = wa.points(xyz, labels, f, p)
    fin = np.isfinite(r["e"])
    assert np.array_equal(fin, np.isfinite(res))
    err = np.abs(res[fin].astype(np.float64) - r["e"][fin]).max()
    amb = r["ambiguous"]
    share = 1.0 - amb.mean()
    print(f"arc twin: n={len(xyz)} max|e-e_twin|={err:.3e} non-ambiguous={share:.5f}")
    assert err <= 5e-6
    assert share > 0.99
    assert np.array_equal(cell[~amb].astype(np.int64), r["cell"][~amb])
    return r


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_twin(gm, curve):
    drive = synth.arc_drive(3, 4000, seed=11, **CURVES[curve])
    p = wn.params(n_stations=200, **drive["design"])
    with gm.GeometricMapping() as c:
        for cloud, pose in drive["frames"]:
            m = c.wall_map(arc=drive["arc"], **p)
            assert np.allclose(m.arc["curvature"], drive["arc"]["curvature"]) and m.arc["point_chainage"] == 0.0
            lab = (np.arange(len(cloud)) % 11 == 0).astype(np.uint8)
            info, res, cell = m.add_points(cloud, pose, labels=lab)
            r = _against_twin(m, info, res, cell, cloud, lab, pose, p, drive["arc"])
            twm._check_class_counts(m.info(), r)
            assert m.info()["mapped"] > 0.85 * len(cloud)
            m.close()


SIZES = (0, 1, 63, 64, 65, 2049, 20_000)


@pytest.mark.parametrize("grid", sorted(twm.GRIDS))
def test_exact_rebuild(gm, grid):
    # a 400 m radius: the default grid's 1000 m of map stay within |psi| <= 3
    drive = synth.arc_drive(len(SIZES), 20_000, seed=5, arc_radius=400.0, toward=OBLIQUE)
    p = wn.params(**dict(drive["design"], **twm.GRIDS[grid]))
    with gm.GeometricMapping() as c:
        m = c.wall_map(arc=drive["arc"], **p)
        es, cs, total, planes = [], [], 0, 0
        for k, ((cloud, pose), n) in enumerate(zip(drive["frames"], SIZES)):
            xyz = cloud[:n]
            lab = (np.arange(n) % 7 == 0).astype(np.uint8) if k % 2 else None   # some "plane" points
            _, res, cell = m.add_points(xyz, pose, labels=lab)
            if lab is not None:
                assert np.all(np.isnan(res[lab == 1])) and np.all(cell[lab == 1] == -1)
                planes += int(lab.sum())
            es.append(res)
            cs.append(cell)
            total += n
        i = twm._rebuild(m, p, es, cs, total)
        assert i["frames"] == len(SIZES) and i["plane"] == planes and i["mapped"] > 0.5 * total


def test_frame_path_equals_stage_path(gm, tmp_path):
    n = 20_000
    drive = synth.arc_drive(4, n, seed=9, arc_radius=80.0, toward=OBLIQUE, lateral=0.1)
    p = wn.params(n_stations=200, **drive["design"])
    kw = dict(neighborRadius=synth.fixed_k_radius(n))
    with gm.GeometricMapping(n_slots=2, **kw) as c:
        m = c.wall_map(arc=drive["arc"], **p)
        valid = []
        for k, (cloud, pose) in enumerate(drive["frames"]):
            c.submit_frame(k % 2, cloud)
            m.add_frame(k % 2, pose)
            c.wait_frame(k % 2)
            valid.append(c.cropped_cloud(k % 2)[0])
        m.sync()
        ref, info = m.read_raw().tobytes(), m.info()
        assert info["frames"] == 4 and info["mapped"] > 0.5 * sum(len(v) for v in valid)
        s = c.wall_map(arc=drive["arc"], **p)
        for xyz, (_, pose) in zip(valid, drive["frames"]):
            s.add_points(xyz, pose, outputs=False)
        assert s.read_raw().tobytes() == ref
        si = s.info()
        for k in ("mapped", "outside", "beyond_gate", "plane", "cells_hit", "frames"):
            assert si[k] == info[k], k
        # a saved map comes back on its arc
        path = str(tmp_path / "arc.npz")
        s.save(path)
        b = gm.WallMap.load(c, path)
        assert b.read_raw().tobytes() == ref and bytes(b.arc_struct()) == bytes(m.arc_struct())
        b.regions(baseline=m)


def test_analytic_tube(gm):
    """sigma = 0: every point lies exactly on an 80 m-radius tube with two patches.  1e-5 m: the chain's 5e-6 m plus the
    rounding of the fp32 inputs."""
    NST = 200
    patches = synth.DRIVE_PATCHES[:2]
    drive = synth.arc_drive(12, 60_000, seed=21, arc_radius=80.0, toward=(0.0, 1.0, 0.0), sigma=0.0, patches=patches)
    p = wn.params(n_stations=NST, **drive["design"])
    with gm.GeometricMapping() as c:
        m, straight = c.wall_map(arc=drive["arc"], **p), c.wall_map(**p)
        n = 0
        for cloud, pose in drive["frames"]:
            m.add_points(cloud, pose, outputs=False)
            straight.add_points(cloud, pose, outputs=False)
            n += len(cloud)
        count, mean, _, _ = (x.reshape(NST, 90) for x in m.read())
        i, si = m.info(), straight.info()
    assert i["mapped"] > 0.99 * n
    inside = np.zeros(count.shape, bool)
    for t0, t1, p0, p1, dr in patches:
        js, ks = slice(int(t0 / 0.25), int(t1 / 0.25)), slice(int(p0 / 4), int(p1 / 4))
        assert np.all(count[js, ks] > 0)
        worst = np.abs(mean[js, ks].astype(np.float64) - dr).max()
        print(f"analytic: patch dr={dr} worst |mean - dr| = {worst:.3e}")
        assert worst <= 1e-5
        inside[js, ks] = True
    rest = ~inside & (count > 0)
    assert rest.sum() > 10_000
    worst = np.abs(mean[rest].astype(np.float64)).max()
    print(f"analytic: {rest.sum()} cells elsewhere, worst |mean| = {worst:.3e}")
    assert worst <= 1e-5
    # the assertion that shows the feature: against the straight design cylinder the curved tube is mostly beyond the gate
    print(f"straight map on the same frames: beyond_gate {si['beyond_gate']} of {n}")
    assert si["beyond_gate"] > n // 2


def test_chainage(gm):
    """The same cloud under a pose and under that pose carried 4000 stations (1000 m) along a 500 m-radius arc."""
    p = wn.params(n_stations=4200, t_min=-20.0)
    arc = dict(curvature=(0.0, 0.0012, 0.0016), point_chainage=500.0)
    D = wa.design(p, arc)
    o, a, u, v = wa.frame(D, 10.1)
    local = synth.pose_matrix((0, 0, 0), yaw_deg=5.0, roll_deg=3.0)[:, :3]
    p0 = np.concatenate([np.stack([a, -v, u], axis=1) @ local, (o + 0.2 * u + 0.1 * v).reshape(3, 1)], axis=1)
    ang = D["kappa"] * 1000.0     # about b through C, turning a toward n
    b = D["b"]
    K = np.array([[0.0, -b[2], b[1]], [b[2], 0.0, -b[0]], [-b[1], b[0], 0.0]])
    Rot = np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)
    p1 = np.concatenate([Rot @ p0[:, :3], (D["C"] + Rot @ (p0[:, 3] - D["C"])).reshape(3, 1)], axis=1)
    rng = np.random.default_rng(13)
    t, phi = rng.uniform(10.1 - 4.5, 10.1 + 4.5, 6000), rng.uniform(0.0, 2 * np.pi, 6000)
    world = wa.point(D, t, phi, 2.0 + rng.normal(0.0, 0.01, 6000))
    cloud = np.ascontiguousarray(((world - p0[:, 3]) @ p0[:, :3]).astype(np.float32))
    with gm.GeometricMapping() as c:
        m = c.wall_map(arc=arc, **p)
        i0, e0, c0 = m.add_points(cloud, p0)
        i1, e1, c1 = m.add_points(cloud, p1)
        assert i1["anchor_station"] - i0["anchor_station"] == 4000
        fin = np.isfinite(e0)
        assert np.array_equal(fin, np.isfinite(e1)) and np.abs(e0[fin].astype(np.float64) - e1[fin]).max() <= 5e-6
        amb = (wa.points(cloud, None, _arc_frame(m, p0), p)["ambiguous"] | wa.points(cloud, None, _arc_frame(m, p1), p)["ambiguous"])
        assert (1.0 - amb.mean()) > 0.99
        both = ~amb & (c0 >= 0)
        assert both.mean() > 0.9 and np.array_equal(c0[~amb] >= 0, c1[~amb] >= 0)
        assert np.all(c1[both].astype(np.int64) - c0[both] == 4000 * 90)


def test_check_and_checked_add(gm):
    n = 5000
    kw = dict(arc_radius=80.0, toward=OBLIQUE)
    survey = synth.arc_drive(4, 20_000, seed=3, patches=(), **kw)
    drive = synth.arc_drive(4, n, seed=3, **kw)            # the same poses; the wall moved inside the patches
    p = wn.params(n_stations=200, **drive["design"])
    ck = dict(threshold=0.004, min_count=2)
    seen = dict(pos=0, neg=0, skipped=0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(arc=drive["arc"], **p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        raw = m.read_raw()
        before = raw.tobytes()
        for k, (cloud, pose) in enumerate(drive["frames"]):
            lab = (np.arange(n) % 7 == 0).astype(np.uint8) if k % 2 else None
            info, rows, out = m.check_points(cloud, pose, labels=lab, **ck)
            e, cell, delta, cls = (out[k_] for k_ in ("e", "cell", "delta", "cls"))
            # the chain: the check's (e, cell) against the fp64 twin under the check's own gate
            r = wa.points(cloud, lab, _arc_frame(m, pose), p, gate=kn.DEFAULTS["gate"])
            fin = np.isfinite(r["e"])
            assert np.array_equal(fin, np.isfinite(e)) and np.abs(e[fin].astype(np.float64) - r["e"][fin]).max() <= 5e-6
            assert np.array_equal(cell[~r["ambiguous"]].astype(np.int64), r["cell"][~r["ambiguous"]])
            # the rule: the existing check twin fed the arc chain's (e, cell)
            winfo, wrows = kn.check(cloud, e, cell, raw, labels=lab, status=info["status"], **ck)
            wdelta, wcls = kn.classify(e, cell, raw, lab, **ck)
            assert np.array_equal(cls, wcls) and np.array_equal(delta.astype(np.int64), np.clip(wdelta, -2 ** 31, 2 ** 31 - 1))
            assert rows.tobytes() == wrows.tobytes()
            for key in winfo:
                assert info[key] == winfo[key], key
            seen["pos"] += info["changed_pos"]
            seen["neg"] += info["changed_neg"]
            # the checked add: the bytes of a plain add of the cloud with the skipped rows deleted
            a, b = c.wall_map(arc=drive["arc"], **p), c.wall_map(arc=drive["arc"], **p)
            a.add_raw(raw)
            b.add_raw(raw)
            ainfo, res, acell = a.add_points_checked(cloud, pose, rows, labels=lab, min_delta=0.012)
            _, skipped = an.select(rows, n, min_delta=0.012)
            keep = an.keep(n, skipped)
            _, pe, pc = b.add_points(cloud[keep], pose, labels=None if lab is None else lab[keep])
            assert a.read_raw().tobytes() == b.read_raw().tobytes()
            assert ainfo["skipped"] == len(skipped) and np.all(acell[~keep] == -1) and np.array_equal(acell[keep], pc)
            assert np.array_equal(res[keep].view(np.uint32), pe.view(np.uint32))
            ia, ib = a.info(), b.info()
            for key in ("mapped", "outside", "beyond_gate", "plane", "cells_hit"):
                assert ia[key] == ib[key], key
            seen["skipped"] += len(skipped)
            a.close()
            b.close()
        assert m.read_raw().tobytes() == before            # a check reads
        print(seen)
        assert seen["pos"] > 50 and seen["neg"] > 50 and seen["skipped"] > 50


EDGE_SIZES = (0, 1, 63, 64, 65, 1025, 2049)   # one 1024-thread block: its stride plus 1, two strides plus 1


@pytest.mark.parametrize("axis", ["arc", "straight"])
def test_checked_add_at_trip_and_window_edges(gm, monkeypatch, axis):
    """The masked add on both axes at the edges of its point stream -- no point, a last wave with lanes past n, a trip
    whose second slot lies wholly past n -- on two-centimetre stations, where the LDS window holds the 11 stations around
    the anchor and the rest of the 5 m box goes to the map directly.  Every third point is a selected row; the map, the
    per-point outputs and the counts are those of the plain add of the points that stay (the twin's selection)."""
    monkeypatch.setenv("GM_WALL_POINTS_PER_BLOCK", "4096")   # read when a map is created: one block for every size here
    n_max = max(EDGE_SIZES)
    if axis == "arc":
        drive = synth.arc_drive(len(EDGE_SIZES), n_max, seed=5, arc_radius=400.0, toward=OBLIQUE)
        kw = dict(arc=drive["arc"])
    else:
        drive = synth.tunnel_drive(len(EDGE_SIZES), n_max, seed=5)
        kw = dict()
    p = wn.params(**dict(drive["design"], **twm.GRIDS["fine_stations"]))
    nsec = p["n_sectors"]
    wmax = 4096 // nsec                                     # the window: stations [-(wmax // 2), wmax - wmax // 2) from the anchor
    sides = np.zeros(2, np.int64)
    with gm.GeometricMapping() as c:
        for (cloud, pose), n in zip(drive["frames"], EDGE_SIZES):
            xyz = np.ascontiguousarray(cloud[:n])
            lab = (np.arange(n) % 7 == 0).astype(np.uint8)
            rows = np.zeros(len(range(1, n, 3)), kn.POINT)
            rows["index"] = np.arange(1, n, 3)
            rows["delta"] = np.where(rows["index"] % 2 == 0, 1.0, -1.0)
            a, b = c.wall_map(**kw, **p), c.wall_map(**kw, **p)
            info, res, cell = a.add_points_checked(xyz, pose, rows, labels=lab)
            _, skipped = an.select(rows, n)
            keep = an.keep(n, skipped)
            binfo, pe, pc = b.add_points(xyz[keep], pose, labels=lab[keep])
            assert a.read_raw().tobytes() == b.read_raw().tobytes()
            assert info["n_points"] == n and info["n_rows"] == len(rows) and info["skipped"] == len(skipped) == len(rows)
            assert np.all(cell[:n][~keep] == -1) and np.array_equal(cell[:n][keep], pc[:keep.sum()])
            assert np.array_equal(res[:n][keep].view(np.uint32), pe[:keep.sum()].view(np.uint32))
            ia, ib = a.info(), b.info()
            for key in ("mapped", "outside", "beyond_gate", "plane"):
                assert info[key] == ia[key] == ib[key], key
            assert ia["cells_hit"] == ib["cells_hit"] and info["plane"] == int(lab[keep].sum())
            rel = pc[:keep.sum()][pc[:keep.sum()] >= 0].astype(np.int64) // nsec - binfo["anchor_station"]
            inside = (rel >= -(wmax // 2)) & (rel < wmax - wmax // 2)
            if n >= 1025:
                assert inside.sum() > 0 and (~inside).sum() > 0, (n, inside.sum())
            sides += (inside.sum(), (~inside).sum())
            if n == 0:                                      # and the check of no point, on this axis
                cinfo, crows, _ = a.check_points(xyz, pose, outputs=False)
                assert len(crows) == 0 and cinfo["n_points"] == 0
            a.close()
            b.close()
    print(f"{axis}: {sides[0]} mapped points inside the LDS window, {sides[1]} outside it")
    assert sides[0] > 10 and sides[1] > 1000


@pytest.mark.parametrize("blocks", [(1, 1), (3, 4)])
def test_cloud_and_mesh(gm, blocks):
    bs, bk = blocks
    drive = synth.arc_drive(3, 20_000, seed=7, arc_radius=80.0, toward=OBLIQUE, start=6.0, step=3.0)
    p = wn.params(n_stations=80, **drive["design"])
    D = wa.design(p, drive["arc"])
    station0, n = 10, 41                                   # 10.25 m of map; a ragged last block row
    mid = p["t_min"] + (station0 + n / 2) * p["station_length"]
    anchor = tuple(np.round(wa.frame(D, mid)[0], 3))       # |coordinates| < 8 m: half an fp32 ulp is 2.4e-7 m
    prm = dict(block_stations=bs, block_sectors=bk, anchor=anchor, min_count=2)
    os.environ["GM_WALL_CLOUD_CHUNK"] = str(4 * (90 // bk + 1))   # a few block rows per chunk: the row table of a later chunk
    try:
        with gm.GeometricMapping() as c:
            m = c.wall_map(arc=drive["arc"], **p)
            for cloud, pose in drive["frames"]:
                m.add_points(cloud, pose, outputs=False)
            raw = m.read_raw()
            tab = api.wall_cloud_directions(m.prm, **prm)
            info, rec = m.cloud(station0, n, **prm)
            winfo, wrec = wa.cloud(raw, p, drive["arc"], station0, n, directions=tab, **prm)
            assert info == winfo and info["points"] > 0.8 * info["blocks"]
            for f in ("x", "y", "z"):
                assert np.array_equal(rec[f].view(np.uint32), wrec[f].view(np.uint32)), f
            assert rec.tobytes() == wrec.tobytes()
            minfo, v, tri = m.mesh(station0, n, **prm)
            assert v.tobytes() == rec.tobytes() and minfo["cloud"] == info
            tinfo, wtri = api.wall_mesh_triangulate(info["blocks_stations"], info["blocks_sectors"], v)
            assert tri.tobytes() == wtri.tobytes() and len(tri) > info["points"]
            for key in ("wrapped", "quads", "quads_two", "quads_one", "quads_none", "triangles"):
                assert minfo[key] == tinfo[key], key
            # every vertex lies at its block's centre chainage and angle, at rho = R + mean
            xyz = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64) + np.asarray(anchor)
            s, phi, e = api.wall_arc_project(m.prm, m.arc_struct(), xyz)
            NK = info["blocks_sectors"]
            J, K = v["block"].astype(np.int64) // NK, v["block"].astype(np.int64) % NK
            j0 = station0 + J * bs
            tc = p["t_min"] + (2 * j0 + np.minimum(bs, station0 + n - j0)) * 0.5 * p["station_length"]
            nk = np.minimum(bk, 90 - K * bk)
            pc = 2 * np.pi * (2 * K * bk + nk) / (2.0 * 90)
            dphi = np.abs(np.mod(phi - pc + np.pi, 2 * np.pi) - np.pi)
            print(f"vertices: max |s - tc| = {np.abs(s - tc).max():.2e} m, max |phi - phi_c| = {dphi.max():.2e} rad")
            assert np.abs(s - tc).max() <= 1e-6 and dphi.max() <= 1e-6
            assert np.abs(e - v["mean"].astype(np.float64)).max() <= 1e-6
    finally:
        os.environ.pop("GM_WALL_CLOUD_CHUNK", None)


def test_refusals_and_straight_maps_beside(gm):
    drive = synth.arc_drive(2, 4000, seed=2, arc_radius=80.0)
    sdrive = synth.tunnel_drive(2, 4000, seed=2)
    p = wn.params(n_stations=200, **drive["design"])
    U, I = _lib.GM_ERR_UNSUPPORTED, _lib.GM_ERR_INVALID_ARG
    with gm.GeometricMapping() as c:
        m = c.wall_map(arc=drive["arc"], **p)
        straight = c.wall_map(**p)
        assert straight.arc is None and m.arc is not None
        cloud, pose = drive["frames"][0]
        m.add_points(cloud, pose, outputs=False)
        before = m.read_raw().tobytes()
        for call in (m.locate_points, m.align_points):
            with pytest.raises(_lib.GmError) as ex:
                call(cloud, pose)
            assert ex.value.status == U
        c.process_frame(cloud)
        for call in (m.locate_frame, m.align_frame):
            with pytest.raises(_lib.GmError) as ex:
                call(0, pose)
            assert ex.value.status == U
        assert m.read_raw().tobytes() == before
        # a baseline must be a map on the same arc
        other = c.wall_map(arc=dict(curvature=(0.0, 1 / 81.0, 0.0), point_chainage=0.0), **p)
        same = c.wall_map(arc=drive["arc"], **p)
        for base in (other, straight):
            with pytest.raises(_lib.GmError) as ex:
                m.regions(baseline=base)
            assert ex.value.status == I
        with pytest.raises(_lib.GmError) as ex:
            straight.regions(baseline=m)
        assert ex.value.status == I
        m.regions(baseline=same)
        # gm_wall_map_create_arc's limits
        for bad in (dict(curvature=(0.0, 1 / 1.1e6, 0.0), point_chainage=0.0), dict(curvature=(0.0, 1 / 4.4, 0.0), point_chainage=0.0),
                    dict(curvature=(0.0, 1 / 16.0, 0.0), point_chainage=0.0), dict(curvature=(0.0, float("nan"), 0.0), point_chainage=0.0),
                    dict(curvature=(0.0, 0.01, 0.0), point_chainage=float("inf")), dict(curvature=(0.3, 0.0, 0.0), point_chainage=0.0)):
            with pytest.raises(_lib.GmError) as ex:
                c.wall_map(arc=bad, **p)
            assert ex.value.status == I
        h = C.c_void_p()
        assert c._L.gm_wall_map_create_arc(c._ctx, C.byref(m.prm), None, C.byref(h)) == I and not h.value
        # straight maps created beside arc maps still follow test_exact_rebuild's rule
        sp = wn.params(n_stations=200, **sdrive["design"])
        s2 = c.wall_map(**sp)
        es, cs = [], []
        for xyz, ps in sdrive["frames"]:
            i, res, cell = s2.add_points(xyz, ps)
            twm._check_against_twin(i, res, cell, xyz, None, ps, sp)
            es.append(res)
            cs.append(cell)
        twm._rebuild(s2, sp, es, cs, 8000)
