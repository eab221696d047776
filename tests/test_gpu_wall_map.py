"""GPU tests of the persistent wall map (gm_wall_*, csrc/k_wall.hip + gm_wall.hip): agreement with the fp64 twin
(tests/wall_np.py), every raw cell bit for bit against the integer rule applied to the device's own per-point outputs over
many adds and grids, the frame path against the stage path over every pipeline path and order, the per-frame surface map
as a special case, independence of the chainage, analytic truth of a drive with world-fixed patches, edges and failures."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_np as sn  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
SIGMA = 0.01
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
FIT = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER | _lib.GM_CFG_CYLINDER_FIT
SURF = FIT | _lib.GM_CFG_SURFACE_MAP
KW = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
IDENT = np.eye(4)[:3]


def _check_against_twin(info, res, cell, xyz, labels, pose, p):
    """One add against the twin: the reported frame, residuals, cells and class counts (the bounds of the surface map's
    twin test, which holds the same fp32 chain)."""
    f = wn.add_frame(wn.design_frame(p), p, pose)
    assert info["anchor_station"] == f["anchor"]
    for k in ("o", "a", "u", "v"):
        assert np.abs(info[k].astype(np.float64) - f[k]).max() <= 1e-6, k
    assert float(info["R"]) == f["R"] and float(info["station_length"]) == f["ds"] and float(info["gate"]) == f["gate"]
    assert float(info["sector_angle"]) == f["dtheta"]
    r = wn.points(xyz, labels, info, p)
    fin = np.isfinite(r["e"])
    assert np.array_equal(fin, np.isfinite(res))
    err = np.abs(res[fin].astype(np.float64) - r["e"][fin]).max()
    amb = r["ambiguous"]
    share = 1.0 - amb.mean()
    print(f"twin: n={len(xyz)} max|e-e_twin|={err:.3e} non-ambiguous={share:.5f}")
    assert err <= 5e-6
    assert share > 0.99
    assert np.array_equal(cell[~amb].astype(np.int64), r["cell"][~amb])
    return r


def _check_class_counts(info, r):
    """The map's totals after ONE add against the twin's classes: within the number of ambiguous points."""
    n_amb = int(r["ambiguous"].sum())
    for k, cl in (("mapped", wn.MAPPED), ("outside", wn.OUTSIDE), ("beyond_gate", wn.BEYOND), ("plane", wn.PLANE)):
        assert abs(info[k] - int((r["cls"] == cl).sum())) <= n_amb, k
    assert info["mapped"] + info["outside"] + info["beyond_gate"] + info["plane"] == len(r["cls"]) and info["frames"] == 1


def _posed_velodyne():
    """The 64-ring lidar frame under a 5 / 3 degree pose: the design is the generator's tunnel taken into the map frame."""
    xyz = synth.velodyne_tunnel(rings=64)["xyz"]
    pose = synth.pose_matrix((12.3, -0.4, 0.2), yaw_deg=5.0, roll_deg=3.0)
    design = dict(point=tuple(pose[:, :3] @ np.array([0.0, 0.3, 0.5]) + pose[:, 3]), direction=tuple(pose[:, :3] @ np.array([1.0, 0.0, 0.0])),
                  radius=2.0)
    return xyz, pose, design


def test_twin(gm):
    drive = synth.tunnel_drive(4, 200_000, seed=11)
    p = wn.params(n_stations=160, **drive["design"])
    with gm.GeometricMapping(neighborRadius=synth.fixed_k_radius(200_000)) as c:
        for cloud, pose in drive["frames"]:
            c.process_frame(cloud)
            xyz, _ = c.cropped_cloud()
            m = c.wall_map(**p)
            info, res, cell = m.add_points(xyz, pose)
            r = _check_against_twin(info, res, cell, xyz, None, pose, p)
            _check_class_counts(m.info(), r)
            assert m.info()["mapped"] > 0.9 * len(xyz)
            m.close()
        xyz, pose, design = _posed_velodyne()
        pv = wn.params(n_stations=120, **design)
        mv = c.wall_map(**pv)
        c.process_frame(xyz)
        v, _ = c.cropped_cloud()
        info, res, cell = mv.add_points(v, pose)
        r = _check_against_twin(info, res, cell, v, None, pose, pv)
        _check_class_counts(mv.info(), r)
        assert mv.info()["mapped"] > 0.3 * len(v)


GRIDS = {
    "default": dict(),
    "one_cell": dict(n_stations=1, n_sectors=1, station_length=64.0, t_min=-8.0),
    "fine_stations": dict(n_stations=2500, n_sectors=360, station_length=0.02),     # a frame's footprint exceeds the LDS window
    "max_sectors": dict(n_stations=200, n_sectors=4096),                            # one station per LDS window
}


def _rebuild(m, p, es, cs, n_points):
    nc = p["n_stations"] * p["n_sectors"]
    e, cell = np.concatenate(es), np.concatenate(cs)
    assert cell.max() < nc
    want = wn.cells_from(e, cell, nc)
    raw = m.read_raw()
    assert raw.shape == (p["n_stations"], p["n_sectors"])
    assert raw.tobytes() == want.tobytes()
    got = m.read()
    for a, b in zip(got, wn.records_from(want)):
        assert np.array_equal(a.reshape(-1).view(np.uint32), b.view(np.uint32))
    i = m.info()
    assert i["cells_hit"] == int((want["count"] > 0).sum()) and i["mapped"] == int((cell >= 0).sum())
    assert i["mapped"] + i["outside"] + i["beyond_gate"] + i["plane"] == n_points
    return i


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_exact_rebuild(gm, grid):
    drive = synth.tunnel_drive(8, 150_000, seed=5)
    p = wn.params(**dict(drive["design"], **GRIDS[grid]))
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        es, cs, n = [], [], 0
        for k, (cloud, pose) in enumerate(drive["frames"]):
            lab = (np.arange(len(cloud)) % 7 == 0).astype(np.uint8) if k % 2 else None   # some "plane" points
            _, res, cell = m.add_points(cloud, pose, labels=lab)
            if lab is not None:
                assert np.all(np.isnan(res[lab == 1])) and np.all(cell[lab == 1] == -1)
            es.append(res)
            cs.append(cell)
            n += len(cloud)
        i = _rebuild(m, p, es, cs, n)
        assert i["frames"] == 8 and i["plane"] == sum(int((np.arange(150_000) % 7 == 0).sum()) for k in range(8) if k % 2)
        assert i["mapped"] > 0.5 * n


def test_exact_rebuild_10m_frame(gm):
    big = synth.tunnel_patches(10_000_000, seed=3, floor_z=None)
    drive = synth.tunnel_drive(7, 50_000, seed=6)
    p = wn.params(n_stations=400, **drive["design"])
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        _, res, cell = m.add_points(big, synth.pose_matrix((20.0, 0.1, -0.1), yaw_deg=2.0))
        es, cs, n = [res], [cell], len(big)
        for cloud, pose in drive["frames"]:
            _, res, cell = m.add_points(cloud, pose)
            es.append(res)
            cs.append(cell)
            n += len(cloud)
        i = _rebuild(m, p, es, cs, n)
        assert i["frames"] == 8 and i["mapped"] > 0.9 * n


def _blocking(gm, clouds, poses, p, flags=_lib.GM_CFG_DEFAULT, **kw):
    """Every cloud through process_frame + add_frame on one context.  Returns the map's raw bytes, its info, and per frame
    the valid cloud and labels (None without RANSAC)."""
    valid = []
    with gm.GeometricMapping(flags=flags, **kw) as c:
        m = c.wall_map(**p)
        for cloud, pose in zip(clouds, poses):
            res = c.process_frame(cloud)
            m.add_frame(0, pose)
            xyz, _ = c.cropped_cloud()
            assert len(xyz) == res["n_valid"]
            valid.append((xyz, c.labels() if flags & _lib.GM_CFG_RANSAC_PLANE else None))
        return m.read_raw().tobytes(), m.info(), valid


def _staged(c, p, valid, poses, order=None):
    m = c.wall_map(**p)
    for k in (order if order is not None else range(len(valid))):
        m.add_points(valid[k][0], poses[k], labels=valid[k][1], outputs=False)
    return m


def test_frame_path_equals_stage_path(gm, tmp_path):
    drive = synth.tunnel_drive(8, 120_000, seed=9)
    clouds = [f[0] for f in drive["frames"]]
    poses = [f[1] for f in drive["frames"]]
    p = wn.params(n_stations=176, **drive["design"])
    kw = dict(neighborRadius=synth.fixed_k_radius(120_000))
    ref, info, valid = _blocking(gm, clouds, poses, p, **kw)
    assert info["frames"] == 8 and info["mapped"] > 0
    assert info["mapped"] + info["outside"] + info["beyond_gate"] + info["plane"] == sum(len(v[0]) for v in valid)
    # graph replays
    got, _, _ = _blocking(gm, clouds, poses, p, flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_GRAPH, **kw)
    assert got == ref
    # four streaming slots, add_frame right behind each submit, slots reused without a sync in between
    with gm.GeometricMapping(n_slots=4, **kw) as c:
        m = c.wall_map(**p)
        for k, (cloud, pose) in enumerate(zip(clouds, poses)):
            c.submit_frame(k % 4, cloud)
            m.add_frame(k % 4, pose)
        m.sync()
        assert m.read_raw().tobytes() == ref
        assert m.info()["mapped"] == info["mapped"]
    # the stage path: the same clouds and poses through add_points; reversed; two maps merged; saved and loaded
    with gm.GeometricMapping() as c:
        a = _staged(c, p, valid, poses)
        assert a.read_raw().tobytes() == ref
        ia = a.info()
        for k in ("mapped", "outside", "beyond_gate", "plane", "cells_hit", "frames"):
            assert ia[k] == info[k], k
        assert _staged(c, p, valid, poses, order=range(7, -1, -1)).read_raw().tobytes() == ref
        even, odd = _staged(c, p, valid, poses, order=range(0, 8, 2)), _staged(c, p, valid, poses, order=range(1, 8, 2))
        even.add_raw(odd.read_raw())
        assert even.read_raw().tobytes() == ref
        ie = even.info()
        assert ie["cells_hit"] == info["cells_hit"] and ie["frames"] == 4 and ie["mapped"] < info["mapped"]
        path = str(tmp_path / "wall.npz")
        a.save(path)
        recs = a.read()
    with gm.GeometricMapping() as c2:
        b = gm.WallMap.load(c2, path)
        assert b.read_raw().tobytes() == ref
        assert (b.prm.n_stations, b.prm.n_sectors, b.prm.radius) == (176, 90, 2.0)
        for x, y in zip(recs, b.read()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_plane_points_are_counted_and_touch_no_cell(gm):
    # the patch tunnel has a floor: the plane RANSAC labels it 1
    clouds = [synth.tunnel_patches(150_000, seed=s) for s in (1, 2)]
    poses = [synth.pose_matrix((6.0 + 3.0 * k, 0.0, 0.0)) for k in range(2)]
    p = wn.params(n_stations=80)
    ref, info, valid = _blocking(gm, clouds, poses, p, flags=PLANE, neighborRadius=synth.fixed_k_radius(150_000), **KW)
    n_plane = sum(int((lab == 1).sum()) for _, lab in valid)
    assert n_plane > 10_000 and info["plane"] == n_plane
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        es, cs = [], []
        for (xyz, lab), pose in zip(valid, poses):
            _, res, cell = m.add_points(xyz, pose, labels=lab)
            assert np.all(cell[lab == 1] == -1) and np.all(np.isnan(res[lab == 1]))
            es.append(res)
            cs.append(cell)
        assert m.read_raw().tobytes() == ref
        assert ref == wn.cells_from(np.concatenate(es), np.concatenate(cs), 80 * 90).tobytes()


def test_against_the_per_frame_surface_map(gm):
    xyz = synth.tunnel_patches(1_000_000, seed=2)
    kw = dict(neighborRadius=synth.fixed_k_radius(len(xyz)), **KW)

    def run(with_map):
        with gm.GeometricMapping(flags=SURF, **kw) as c:
            res = c.process_frame(xyz)
            out = dict(cloud=c.cropped_cloud(), normals=c.normals(), labels=c.labels(), cmap=c.compressed_map(),
                       fit=c.cylinder_fit(), surf=c.surface_map(), pts=c.surface_points(), n_valid=res["n_valid"])
            if with_map:
                model = out["fit"]["model"].astype(np.float64)
                p = wn.params(n_stations=40, n_sectors=90, station_length=0.25, gate=0.25, t_min=-5.0,
                              point=tuple(model[:3]), direction=tuple(model[3:6]), radius=float(model[6]))
                m = c.wall_map(**p)
                m.add_frame(0, IDENT)
                m.sync()
                out["after"] = dict(cloud=c.cropped_cloud(), normals=c.normals(), labels=c.labels(), cmap=c.compressed_map(),
                                    fit=c.cylinder_fit(), surf=c.surface_map(), pts=c.surface_points())
                out["wall_frame"] = m.read()
                m.clear()
                out["wall"] = m.add_points(out["cloud"][0], IDENT, labels=out["labels"])
                out["wall_cells"] = m.read()
                out["p"] = p
        return out

    def same(a, b):
        if isinstance(a, dict):
            assert a.keys() == b.keys()
            for k in a:
                same(a[k], b[k])
        elif isinstance(a, (tuple, list)):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                same(x, y)
        elif isinstance(a, (bytes, bytearray)):
            assert bytes(a) == bytes(b)
        else:
            assert np.array_equal(np.atleast_1d(np.asarray(a)).view(np.uint8), np.atleast_1d(np.asarray(b)).view(np.uint8))

    on, off = run(True), run(False)
    keys = ("cloud", "normals", "labels", "cmap", "fit", "surf", "pts")
    for k in keys:   # adding to a map changes nothing of the frame: after the add, and against a context with no map
        same(on[k], on["after"][k])
        same(on[k], off[k])
    sinfo, scount, smean, smin, smax = on["surf"]
    e, scell = on["pts"]
    winfo, wres, wcell = on["wall"]
    assert sinfo["status"] == _lib.GM_SURF_OK and winfo["anchor_station"] == 20
    for k in ("o", "a"):    # what the residual depends on
        assert np.array_equal(winfo[k].view(np.uint32), sinfo[k].view(np.uint32)), k
    for k in ("u", "v"):    # (a component that cancels to ~1e-27 keeps the rounding of the device's / the host's fp64 cross product)
        assert np.abs(winfo[k].astype(np.float64) - sinfo[k].astype(np.float64)).max() <= 1e-6, k
    assert float(winfo["R"]) == float(sinfo["R"])
    assert np.array_equal(wres.view(np.uint32), e.view(np.uint32))      # residuals bit-equal
    r = sn.points(on["cloud"][0], on["labels"], sinfo["o"], sinfo["a"], sinfo["u"], sinfo["v"], float(sinfo["R"]), sn.params())
    amb = r["ambiguous"]
    assert np.array_equal(wcell[~amb], scell[~amb])
    dirty = np.zeros(3600, bool)           # cells that hold an ambiguous point in either map
    for cc in (wcell[amb], scell[amb]):
        dirty[cc[cc >= 0]] = True
    clean = ~dirty
    assert clean.sum() > 1000
    for a, b in zip(on["wall_cells"], (scount, smean, smin, smax)):
        assert np.array_equal(a.reshape(-1)[clean].view(np.uint32), b.reshape(-1)[clean].view(np.uint32))
    for a, b in zip(on["wall_frame"], on["wall_cells"]):   # and the frame path gave the stage path's cells
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _wall_seen_from(p, pose, n, seed):
    """n noisy points of p's design cylinder within 6 m of the sensor's chainage, in the SENSOR coordinates of `pose`,
    cropped to the default box."""
    rng = np.random.default_rng(seed)
    D = wn.design_frame(p)
    s = (pose[:, 3] - D["o"]) @ D["a"]
    t, phi = rng.uniform(s - 6.0, s + 6.0, n), rng.uniform(0.0, 2 * np.pi, n)
    rr = D["R"] + rng.normal(0.0, SIGMA, n)
    world = D["o"] + t[:, None] * D["a"] + (rr * np.cos(phi))[:, None] * D["u"] + (rr * np.sin(phi))[:, None] * D["v"]
    cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(np.float32)
    return np.ascontiguousarray(cloud[np.all(np.abs(cloud) <= 5.0, axis=1)])


def test_chainage(gm):
    p, p0, p1 = wn.chainage_pair(20000)
    cloud = _wall_seen_from(p, p0, 300_000, seed=13)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        i0, r0, c0 = m.add_points(cloud, p0)
        i1, r1, c1 = m.add_points(cloud, p1)
        assert i1["anchor_station"] - i0["anchor_station"] == 20000
        for k in ("o", "a", "u", "v"):
            assert np.array_equal(i0[k].view(np.uint32), i1[k].view(np.uint32)), k
        assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))
        mapped = c0 >= 0
        assert mapped.mean() > 0.9 and np.array_equal(mapped, c1 >= 0)
        assert np.all(c1[mapped].astype(np.int64) - c0[mapped] == 20000 * 90)
        j0 = int(c0[mapped].min()) // 90
        n = int(c0[mapped].max()) // 90 - j0 + 1
        w0, w1 = m.read_raw(j0, n), m.read_raw(j0 + 20000, n)
        assert w0["count"].sum() == mapped.sum() and w0.tobytes() == w1.tobytes()
        assert m.info()["cells_hit"] == 2 * int((w0["count"] > 0).sum())
        # an oblique axis and a general pose: o' within one fp32 ulp, residuals within 5e-6 m, cells equal off the edges
        q = wn.params(n_stations=20100, t_min=-8.0, point=(1.0, 2.0, 0.5), direction=(1.0, 0.05, 0.02))
        D = wn.design_frame(q)
        base = synth.pose_matrix((1.0 + 2.0, 2.0 + 0.1, 0.5 + 0.04), yaw_deg=5.0, roll_deg=3.0)
        far = base.copy()
        far[:, 3] += 20000 * 0.25 * D["a"]
        mq = c.wall_map(**q)
        cloud = _wall_seen_from(q, base, 300_000, seed=14)
        g0, e0, k0 = mq.add_points(cloud, base)
        g1, e1, k1 = mq.add_points(cloud, far)
        shift = g1["anchor_station"] - g0["anchor_station"]
        assert shift == 20000
        ulp = np.spacing(np.abs(g0["o"]))
        assert np.all(np.abs(g0["o"].astype(np.float64) - g1["o"].astype(np.float64)) <= ulp)
        for k in ("a", "u", "v"):
            assert np.array_equal(g0[k], g1[k])
        fin = np.isfinite(e0)
        assert np.array_equal(fin, np.isfinite(e1)) and np.abs(e0[fin].astype(np.float64) - e1[fin]).max() <= 5e-6
        amb = wn.points(cloud, None, g0, q)["ambiguous"] | wn.points(cloud, None, g1, q)["ambiguous"]
        assert (1.0 - amb.mean()) > 0.99
        both = ~amb & (k0 >= 0)
        assert both.mean() > 0.9
        assert np.array_equal(k0[~amb] >= 0, k1[~amb] >= 0)
        assert np.all(k1[both].astype(np.int64) - k0[both] == shift * 90)


def test_analytic_drive(gm):
    # 1.2 M points a frame: ~1000 a cell, so the bound's 2e-4 m is 0.6 sigma / sqrt(count) of headroom over its 4: the
    # chance that one of the ~17 000 undisturbed cells exceeds it by noise alone is ~5 % (at 400 k points a frame and
    # ~250 a cell it is ~50 %, and a 4.06 sigma cell did turn up in the twin as on the device)
    n = 1_200_000
    NST = 208          # 52 m of map for a 48 m tunnel
    drive = synth.tunnel_drive(12, n, seed=21, sigma=SIGMA)
    assert drive["length"] >= 40.0
    p = wn.params(n_stations=NST, **drive["design"])
    ref, info, valid = _blocking(gm, [f[0] for f in drive["frames"]], [f[1] for f in drive["frames"]], p,
                                 neighborRadius=synth.fixed_k_radius(n))
    raw = np.frombuffer(ref, wn.RAW_CELL).reshape(NST, 90)
    count, mean, mn, mx = (x.reshape(NST, 90) for x in wn.records_from(raw.reshape(-1)))
    near = np.zeros(count.shape, bool)
    for t0, t1, p0, p1, dr in drive["patches"]:
        js, ks = slice(int(t0 / 0.25), int(t1 / 0.25)), slice(int(p0 / 4), int(p1 / 4))
        c, m = count[js, ks].astype(np.float64), mean[js, ks].astype(np.float64)
        assert np.all(c > 0) and np.all(np.abs(m - dr) <= 4 * SIGMA / np.sqrt(c) + 2e-4), (dr, m)
        assert np.all(mn[js, ks] * np.sign(dr) > 0.15 - 6 * SIGMA) or dr < 0
        near[max(js.start - 1, 0):js.stop + 1, max(ks.start - 1, 0):ks.stop + 1] = True
    far = ~near & (count > 0)
    assert far.sum() > 10_000
    c, m = count[far].astype(np.float64), mean[far].astype(np.float64)
    worst = np.max(np.abs(m) - (4 * SIGMA / np.sqrt(c) + 2e-4))
    print(f"analytic: far cells={far.sum()} worst margin={worst:.3e}")
    assert np.all(np.abs(m) <= 4 * SIGMA / np.sqrt(c) + 2e-4)
    # a cell seen by several frames holds the sum of their per-frame counts
    with gm.GeometricMapping() as cx:
        total = np.zeros(NST * 90, np.int64)
        seen_by = np.zeros(NST * 90, np.int64)
        for (xyz, _), (_, pose) in zip(valid, drive["frames"]):
            one = cx.wall_map(**p)
            one.add_points(xyz, pose, outputs=False)
            cnt = one.read_raw()["count"].reshape(-1).astype(np.int64)
            one.close()
            total += cnt
            seen_by += cnt > 0
        assert np.array_equal(total, count.reshape(-1).astype(np.int64)) and (seen_by >= 2).sum() > 5000
    # chainages nobody saw are empty: the tunnel ends at 48 m = station 192
    empty = count == 0
    assert np.all(empty[192:]) and np.all(np.isnan(mean[empty])) and np.all(np.isnan(mn[empty]))
    assert not empty[int(6 / 0.25):int(44 / 0.25)].any()


def test_edges_and_failures(gm):
    drive = synth.tunnel_drive(1, 100_000, seed=2, start=6.0)
    cloud, pose = drive["frames"][0]
    cloud = cloud[np.all(np.abs(cloud) <= 5.0, axis=1)]
    L = _lib.load()
    with gm.GeometricMapping(n_slots=2) as c, gm.GeometricMapping() as other:
        # frames partly and wholly beyond either end: the twin's cells, nothing else
        for name, t_min, nst in (("low end", 6.0, 40), ("high end", -4.0, 40), ("below", 30.0, 40), ("above", -40.0, 40)):
            p = wn.params(n_stations=nst, t_min=t_min)
            m = c.wall_map(**p)
            info, res, cell = m.add_points(cloud, pose)
            r = wn.points(cloud, None, info, p)
            amb = r["ambiguous"]
            assert np.array_equal(cell[~amb].astype(np.int64), r["cell"][~amb]), name
            assert cell.max() < nst * 90 and cell.min() >= -1
            i = m.info()
            assert abs(i["outside"] - int((r["cls"] == wn.OUTSIDE).sum())) <= int(amb.sum()), name
            assert i["mapped"] + i["outside"] + i["beyond_gate"] == len(cloud)
            if name in ("below", "above"):
                assert i["mapped"] == 0 and i["cells_hit"] == 0 and i["outside"] > 0.9 * len(cloud)
                assert not m.read_raw().tobytes().strip(b"\0")
            else:
                assert 0 < i["mapped"] < len(cloud) and i["outside"] > 0
                assert m.read_raw().tobytes() == wn.cells_from(res, cell, nst * 90).tobytes()
            m.close()
        # windows, clear, buffers
        p = wn.params(n_stations=80)
        m = c.wall_map(**p)
        _, res, cell = m.add_points(cloud, pose)
        full = m.read_raw()
        assert np.array_equal(m.read_raw(0, 3), full[:3]) and np.array_equal(m.read_raw(77, 3), full[77:])
        assert m.read_raw(80, 0).shape == (0, 90) and m.read(10, 0)[0].shape == (0, 90)
        for s0, n in ((0, 81), (80, 1), (81, 0), (2**31, 2**31)):
            for fn in (m.read, m.read_raw, m.clear):
                with pytest.raises(gm.GmError) as e:
                    fn(s0, n)
                assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(gm.GmError) as e:
            m.add_raw(full, station0=1)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        import ctypes as C
        got = C.c_uint64(0)
        buf = (_lib.WallRawCell * 10)()
        assert L.gm_wall_map_read_raw(m._map, 0, 2, buf, 10, C.byref(got)) == _lib.GM_ERR_CAPACITY and got.value == 180
        assert L.gm_wall_map_read(m._map, 0, 2, None, 0, C.byref(got)) == _lib.GM_ERR_CAPACITY and got.value == 180
        before = m.info()
        m.clear(30, 5)
        after = m.read_raw()
        want = full.copy()
        want[30:35] = 0
        assert after.tobytes() == want.tobytes() and full[30:35]["count"].sum() > 0
        i = m.info()
        assert i["mapped"] == before["mapped"] and i["frames"] == 1 and i["cells_hit"] < before["cells_hit"]
        m.clear()
        i = m.info()
        assert not m.read_raw().tobytes().strip(b"\0")
        assert (i["frames"], i["mapped"], i["outside"], i["beyond_gate"], i["plane"], i["cells_hit"]) == (0,) * 6
        # bad poses
        good = synth.pose_matrix((1, 2, 3), yaw_deg=10)
        scaled, mirrored, nan = good.copy(), good.copy(), good.copy()
        scaled[:, :3] *= 1.001
        mirrored[:, 0] *= -1
        nan[2, 3] = np.nan
        for bad in (scaled, mirrored, nan):
            assert not wn.pose_ok(bad)
            with pytest.raises(gm.GmError) as e:
                m.add_points(cloud, bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        assert m.info()["frames"] == 0
        # a slot without a frame; the wrong context; a slot out of range
        with pytest.raises(gm.GmError) as e:
            m.add_frame(1, good)
        assert e.value.status == _lib.GM_ERR_NOT_READY
        ident = np.ascontiguousarray(IDENT)
        dp = ident.ctypes.data_as(C.POINTER(C.c_double))
        other.process_frame(cloud)
        assert L.gm_wall_map_add_frame(m._map, other._ctx, 0, dp, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_add_frame(m._map, c._ctx, 7, dp, None) == _lib.GM_ERR_INVALID_ARG
        c.process_frame(cloud)
        with pytest.raises(gm.GmError) as e:
            m.add_frame(0, nan)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        # out-of-limit parameters
        for kw in (dict(n_stations=0), dict(n_sectors=0), dict(n_sectors=4097), dict(n_stations=1 << 23, n_sectors=4),
                   dict(station_length=0.0), dict(t_min=float("nan")), dict(gate=9.0), dict(radius=0.0),
                   dict(direction=(0, 0, 0)), dict(up=(0, 0, 0))):
            with pytest.raises(gm.GmError) as e:
                c.wall_map(**kw)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG, kw
        # a frame whose n_valid is 0
        res = c.process_frame(np.full((100, 3), 50.0, np.float32))
        assert res["n_valid"] == 0
        m.add_frame(0, good)
        i = m.info()
        assert i["frames"] == 1 and i["mapped"] + i["outside"] + i["beyond_gate"] + i["plane"] == 0 and i["cells_hit"] == 0
        # empty stage call
        m.add_points(np.zeros((0, 3), np.float32), good)
        # maps alive when the context goes: freed with it, the handles are dead afterwards
        alive = c.wall_map(n_stations=10)
        alive.add_points(cloud, pose, outputs=False)
    with pytest.raises(ValueError):
        alive.info()
    alive.close()
