"""GPU tests of the wall map on a clothoid design axis (gm_wall_map_create_clothoid): add, checked add, check, cloud and
mesh against the twin tests/wall_clothoid_np.py, and the integer rule of tests/wall_np.py byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_wall_map as twm  # noqa: E402  (GRIDS and the rebuild rule)
import wall_add_checked_np as an  # noqa: E402
import wall_check_np as kn  # noqa: E402
import wall_clothoid_np as wl  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
OBLIQUE = (0.0, 0.6, 0.8)
CURVES = {
    "horizontal_from_straight": dict(curvature=0.0, rate=1 / (80.0 * 48.0), toward=(0.0, 1.0, 0.0)),
    "vertical_flattening": dict(curvature=1 / 100.0, rate=-1 / 6000.0, toward=(0.0, 0.0, -1.0)),
    "oblique_s": dict(curvature=-1 / 150.0, rate=1 / (150.0 * 24.0), toward=OBLIQUE, yaw_deg=8.0, roll_deg=6.0, lateral=0.4),
}
# twice the worst |e32 - e64| of the CPU sweep (tests/test_wall_clothoid_np.py: 2.6e-6 m), rounded up to one digit
TOL = 6e-6


def _frame(m, pose):
    """The frame the library reports for this map and pose (gm_wall_clothoid_add_frame), as the twin's points() takes it."""
    return api.wall_clothoid_add_frame(m.prm, m.clothoid_struct(), pose)


def _against_twin(m, info, res, cell, xyz, labels, pose, p, cl):
    f = _frame(m, pose)
    w = wl.add_frame(wl.design(p, cl), p, pose)
    assert info["anchor_station"] == f["anchor_station"] == w["anchor"]
    for k in ("o", "a"):
        assert np.array_equal(info[k].view(np.uint32), f[k].view(np.uint32)), k
    for k in ("o", "a", "u", "v"):
        assert np.abs(info[k].astype(np.float64) - w[k]).max() <= 1e-6, k
    assert float(info["R"]) == w["R"] and float(info["station_length"]) == w["ds"] and float(info["gate"]) == w["gate"]
    assert float(f["rate"]) == w["rate"] and abs(float(f["kappa"]) - w["kappa"]) <= 1e-9
    r = wl.points(xyz, labels, f, p)
    fin = np.isfinite(r["e"])
    assert np.array_equal(fin, np.isfinite(res))
    err = np.abs(res[fin].astype(np.float64) - r["e"][fin]).max()
    amb = r["ambiguous"]
    share = 1.0 - amb.mean()
    print(f"clothoid twin: n={len(xyz)} max|e-e_twin|={err:.3e} non-ambiguous={share:.5f}")
    assert err <= TOL
    assert share > 0.99
    assert np.array_equal(cell[~amb].astype(np.int64), r["cell"][~amb])
    return r


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_twin(gm, curve):
    drive = synth.clothoid_drive(3, 4000, seed=11, **CURVES[curve])
    p = wn.params(n_stations=200, **drive["design"])
    with gm.GeometricMapping() as c:
        for cloud, pose in drive["frames"]:
            m = c.wall_map(clothoid=drive["clothoid"], **p)
            got = m.clothoid
            assert m.arc is None and np.allclose(got["normal"], drive["clothoid"]["normal"])
            assert (got["curvature"], got["rate"], got["point_chainage"]) == (CURVES[curve]["curvature"], CURVES[curve]["rate"], 0.0)
            lab = (np.arange(len(cloud)) % 11 == 0).astype(np.uint8)
            info, res, cell = m.add_points(cloud, pose, labels=lab)
            r = _against_twin(m, info, res, cell, cloud, lab, pose, p, drive["clothoid"])
            twm._check_class_counts(m.info(), r)
            assert m.info()["mapped"] > 0.85 * len(cloud)
            m.close()


SIZES = (0, 1, 63, 64, 65, 2049, 20_000)
# the default grid's 1000 m of map stay within |psi| <= 3: kappa falls from 1 / 400 to 0 at 500 m
LONG = dict(curvature=1 / 400.0, rate=-5.0e-6, toward=OBLIQUE)


@pytest.mark.parametrize("grid", sorted(twm.GRIDS))
def test_exact_rebuild(gm, grid):
    drive = synth.clothoid_drive(len(SIZES), 20_000, seed=5, **LONG)
    p = wn.params(**dict(drive["design"], **twm.GRIDS[grid]))
    with gm.GeometricMapping() as c:
        m = c.wall_map(clothoid=drive["clothoid"], **p)
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
    drive = synth.clothoid_drive(4, n, seed=9, **CURVES["oblique_s"] | dict(yaw_deg=4.0, roll_deg=3.0, lateral=0.1))
    p = wn.params(n_stations=200, **drive["design"])
    kw = dict(neighborRadius=synth.fixed_k_radius(n))
    with gm.GeometricMapping(n_slots=2, **kw) as c:
        m = c.wall_map(clothoid=drive["clothoid"], **p)
        valid = []
        for k, (cloud, pose) in enumerate(drive["frames"]):
            c.submit_frame(k % 2, cloud)
            m.add_frame(k % 2, pose)
            c.wait_frame(k % 2)
            valid.append(c.cropped_cloud(k % 2)[0])
        m.sync()
        ref, info = m.read_raw().tobytes(), m.info()
        assert info["frames"] == 4 and info["mapped"] > 0.5 * sum(len(v) for v in valid)
        s = c.wall_map(clothoid=drive["clothoid"], **p)
        for xyz, (_, pose) in zip(valid, drive["frames"]):
            s.add_points(xyz, pose, outputs=False)
        assert s.read_raw().tobytes() == ref
        si = s.info()
        for k in ("mapped", "outside", "beyond_gate", "plane", "cells_hit", "frames"):
            assert si[k] == info[k], k
        # a saved map comes back on its clothoid
        path = str(tmp_path / "clothoid.npz")
        s.save(path)
        b = gm.WallMap.load(c, path)
        assert b.read_raw().tobytes() == ref and bytes(b.clothoid_struct()) == bytes(m.clothoid_struct()) and b.arc is None
        b.regions(baseline=m)


def test_analytic_tube(gm):
    """sigma = 0: every point lies exactly on a tube around a clothoid with two patches.  1e-5 m: the chain's 5e-6 m plus
    the rounding of the fp32 inputs.  The clothoid starts at a 100 km radius and its rate takes it 0.125 m, half the gate,
    off its osculating circle over the map's 48 m (rate t^3 / 6): a straight map and the arc map that osculates at
    chainage 0 see that departure in the sectors that face +-n, where the clothoid map sees nothing."""
    NST, T_MAX = 200, 48.0
    k0 = 1.0e-5
    rate = 0.125 * 6.0 / T_MAX ** 3
    patches = synth.DRIVE_PATCHES[:2]
    drive = synth.clothoid_drive(12, 20_000, seed=21, curvature=k0, rate=rate, toward=(0.0, 1.0, 0.0), sigma=0.0, patches=patches)
    p = wn.params(n_stations=NST, **drive["design"])
    with gm.GeometricMapping() as c:
        m, straight = c.wall_map(clothoid=drive["clothoid"], **p), c.wall_map(**p)
        osculating = c.wall_map(arc=dict(curvature=(0.0, k0, 0.0), point_chainage=0.0), **p)
        n = 0
        for cloud, pose in drive["frames"]:
            for w in (m, straight, osculating):
                w.add_points(cloud, pose, outputs=False)
            n += len(cloud)
        count, mean, _, _ = (x.reshape(NST, 90) for x in m.read())
        others = [[x.reshape(NST, 90) for x in w.read()][:2] for w in (straight, osculating)]
        i = m.info()
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
    # the assertion that shows the feature: n = +y is phi = 270 degrees (u = +z, v = -y), -n is phi = 90 degrees
    departure = rate * T_MAX ** 3 / 6.0
    for name, (ocount, omean) in zip(("straight", "osculating arc"), others):
        facing = np.zeros(count.shape, bool)
        facing[:, [22, 67]] = True
        facing &= (ocount > 0) & ~inside
        seen = np.abs(omean[facing].astype(np.float64)).max()
        print(f"{name} map on the same frames: largest |cell mean| facing +-n {seen:.4f} m of a departure of {departure:.4f} m")
        assert seen >= 0.5 * departure


def test_chainage_invariance(gm):
    """The same drive on a map whose point_chainage and t_min are both moved by 5 km: the same anchors relative to t_min, e
    within the tolerance, equal cells off the ambiguous mask."""
    drive = synth.clothoid_drive(3, 6000, seed=13, **CURVES["oblique_s"])
    p0 = wn.params(n_stations=200, **drive["design"])
    p1 = dict(p0, t_min=5000.0)
    cl1 = dict(drive["clothoid"], point_chainage=5000.0)
    with gm.GeometricMapping() as c:
        m0, m1 = c.wall_map(clothoid=drive["clothoid"], **p0), c.wall_map(clothoid=cl1, **p1)
        for cloud, pose in drive["frames"]:
            i0, e0, c0 = m0.add_points(cloud, pose)
            i1, e1, c1 = m1.add_points(cloud, pose)
            assert i1["anchor_station"] == i0["anchor_station"]
            f0, f1 = _frame(m0, pose), _frame(m1, pose)
            assert abs((f1["sensor_chainage"] - 5000.0) - f0["sensor_chainage"]) <= 1e-9
            fin = np.isfinite(e0)
            assert np.array_equal(fin, np.isfinite(e1)) and np.abs(e0[fin].astype(np.float64) - e1[fin]).max() <= TOL
            amb = wl.points(cloud, None, f0, p0)["ambiguous"] | wl.points(cloud, None, f1, p1)["ambiguous"]
            assert (1.0 - amb.mean()) > 0.99
            assert (c0[~amb] >= 0).mean() > 0.85 and np.array_equal(c0[~amb], c1[~amb])


def test_check_and_checked_add(gm):
    n = 5000
    kw = dict(CURVES["oblique_s"], yaw_deg=4.0, roll_deg=3.0, lateral=0.25)
    survey = synth.clothoid_drive(4, 20_000, seed=3, patches=(), **kw)
    drive = synth.clothoid_drive(4, n, seed=3, **kw)            # the same poses; the wall moved inside the patches
    p = wn.params(n_stations=200, **drive["design"])
    ck = dict(threshold=0.004, min_count=2)
    seen = dict(pos=0, neg=0, skipped=0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(clothoid=drive["clothoid"], **p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        raw = m.read_raw()
        before = raw.tobytes()
        for k, (cloud, pose) in enumerate(drive["frames"]):
            lab = (np.arange(n) % 7 == 0).astype(np.uint8) if k % 2 else None
            info, rows, out = m.check_points(cloud, pose, labels=lab, **ck)
            e, cell, delta, cls = (out[k_] for k_ in ("e", "cell", "delta", "cls"))
            # the chain: the check's (e, cell) against the fp64 twin under the check's own gate
            r = wl.points(cloud, lab, _frame(m, pose), p, gate=kn.DEFAULTS["gate"])
            fin = np.isfinite(r["e"])
            assert np.array_equal(fin, np.isfinite(e)) and np.abs(e[fin].astype(np.float64) - r["e"][fin]).max() <= TOL
            assert np.array_equal(cell[~r["ambiguous"]].astype(np.int64), r["cell"][~r["ambiguous"]])
            # the rule: the existing check twin fed the clothoid chain's (e, cell)
            winfo, wrows = kn.check(cloud, e, cell, raw, labels=lab, status=info["status"], **ck)
            wdelta, wcls = kn.classify(e, cell, raw, lab, **ck)
            assert np.array_equal(cls, wcls) and np.array_equal(delta.astype(np.int64), np.clip(wdelta, -2 ** 31, 2 ** 31 - 1))
            assert rows.tobytes() == wrows.tobytes()
            for key in winfo:
                assert info[key] == winfo[key], key
            seen["pos"] += info["changed_pos"]
            seen["neg"] += info["changed_neg"]
            # the checked add: the bytes of a plain add of the cloud with the skipped rows deleted
            a, b = c.wall_map(clothoid=drive["clothoid"], **p), c.wall_map(clothoid=drive["clothoid"], **p)
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


EDGE_SIZES = (0, 1, 63, 64, 65, 1025, 2049)   # a mask word's edge; one 1024-thread block: its stride plus 1, two strides plus 1


def test_checked_add_and_check_at_trip_and_window_edges(gm, monkeypatch):
    """The masked clothoid add at the edges of its point stream -- no point, a last wave with lanes past n (63, 64 and 65
    points: a mask word's edge), a trip whose second slot lies wholly past n -- on two-centimetre stations, where the LDS
    window holds the 11 stations around the anchor and the rest of the 5 m box goes to the map directly.  Every third
    point is a selected row; the map, the per-point outputs and the counts are those of the plain add of the points that
    stay (the twin's selection).  The check of each size classes as many points as it was given."""
    monkeypatch.setenv("GM_WALL_POINTS_PER_BLOCK", "4096")   # read when a map is created: one block for every size here
    n_max = max(EDGE_SIZES)
    drive = synth.clothoid_drive(len(EDGE_SIZES), n_max, seed=5, **LONG)
    kw = dict(clothoid=drive["clothoid"])
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
            cinfo, crows, cout = a.check_points(xyz, pose, labels=lab)
            assert cinfo["n_points"] == n and len(cout["cls"]) == n
            if n:                                            # the check's chain is the add's: the same residual bits
                _, fe, fc = b.add_points(xyz, pose, labels=lab)
                assert np.array_equal(cout["e"].view(np.uint32), fe.view(np.uint32))
                gate_in = ~(np.abs(fe) > np.float32(kn.DEFAULTS["gate"]))   # (the check's own gate may be narrower than the map's)
                assert np.array_equal(cout["cell"][gate_in & (fc >= 0)], fc[gate_in & (fc >= 0)])
            a.close()
            b.close()
    print(f"clothoid: {sides[0]} mapped points inside the LDS window, {sides[1]} outside it")
    assert sides[0] > 10 and sides[1] > 1000


@pytest.mark.parametrize("blocks", [(1, 1), (3, 4)])
def test_cloud_and_mesh(gm, blocks):
    bs, bk = blocks
    drive = synth.clothoid_drive(3, 20_000, seed=7, start=6.0, step=3.0, **CURVES["oblique_s"] | dict(yaw_deg=4.0, roll_deg=3.0, lateral=0.25))
    p = wn.params(n_stations=80, **drive["design"])
    D = wl.design(p, drive["clothoid"])
    station0, n = 10, 41                                   # 10.25 m of map; a ragged last block row
    mid = p["t_min"] + (station0 + n / 2) * p["station_length"]
    anchor = tuple(np.round(wl.frame(D, mid)[0], 3))       # |coordinates| < 8 m: half an fp32 ulp is 2.4e-7 m
    prm = dict(block_stations=bs, block_sectors=bk, anchor=anchor, min_count=2)
    os.environ["GM_WALL_CLOUD_CHUNK"] = str(4 * (90 // bk + 1))   # a few block rows per chunk: the row table of a later chunk
    try:
        with gm.GeometricMapping() as c:
            m = c.wall_map(clothoid=drive["clothoid"], **p)
            for cloud, pose in drive["frames"]:
                m.add_points(cloud, pose, outputs=False)
            raw = m.read_raw()
            tab = api.wall_cloud_directions(m.prm, **prm)
            info, rec = m.cloud(station0, n, **prm)
            winfo, wrec = wl.cloud(raw, p, drive["clothoid"], station0, n, directions=tab, **prm)
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
            s, phi, e = api.wall_clothoid_project(m.prm, m.clothoid_struct(), xyz)
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


def test_refusals(gm):
    drive = synth.clothoid_drive(2, 4000, seed=2, **CURVES["horizontal_from_straight"])
    p = wn.params(n_stations=200, **drive["design"])
    cl = drive["clothoid"]
    U, I = _lib.GM_ERR_UNSUPPORTED, _lib.GM_ERR_INVALID_ARG
    with gm.GeometricMapping() as c:
        m = c.wall_map(clothoid=cl, **p)
        straight = c.wall_map(**p)
        arc = c.wall_map(arc=dict(curvature=(0.0, 1 / 80.0, 0.0), point_chainage=0.0), **p)
        assert straight.clothoid is None and arc.clothoid is None and m.clothoid is not None and m.arc is None
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
        # a baseline must be a map on the same clothoid
        other = c.wall_map(clothoid=dict(cl, rate=cl["rate"] * 1.01), **p)
        same = c.wall_map(clothoid=cl, **p)
        for base in (other, arc, straight):
            with pytest.raises(_lib.GmError) as ex:
                m.regions(baseline=base)
            assert ex.value.status == I
        for w in (straight, arc):
            with pytest.raises(_lib.GmError) as ex:
                w.regions(baseline=m)
            assert ex.value.status == I
        m.regions(baseline=same)
        # gm_wall_map_create_clothoid's limits (200 stations: 50 m of map)
        nan, inf = float("nan"), float("inf")
        ok = dict(normal=(0.0, 1.0, 0.0), curvature=0.0, rate=1e-4, point_chainage=0.0)
        for bad in (dict(ok, rate=1.9e-8),                  # |rate| L < 1e-6
                    dict(ok, rate=0.0),
                    dict(ok, rate=0.0045),                  # (R + gate) max |kappa| > 0.5 at the far end
                    dict(ok, curvature=-0.23),              # ... at the start
                    dict(ok, rate=0.0025),                  # |psi| > 3 at the far end
                    dict(ok, curvature=0.2, rate=-0.005),   # |psi| = 4 where kappa = 0, inside the map; 3.75 at its end
                    dict(ok, curvature=0.19, rate=-0.0059),  # ... 3.06 there only: 2.1 at the end
                    dict(ok, normal=(0.0, nan, 0.0)), dict(ok, curvature=inf), dict(ok, rate=nan), dict(ok, point_chainage=inf),
                    dict(ok, normal=(0.3, 0.0, 0.0)),       # along the axis: no side is left
                    dict(ok, normal=(0.0, 0.0, 0.0))):
            with pytest.raises(_lib.GmError) as ex:
                c.wall_map(clothoid=bad, **p)
            assert ex.value.status == I, bad
        for field, value in (("struct_size", 48), ("reserved", 1)):
            s = api.wall_clothoid(**ok)
            setattr(s, field, value)
            with pytest.raises(_lib.GmError) as ex:
                c.wall_map(clothoid=s, **p)
            assert ex.value.status == I
        with pytest.raises(ValueError):
            c.wall_map(clothoid=ok, arc=dict(curvature=(0.0, 0.01, 0.0), point_chainage=0.0), **p)
        h = C.c_void_p()
        assert c._L.gm_wall_map_create_clothoid(c._ctx, C.byref(m.prm), None, C.byref(h)) == I and not h.value
        # a pose whose anchor is out of range; a pose past the map's end is accepted and maps nothing
        far = pose.copy()
        far[0, 3] = 1.0e300
        with pytest.raises(_lib.GmError) as ex:
            m.add_points(cloud, far)
        assert ex.value.status == I
        o, a, u, v, _, _ = api.wall_clothoid_frame(m.prm, m.clothoid_struct(), 75.0)
        past = np.concatenate([np.stack([a, -v, u], axis=1), o.reshape(3, 1)], axis=1)
        fresh = c.wall_map(clothoid=cl, **p)
        info, _, cell = fresh.add_points(cloud, past)
        assert info["anchor_station"] >= 299 and np.all(cell == -1) and fresh.info()["mapped"] == 0
        assert m.read_raw().tobytes() == before
