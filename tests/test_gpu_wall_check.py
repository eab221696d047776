"""GPU tests of the wall-map check (gm_wall_map_check_*, csrc/k_wall_check.hip + gm_wall_slot.hip): every size and tile edge
byte for byte against the integer twin (tests/wall_check_np.py) on the device's own per-point (e, cell) pairs, all / none
changed, analytic truth of a drive with world-fixed patches, the frame path against the stage path over every pipeline
path and the ordering rule, independence of the chainage, the results' lifetime and the failures."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_check_np as kn  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
KW = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
INFO_KEYS = ("status", "threshold_q", "n_points") + kn.NAMES + ("peak_pos", "peak_neg")


def _same_info(info, want):
    for k in INFO_KEYS:
        assert info[k] == want[k], (k, info[k], want[k])
    assert sum(info[k] for k in kn.NAMES) == info["n_points"]


def _map_state(m):
    i = m.info()
    return m.read_raw().tobytes(), tuple(i[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))


GRIDS = {
    "160x90": dict(n_stations=160, n_sectors=90, t_min=2.0),               # (the first frames reach below chainage 2: outside)
    "200x4096": dict(n_stations=200, n_sectors=4096, t_min=2.0),           # exceeds nothing here, makes sparse cells
}
SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 20_000)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_sizes_and_edges_byte_for_byte(gm, grid):
    survey = synth.tunnel_drive(4, 20_000, seed=3, patches=())
    drive = synth.tunnel_drive(4, 20_000, seed=3)          # the same poses; the wall moved inside the patches
    p = wn.params(**dict(drive["design"], **GRIDS[grid]))
    ck = dict(threshold=0.02, min_count=2, gate=0.12)             # (the 0.15 m patches lie beyond this gate)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        raw = m.read_raw()
        before = _map_state(m)
        scratch = c.wall_map(**dict(p, gate=ck["gate"]))
        lists, seen = 0, np.zeros(7, np.int64)
        for k, n in enumerate(SIZES):
            cloud, pose = drive["frames"][k % 4]
            xyz = cloud[:n]
            lab = (np.arange(n) % 7 == 0).astype(np.uint8)
            ainfo, e, cell = scratch.add_points(xyz, pose, labels=lab)
            for ref in (kn.MEAN, kn.ENVELOPE):
                info, rec, out = m.check_points(xyz, pose, labels=lab, reference=ref, **ck)
                # the add's chain, bit for bit, under the check's gate
                assert np.array_equal(out["e"].view(np.uint32), e.view(np.uint32)) and np.array_equal(out["cell"], cell)
                for f in ("o", "a", "u", "v", "R", "station_length", "sector_angle", "gate"):
                    assert np.array_equal(np.asarray(info["add"][f]).view(np.uint32), np.asarray(ainfo[f]).view(np.uint32)), f
                assert info["add"]["anchor_station"] == ainfo["anchor_station"]
                # the integer rule on those pairs and the checked map's raw cells
                want, wrec = kn.check(xyz, e, cell, raw, labels=lab, reference=ref, **ck)
                delta, cls = kn.classify(e, cell, raw, labels=lab, reference=ref, **ck)
                assert np.array_equal(out["cls"], cls) and np.array_equal(out["delta"].astype(np.int64), delta)
                _same_info(info, want)
                assert rec.tobytes() == wrec.tobytes()
                assert np.all(np.diff(rec["index"].astype(np.int64)) > 0)
                assert info["plane"] == int(lab.sum()) and info["changed_pos"] + info["changed_neg"] == len(rec)
                print(f"{grid} n={n} ref={ref}: " + " ".join(f"{k_}={info[k_]}" for k_ in kn.NAMES))
                lists += len(rec)
                seen += np.bincount(cls, minlength=7)
        assert lists > 0 and np.all(seen > 0)                                # every class occurred
        assert _map_state(m) == before


def test_all_changed_and_none_changed(gm):
    n = 10_000                                                 # three tiles
    survey = synth.tunnel_drive(4, 20_000, seed=8, radius=2.05, patches=())
    drive = synth.tunnel_drive(4, n, seed=9, patches=())
    p = wn.params(**dict(drive["design"], n_stations=160, radius=2.0))
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)                                    # the surveyed wall lies 0.05 m outside the design
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        cloud, pose = drive["frames"][1]                       # the wall seen now lies on it: 5 sigma inside the survey
        info, rec, out = m.check_points(cloud, pose, threshold=2.0 ** -20, min_count=1)
        assert info["threshold_q"] == 1 and info["n_points"] == n
        usable = n - info["plane"] - info["beyond_gate"] - info["outside"] - info["unsurveyed"]
        assert usable > 2 * 4096 and info["unchanged"] == 0 and len(rec) == usable
        assert np.array_equal(rec["index"], np.flatnonzero(out["cls"] >= kn.CHANGED_POS))
        assert info["changed_neg"] > 0.99 * usable and info["peak_neg"] == int(out["delta"].min()) < 0
        info, rec, out = m.check_points(cloud, pose, threshold=8.0, gate=8.0)
        assert info["threshold_q"] == 8 << 20 and len(rec) == 0 and info["peak_pos"] == 0 and info["peak_neg"] == 0
        assert info["changed_pos"] == 0 and info["changed_neg"] == 0 and info["unchanged"] > 0
        got = C.c_uint32(7)
        assert c._L.gm_wall_map_get_check(m._map, 0, None, None, 0, C.byref(got)) == _lib.GM_OK and got.value == 0


def test_analytic_truth(gm):
    """World-fixed +-0.15 m patches against a survey of the bare wall: no changed point outside a patch, every patch point
    changed with the patch's sign or in a cell the survey left unusable, at most 2 % of the mapped points unsurveyed (the
    fp64 twin of the rule gives 0, 0 of 1 903 and 1.41 % on these inputs, with no |delta| within 5 mm of T)."""
    survey = synth.tunnel_drive(8, 20_000, seed=21, patches=())
    drive = synth.tunnel_drive(8, 20_000, seed=21)
    p = wn.params(n_stations=192, **drive["design"])
    ck = dict(threshold=0.08, min_count=4, reference=kn.MEAN)
    tot = dict(points=0, patch=0, false_pos=0, missed=0, unsurveyed=0, mapped=0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        for (bare, _), (cloud, pose) in zip(survey["frames"], drive["frames"]):
            # the two drives share every random draw: a point differs iff a patch moved it, outward iff the patch's dr > 0
            patch = np.any(bare != cloud, axis=1)
            world = cloud.astype(np.float64) @ pose[:, :3].T + pose[:, 3]
            world0 = bare.astype(np.float64) @ pose[:, :3].T + pose[:, 3]
            sign = np.sign(np.hypot(world[:, 1], world[:, 2]) - np.hypot(world0[:, 1], world0[:, 2])).astype(np.int64)
            info, rec, out = m.check_points(cloud, pose, **ck)
            cls = out["cls"]
            changed = cls >= kn.CHANGED_POS
            assert info["plane"] == 0 and info["beyond_gate"] == 0 and info["outside"] == 0      # every point mapped
            tot["points"] += len(cloud)
            tot["patch"] += int(patch.sum())
            tot["false_pos"] += int((changed & ~patch).sum())
            want = np.where(sign > 0, kn.CHANGED_POS, kn.CHANGED_NEG)
            tot["missed"] += int((patch & (cls != want) & (cls != kn.UNSURVEYED)).sum())
            tot["unsurveyed"] += info["unsurveyed"]
            tot["mapped"] += int((out["cell"] >= 0).sum())
            assert np.array_equal(rec["index"], np.flatnonzero(changed))
    print("analytic truth:", tot, f"unsurveyed share {tot['unsurveyed'] / tot['mapped']:.4f}")
    assert tot["patch"] == 1903
    assert tot["false_pos"] == 0
    assert tot["missed"] == 0
    assert tot["unsurveyed"] <= 0.02 * tot["mapped"]


# ---- frame path = stage path ----

N_FRAME = 30_000
CK = dict(threshold=0.08, min_count=4)


def _drive():
    survey = synth.tunnel_drive(8, N_FRAME, seed=31, patches=())
    drive = synth.tunnel_drive(8, N_FRAME, seed=31)
    p = wn.params(n_stations=192, **drive["design"])
    return survey, [f[0] for f in drive["frames"]], [f[1] for f in drive["frames"]], p


def _outputs(c, res, slot=0):
    keep = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in res.items() if k not in ("stage_ms", "normals_kernel_ms")}
    return (repr(sorted(keep.items())), c._fetch(c._L.gm_get_cropped_xyz, slot, 4).tobytes(), c.normals(slot).tobytes(),
            c._fetch(c._L.gm_get_voxel_centroids, slot, 4).tobytes())


def _frames_without_checks(gm, clouds, poses, p, baseline, flags, kw):
    """Blocking frames with add_frame only.  Per frame: valid cloud, pad words, labels, the other outputs."""
    seen = []
    with gm.GeometricMapping(flags=flags, **kw) as c:
        m = c.wall_map(**p)
        m.add_raw(baseline)
        for cloud, pose in zip(clouds, poses):
            res = c.process_frame(cloud)
            m.add_frame(0, pose)
            xyz, rows = c.cropped_cloud()
            lab = c.labels() if flags & _lib.GM_CFG_RANSAC_PLANE else None
            seen.append((xyz, rows, lab, _outputs(c, res)))
        return seen, m.read_raw().tobytes()


def _stage_reference(gm, seen, poses, p, baseline):
    """check_points on each frame's valid cloud and labels against a map rebuilt to the state the frame's check saw."""
    want = []
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        m.add_raw(baseline)
        for (xyz, rows, lab, _), pose in zip(seen, poses):
            info, rec, _ = m.check_points(xyz, pose, labels=lab, outputs=False, **CK)
            rec["row"] = rows.view(np.uint32)[rec["index"]]          # the frame path reports the pad word, the stage call the index
            want.append((info, rec.tobytes()))
            m.add_points(xyz, pose, labels=lab, outputs=False)
    return want


def _baseline(gm, survey, p):
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        return m.read_raw()


def test_frame_path_equals_stage_path(gm):
    survey, clouds, poses, p = _drive()
    baseline = _baseline(gm, survey, p)
    kw = dict(neighborRadius=synth.fixed_k_radius(N_FRAME))
    seen, final = _frames_without_checks(gm, clouds, poses, p, baseline, _lib.GM_CFG_DEFAULT, kw)
    want = _stage_reference(gm, seen, poses, p, baseline)
    assert sum(len(w[1]) for w in want) > 0 and all(w[0]["unchanged"] > 0 for w in want)

    def blocking(flags, n, kw_, seen_, want_):
        with gm.GeometricMapping(flags=flags, **kw_) as c:
            m = c.wall_map(**p)
            m.add_raw(baseline)
            for k in range(n):
                res = c.process_frame(clouds[k])
                m.check_frame(0, poses[k], **CK)
                m.add_frame(0, poses[k])
                info, rec = m.check_result(0)
                _same_info(info, want_[k][0])
                assert rec.tobytes() == want_[k][1], k
                assert _outputs(c, res) == seen_[k][3], k                       # every other output: as without the checks
            return m.read_raw().tobytes()

    part = blocking(_lib.GM_CFG_DEFAULT, 4, kw, seen, want)
    assert blocking(_lib.GM_CFG_DEFAULT | _lib.GM_CFG_GRAPH, 4, kw, seen, want) == part
    # four streaming slots, check and add right behind each submit, slots reused, no sync until the end: a check sees the
    # adds of every earlier frame (on other slots' streams) and of no later one
    with gm.GeometricMapping(n_slots=4, **kw) as c:
        m = c.wall_map(**p)
        m.add_raw(baseline)
        got = []
        for k in range(8):
            if k >= 4:
                got.append(m.check_result(k % 4))                                # frame k - 4's, before the slot's next check replaces it
            c.submit_frame(k % 4, clouds[k])
            m.check_frame(k % 4, poses[k], **CK)
            m.add_frame(k % 4, poses[k])
        got += [m.check_result(k % 4) for k in range(4, 8)]
        for k, (info, rec) in enumerate(got):
            _same_info(info, want[k][0])
            assert rec.tobytes() == want[k][1], k
        m.sync()
        assert m.read_raw().tobytes() == final
    # the plane RANSAC's labels: plane points are counted and never listed
    pkw = dict(kw, **KW)
    pseen, _ = _frames_without_checks(gm, clouds[:4], poses[:4], p, baseline, PLANE, pkw)
    pwant = _stage_reference(gm, pseen, poses[:4], p, baseline)
    for (xyz, rows, lab, _), (info, recb) in zip(pseen, pwant):
        rec = np.frombuffer(recb, kn.POINT)
        assert info["plane"] == int((lab == 1).sum()) > 0 and not np.any(lab[rec["index"]] == 1)
    blocking(PLANE, 4, pkw, pseen, pwant)


def _wall_seen_from(p, pose, n, seed, dr=0.0):
    rng = np.random.default_rng(seed)
    D = wn.design_frame(p)
    s = (pose[:, 3] - D["o"]) @ D["a"]
    t, phi = rng.uniform(s - 6.0, s + 6.0, n), rng.uniform(0.0, 2 * np.pi, n)
    rr = D["R"] + dr * (phi < 1.0) + rng.normal(0.0, 0.01, n)
    world = D["o"] + t[:, None] * D["a"] + (rr * np.cos(phi))[:, None] * D["u"] + (rr * np.sin(phi))[:, None] * D["v"]
    cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(np.float32)
    return np.ascontiguousarray(cloud[np.all(np.abs(cloud) <= 5.0, axis=1)])


def test_chainage(gm):
    p, p0, p1 = wn.chainage_pair(20000)
    survey = _wall_seen_from(p, p0, 60_000, seed=41)
    cloud = _wall_seen_from(p, p0, 20_000, seed=42, dr=0.1)     # a sixth of the ring moved out by 0.1 m
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        _, _, cell = m.add_points(survey, p0)
        j0 = int(cell[cell >= 0].min()) // 90
        n = int(cell.max()) // 90 - j0 + 1
        m.add_raw(m.read_raw(j0, n), station0=j0 + 20000)       # the same cells, 20 000 stations on
        i0, r0, o0 = m.check_points(cloud, p0, min_count=4)
        i1, r1, o1 = m.check_points(cloud, p1, min_count=4)
        assert i1["add"]["anchor_station"] - i0["add"]["anchor_station"] == 20000
        _same_info(i1, i0)
        assert len(r0) > 1000 and i0["changed_pos"] > 1000 and i0["unchanged"] > 1000
        assert np.array_equal(r1["cell"].astype(np.int64) - r0["cell"], np.full(len(r0), 20000 * 90))
        r1["cell"] = r0["cell"]
        assert r0.tobytes() == r1.tobytes()
        assert np.array_equal(o0["cls"], o1["cls"]) and np.array_equal(o0["delta"], o1["delta"])


def test_lifetime_and_failures(gm):
    drive = synth.tunnel_drive(2, 5_000, seed=2)
    (cloud, pose), (cloud1, pose1) = drive["frames"]
    p = wn.params(n_stations=80, **drive["design"])
    L = _lib.load()
    info, got = _lib.WallCheckInfo(), C.c_uint32(7)
    buf = np.zeros(5_000, kn.POINT)
    bp = buf.ctypes.data_as(C.POINTER(_lib.WallCheckPoint))
    dp = np.ascontiguousarray(pose).ctypes.data_as(C.POINTER(C.c_double))
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(5_000)) as c, gm.GeometricMapping() as other:
        m = c.wall_map(**p)
        m.add_points(cloud, pose, outputs=False)
        # before any check
        assert L.gm_wall_map_get_check(m._map, 0, C.byref(info), None, 0, C.byref(got)) == _lib.GM_ERR_NOT_READY and got.value == 0
        # a slot without a frame; the wrong context; a bad slot; a bad pose; a bad parameter
        assert L.gm_wall_map_check_frame(m._map, c._ctx, 1, dp, None, None) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_check_frame(m._map, other._ctx, 0, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_check_frame(m._map, c._ctx, 7, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_check(m._map, 7, C.byref(info), None, 0, C.byref(got)) == _lib.GM_ERR_INVALID_ARG
        c.process_frame(cloud1)
        nan = pose1.copy()
        nan[1, 3] = np.nan
        for bad in (nan, pose1 * 1.01):
            with pytest.raises(gm.GmError) as e:
                m.check_frame(0, bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(gm.GmError) as e:
            m.check_frame(0, pose1, threshold=9.0)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_check(m._map, 0, C.byref(info), None, 0, C.byref(got)) == _lib.GM_ERR_NOT_READY
        # a check; a count query; a short buffer writes no row
        m.check_frame(0, pose1, threshold=0.03, min_count=1)
        assert L.gm_wall_map_get_check(m._map, 0, C.byref(info), None, 0, C.byref(got)) == _lib.GM_OK
        n1 = got.value
        assert n1 > 1 and info.changed_pos + info.changed_neg == n1 and info.struct_size == C.sizeof(_lib.WallCheckInfo)
        got.value = 0
        assert L.gm_wall_map_get_check(m._map, 0, C.byref(info), bp, n1 - 1, C.byref(got)) == _lib.GM_ERR_CAPACITY
        assert got.value == n1 and buf.tobytes() == bytes(buf.nbytes)
        assert L.gm_wall_map_get_check(m._map, 0, C.byref(info), None, 3, C.byref(got)) == _lib.GM_ERR_INVALID_ARG
        i1, r1 = m.check_result(0)
        assert len(r1) == n1 and (i1, r1.tobytes()) == (lambda a: (a[0], a[1].tobytes()))(m.check_result(0))   # readable again
        # a second check on the slot replaces the first; the other slot has none
        m.check_frame(0, pose1, threshold=0.5, min_count=1)
        i2, r2 = m.check_result(0)
        assert i2["threshold_q"] == 1 << 19 and len(r2) < n1
        assert L.gm_wall_map_get_check(m._map, 1, C.byref(info), None, 0, C.byref(got)) == _lib.GM_ERR_NOT_READY
        # a slot reused by a stage call holds no frame
        m.add_points(cloud, pose, outputs=False)
        with pytest.raises(gm.GmError) as e:
            m.check_frame(0, pose1)
        assert e.value.status == _lib.GM_ERR_NOT_READY
        # a frame whose n_valid is 0
        res = c.process_frame(np.full((100, 3), 50.0, np.float32))
        assert res["n_valid"] == 0
        m.check_frame(0, pose1)
        i0, r0 = m.check_result(0)
        assert i0["n_points"] == 0 and len(r0) == 0 and sum(i0[k] for k in kn.NAMES) == 0
        # a map destroyed with a check outstanding frees cleanly; so does the context with one
        c.submit_frame(1, cloud1)
        m.check_frame(1, pose1)
        m.close()
        c.wait_frame(1)
        m2 = c.wall_map(**p)
        c.submit_frame(0, cloud1)
        m2.check_frame(0, pose1)
