"""GPU tests of the wall-map locate (gm_wall_map_locate_*, csrc/k_wall_locate.hip + gm_wall_slot.hip): every size at which the
fixed grid takes another path against the fp64 twin (tests/wall_locate_np.py) fed the frames the device reported, the
truth of a drive located from perturbed poses, the failures, and the frame path against the stage path over every
pipeline path and the ordering rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_locate_np as ln  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
KW = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
# (131071 .. 131073: the second slot of the 4-point unroll; 524288, 524289: the second trip of the fixed grid)
SIZES = (0, 1, 3, 4, 63, 64, 65, 1025, 4097, 131071, 131072, 131073, 524288, 524289)
SWEEP_SEED = 4            # (tests/wall_locate_np.py's chain on these inputs: ambiguous == 0 on every DESIGN pass)
LATERAL_BOUND, ANGLE_BOUND = 1e-3, 3e-4
TRUTH_SEED = 9


def perturbed(pose, rng, lateral=0.05, angle_deg=0.5):
    """tr moved by up to +-lateral in y and z, Rm right-multiplied by a yaw and a pitch of up to +-angle_deg."""
    dy, dz = rng.uniform(-lateral, lateral, 2)
    yaw, pitch = rng.uniform(-angle_deg, angle_deg, 2)
    out = np.array(pose, np.float64)
    out[:, :3] = out[:, :3] @ synth.pose_matrix((0, 0, 0), yaw_deg=yaw, pitch_deg=pitch)[:, :3]
    out[1, 3] += dy
    out[2, 3] += dz
    return out


def pose_errors(p, got, true):
    """(lateral offset: |tr' - tr_true| perpendicular to a, angle between Rm'^T a and Rm_true^T a)."""
    a = wn.design_frame(p)["a"]
    dt = got[:, 3] - true[:, 3]
    d1, d2 = got[:, :3].T @ a, true[:, :3].T @ a
    return float(np.linalg.norm(dt - (dt @ a) * a)), float(np.arctan2(np.linalg.norm(np.cross(d1, d2)), d1 @ d2))


def sweep_inputs(seed=SWEEP_SEED):
    """The size sweep's survey, parameters and (xyz, labels, pose) per size: points of tunnel_drive frames truncated or
    tiled to n, every seventh a plane point, located from a perturbed pose."""
    survey = synth.tunnel_drive(4, 20_000, seed=seed, patches=())
    drive = synth.tunnel_drive(4, 20_000, seed=seed)          # the same poses; the wall moved inside the patches
    p = wn.params(**dict(drive["design"], n_stations=160, n_sectors=90, t_min=2.0))   # (the first frames reach below chainage 2)
    rng = np.random.default_rng(seed + 100)
    cases = []
    for k, n in enumerate(SIZES):
        cloud, pose = drive["frames"][k % 4]
        xyz = np.ascontiguousarray(np.tile(cloud, ((n + len(cloud) - 1) // len(cloud) or 1, 1))[:n])
        cases.append((n, xyz, (np.arange(n) % 7 == 0).astype(np.uint8), perturbed(pose, rng)))
    return survey, p, cases


def _map_state(m):
    i = m.info()
    return m.read_raw().tobytes(), tuple(i[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))


def _frame_of(rec):
    return {k: rec[k].astype(np.float64) for k in ("o", "a", "u", "v")}


def _pose_is_nan(info):
    return bool(np.all(np.isnan(info["pose"])) and np.all(np.isnan(info["lateral"])) and np.all(np.isnan(info["tilt"])))


@pytest.mark.parametrize("ref", (ln.DESIGN, ln.MAP))
def test_sizes_and_edges_against_the_twin(gm, ref):
    survey, p, cases = sweep_inputs()
    min_count = 8
    seen = dict.fromkeys(ln.CLASSES, 0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        raw = m.read_raw()
        before = _map_state(m)
        for n, xyz, lab, pose in cases:
            info, res, cell = m.locate_points(xyz, pose, labels=lab, reference=ref, min_count=min_count)
            assert info["n_points"] == n and info["anchor_station"] == ln.start(wn.design_frame(p), p, pose)[2]
            failed = bool(info["status"] & ln.FAILED_MASK)
            ran = info["passes"] + (1 if failed else 0)
            assert ran <= 3 and (failed or info["passes"] == 3)
            amb_total = 0
            for k in range(ran):
                rec = info["pass"][k]
                last = k == ran - 1
                assert rec["gate"] == np.float32(0.25 * 2.0 ** -k)
                assert sum(rec[q] for q in ln.CLASSES) == n and rec["plane"] == int(lab.sum())
                t = ln.one_pass(xyz, lab, _frame_of(rec), rec["gate"], raw if ref == ln.MAP else None, min_count,
                                cells=cell if (ref == ln.MAP and last) else None, p=p, anchor=info["anchor_station"])
                amb = t["ambiguous"]
                amb_total += amb
                print(f"ref={ref} n={n} pass={k}: " + " ".join(f"{q}={rec[q]}" for q in ln.CLASSES) + f" ambiguous={amb}",
                      "step", rec["step"], "twin", t["step"])
                if amb == 0:
                    assert {q: rec[q] for q in ln.CLASSES} == t["classes"]
                else:
                    assert abs(rec["used"] - t["classes"]["used"]) <= amb
                for q in ln.CLASSES:
                    seen[q] += rec[q]
                if amb == 0:
                    assert (t["status"] != ln.OK) == (failed and last) and (not failed or not last or info["status"] == t["status"])
                if n >= 64:
                    assert not failed and np.abs(rec["step"] - t["step"]).max() <= 1e-6
                    assert abs(rec["rms"] - t["rms"]) <= 1e-6
                if last and n:
                    if ref == ln.DESIGN:
                        assert np.all(cell == -1)
                    if amb == 0:
                        assert np.array_equal(np.isnan(res), np.isnan(t["res"]))
                    both = ~np.isnan(res) & ~np.isnan(t["res"])
                    assert np.abs(res[both].astype(np.float64) - t["res"][both]).max(initial=0.0) <= 2e-6
                    assert int((~np.isnan(res)).sum()) == rec["used"]
            if amb_total:
                print(f"ref={ref} n={n}: {amb_total} ambiguous points over the passes")   # (DESIGN: the seed was chosen for 0)
            if n < 4:
                assert info["status"] == _lib.GM_LOCATE_DEGENERATE and info["passes"] == 0 and _pose_is_nan(info)
            if not failed:
                assert wn.pose_ok(info["pose"])
                assert np.allclose(info["lateral"], sum(info["pass"][k]["step"][:2] for k in range(3)), rtol=0, atol=1e-15)
                assert np.allclose(info["tilt"], sum(info["pass"][k]["step"][2:] for k in range(3)), rtol=0, atol=1e-15)
        assert _map_state(m) == before                      # the map is not changed
    print("classes over the sweep:", seen)
    want = ln.CLASSES if ref == ln.MAP else ("plane", "gated", "used")
    assert all(seen[q] > 0 for q in want) and all(seen[q] == 0 for q in ln.CLASSES if q not in want)


# ---- truth ----

def _truth_inputs(patches=synth.DRIVE_PATCHES):
    survey = synth.tunnel_drive(8, 20_000, seed=21, patches=patches)
    drive = synth.tunnel_drive(8, 20_000, seed=22, patches=patches)
    p = wn.params(n_stations=192, **drive["design"])
    rng = np.random.default_rng(TRUTH_SEED)
    return survey, drive, p, [perturbed(pose, rng) for _, pose in drive["frames"]]


def test_truth_of_a_perturbed_drive(gm):
    """Frames of tunnel_drive(8, 20 000, seed=22) located from their true poses moved by up to 0.05 m in y and z and turned
    by up to 0.5 degrees in yaw and pitch, against the survey tunnel_drive(8, 20 000, seed=21) added at the true poses (MAP)
    and against the design (DESIGN).  The recovered lateral offset stays below 1e-3 m and the axis angle below 3e-4 rad.
    The fp64 twin on these inputs, from errors of up to 0.067 m and 10.1 mrad: at most 2.15e-4 m and 6.30e-5 rad in MAP
    mode, 1.81e-4 m and 6.23e-5 rad in DESIGN mode -- the floor the frames' own 1 cm noise sets, so the two bounds stand
    4.6 and 4.8 times above the twin's worst, not the 5 times asked for."""
    survey, drive, p, poses_in = _truth_inputs()
    bare = synth.tunnel_drive(8, 20_000, seed=22, patches=())         # the same draws: a point differs iff a patch moved it
    a = wn.design_frame(p)["a"]
    patch_points = 0
    worst = {ln.DESIGN: [0.0, 0.0], ln.MAP: [0.0, 0.0]}
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        for (cloud, true), (cloud0, _), pin in zip(drive["frames"], bare["frames"], poses_in):
            patch = np.any(cloud0 != cloud, axis=1)
            patch_points += int(patch.sum())
            for ref in (ln.DESIGN, ln.MAP):
                info, _, _ = m.locate_points(cloud, pin, reference=ref, outputs=False)
                assert info["status"] == _lib.GM_LOCATE_OK and info["passes"] == 3
                assert wn.pose_ok(info["pose"])
                lat, ang = pose_errors(p, info["pose"], true)
                lat0, ang0 = pose_errors(p, pin, true)
                print(f"ref={ref}: in {lat0:.4f} m {ang0:.5f} rad -> out {lat:.2e} m {ang:.2e} rad, used "
                      f"{[q['used'] for q in info['pass']]}, gated {[q['gated'] for q in info['pass']]}, patch {int(patch.sum())}")
                worst[ref] = [max(worst[ref][0], lat), max(worst[ref][1], ang)]
                assert lat <= LATERAL_BOUND and ang <= ANGLE_BOUND
                assert abs((info["pose"][:, 3] - pin[:, 3]) @ a) <= 1e-9          # the chainage stays the caller's
                if ref == ln.DESIGN:
                    assert info["pass"][2]["gated"] >= int(patch.sum())           # the patches lie 0.15 m off the design
                # idempotence: located again from the returned pose, nothing moves
                again, _, _ = m.locate_points(cloud, info["pose"], reference=ref, outputs=False)
                assert again["status"] == _lib.GM_LOCATE_OK
                assert np.linalg.norm(again["pass"][0]["step"]) <= _lib.GM_FIT_STEP_BOUND
                lat2, ang2 = pose_errors(p, again["pose"], info["pose"])
                assert lat2 < LATERAL_BOUND and ang2 < ANGLE_BOUND
    print("worst:", worst, "patch points:", patch_points)
    assert patch_points > 1000


def test_located_pose_clears_the_check(gm):
    """End to end on the bare wall: under the perturbed pose the check reports changed points, under the located pose none."""
    survey, drive, p, poses_in = _truth_inputs(patches=())
    ck = dict(threshold=0.05, min_count=4)
    changed_in = changed_out = 0
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        for (cloud, _true), pin in zip(drive["frames"], poses_in):
            info, _, _ = m.locate_points(cloud, pin, reference=ln.MAP, min_count=4, outputs=False)
            assert info["status"] == _lib.GM_LOCATE_OK
            i0, _, _ = m.check_points(cloud, pin, outputs=False, **ck)
            i1, _, _ = m.check_points(cloud, info["pose"], outputs=False, **ck)
            changed_in += i0["changed_pos"] + i0["changed_neg"]
            changed_out += i1["changed_pos"] + i1["changed_neg"]
            assert i1["unchanged"] > 10_000
    print("changed under the perturbed poses:", changed_in, "under the located poses:", changed_out)
    assert changed_in > 0 and changed_out == 0


# ---- failures ----

def test_failures(gm):
    drive = synth.tunnel_drive(2, 5_000, seed=2)
    (cloud, pose), (cloud1, pose1) = drive["frames"]
    p = wn.params(n_stations=80, **drive["design"])
    L = _lib.load()
    info = _lib.WallLocateInfo()
    dp = np.ascontiguousarray(pose).ctypes.data_as(C.POINTER(C.c_double))
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(5_000)) as c, gm.GeometricMapping() as other:
        m = c.wall_map(**p)
        before = _map_state(m)
        # before any locate
        assert L.gm_wall_map_get_locate(m._map, 0, C.byref(info)) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_get_locate(m._map, 0, None) == _lib.GM_ERR_INVALID_ARG
        # a slot without a frame; the wrong context; a bad slot
        assert L.gm_wall_map_locate_frame(m._map, c._ctx, 1, dp, None) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_locate_frame(m._map, other._ctx, 0, dp, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_locate_frame(m._map, c._ctx, 7, dp, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_locate(m._map, 7, C.byref(info)) == _lib.GM_ERR_INVALID_ARG
        c.process_frame(cloud1)
        # a bad pose; a bad parameter
        nan = pose1.copy()
        nan[1, 3] = np.nan
        for bad in (nan, pose1 * 1.01):
            with pytest.raises(gm.GmError) as e:
                m.locate_frame(0, bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        for kw in (dict(reference=2), dict(min_count=0), dict(gate=0.0), dict(gate=8.5)):
            with pytest.raises(gm.GmError) as e:
                m.locate_frame(0, pose1, **kw)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
            with pytest.raises(gm.GmError) as e:
                m.locate_points(cloud, pose, **kw)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_locate(m._map, 0, C.byref(info)) == _lib.GM_ERR_NOT_READY
        # a MAP locate on an empty map: every point that is not plane is unsurveyed
        m.locate_frame(0, pose1, reference=ln.MAP)
        r = m.locate_result(0)
        n = r["n_points"]
        assert n > 1000 and r["status"] == _lib.GM_LOCATE_DEGENERATE and r["passes"] == 0 and _pose_is_nan(r)
        assert r["pass"][0]["unsurveyed"] == n - r["pass"][0]["plane"] and r["pass"][0]["used"] == 0
        assert np.all(np.isnan(r["pass"][0]["step"])) and np.isnan(r["pass"][0]["rms"])
        assert r["pass"][1]["gate"] == 0 and r["pass"][2]["gate"] == 0             # the passes behind the failure did not run
        assert L.gm_wall_map_get_locate(m._map, 1, C.byref(info)) == _lib.GM_ERR_NOT_READY
        assert m.locate_result(0)["bytes"] == r["bytes"]                           # readable again
        # every point at one sensor x under an identity rotation: one t, so the tilt is unobservable
        rng = np.random.default_rng(5)
        phi = rng.uniform(0, 2 * np.pi, 500)
        ring = np.stack([np.full(500, 0.5), 2.0 * np.cos(phi), 2.0 * np.sin(phi)], axis=1).astype(np.float32)
        r, res, cell = m.locate_points(ring, synth.pose_matrix((10.0, 0.01, -0.02)))
        assert r["status"] & _lib.GM_LOCATE_FAILED_MASK and r["status"] == _lib.GM_LOCATE_SINGULAR and _pose_is_nan(r)
        assert r["pass"][0]["used"] == 500 and r["passes"] == 0
        # the stage call took slot 0: it holds no frame
        with pytest.raises(gm.GmError) as e:
            m.locate_frame(0, pose1)
        assert e.value.status == _lib.GM_ERR_NOT_READY
        # a frame whose n_valid is 0
        res0 = c.process_frame(np.full((100, 3), 50.0, np.float32))
        assert res0["n_valid"] == 0
        m.locate_frame(0, pose1)
        r = m.locate_result(0)
        assert r["n_points"] == 0 and r["status"] == _lib.GM_LOCATE_DEGENERATE and _pose_is_nan(r)
        assert _map_state(m) == before
        # a map destroyed with a locate outstanding frees cleanly; so does the context with one
        c.submit_frame(1, cloud1)
        m.locate_frame(1, pose1)
        m.close()
        c.wait_frame(1)
        m2 = c.wall_map(**p)
        c.submit_frame(0, cloud1)
        m2.locate_frame(0, pose1)


# ---- frame path = stage path ----

N_FRAME = 20_000


@pytest.mark.parametrize("graph", (False, True))
def test_frame_path_equals_stage_path(gm, graph):
    survey = synth.tunnel_drive(4, N_FRAME, seed=31)
    drive = synth.tunnel_drive(4, N_FRAME, seed=32)
    p = wn.params(n_stations=192, **drive["design"])
    rng = np.random.default_rng(33)
    clouds = [f[0] for f in drive["frames"]]
    poses = [perturbed(f[1], rng) for f in drive["frames"]]
    flags = PLANE | (_lib.GM_CFG_GRAPH if graph else 0)
    lk = dict(reference=ln.MAP, min_count=4)
    L = _lib.load()
    live = L.gm_debug_live_buffers()
    with gm.GeometricMapping(flags=flags, n_slots=2, neighborRadius=synth.fixed_k_radius(N_FRAME), **KW) as c:
        m = c.wall_map(**p)
        created = L.gm_debug_live_buffers()
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        assert L.gm_debug_live_buffers() > created
        with_adds = L.gm_debug_live_buffers()
        before = _map_state(m)
        for k in range(2):
            c.submit_frame(0, clouds[k])                      # right behind the submit
            m.locate_frame(0, poses[k], **lk)
            streamed = m.locate_result(0)
            c.wait_frame(0)
            assert m.locate_result(0)["bytes"] == streamed["bytes"]
            m.locate_frame(0, poses[k], **lk)                 # after the wait
            waited = m.locate_result(0)
            m.locate_frame(0, poses[k], reference=ln.DESIGN)
            design = m.locate_result(0)
            xyz, _rows = c.cropped_cloud(0)
            lab = c.labels(0)
            assert streamed["status"] == _lib.GM_LOCATE_OK and streamed["n_points"] == len(xyz) > 10_000
            assert streamed["pass"][0]["plane"] == int((lab == 1).sum())
            staged, _, _ = m.locate_points(xyz, poses[k], labels=lab, outputs=False, **lk)
            assert staged["bytes"] == streamed["bytes"] == waited["bytes"], k
            staged, _, _ = m.locate_points(xyz, poses[k], labels=lab, outputs=False, reference=ln.DESIGN)
            assert staged["bytes"] == design["bytes"] != streamed["bytes"], k
        assert L.gm_debug_live_buffers() > with_adds          # the locate's scratch, allocated on first use
        assert _map_state(m) == before
    assert L.gm_debug_live_buffers() == live


def test_ordering_across_slots(gm):
    """An add enqueued on slot 1 before the locate on slot 0 is seen; one enqueued after it is not."""
    drive = synth.tunnel_drive(2, N_FRAME, seed=41, patches=())
    (cloud0, pose0), (cloud1, pose1) = drive["frames"]                # (3.5 m apart: the frames overlap)
    p = wn.params(n_stations=192, **drive["design"])
    pin = perturbed(pose0, np.random.default_rng(42))
    lk = dict(reference=ln.MAP, min_count=1)
    kw = dict(n_slots=2, neighborRadius=synth.fixed_k_radius(N_FRAME))
    with gm.GeometricMapping(**kw) as c:
        held = c.wall_map(**p)                                        # a map that already holds frame 1
        c.process_frame(cloud1)
        held.add_frame(0, pose1)
        held.sync()
        c.process_frame(cloud0)
        held.locate_frame(0, pin, **lk)
        want = held.locate_result(0)
        assert want["status"] == _lib.GM_LOCATE_OK and want["pass"][0]["unsurveyed"] > 0 and want["pass"][0]["used"] > 1000
        m = c.wall_map(**p)                                           # an empty map, nothing waited for in between
        c.submit_frame(1, cloud1)
        m.add_frame(1, pose1)
        c.submit_frame(0, cloud0)
        m.locate_frame(0, pin, **lk)
        c.wait_frame(1)
        c.submit_frame(1, cloud0)
        m.add_frame(1, pose0)                                         # enqueued after the locate: not seen
        got = m.locate_result(0)
        c.wait_frame(0)
        c.wait_frame(1)
        m.sync()
        assert got["bytes"] == want["bytes"]
        assert m.info()["frames"] == 2
