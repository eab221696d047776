"""GPU tests of the locate on a wall alignment (gm_wall_alignment_locate_*): one straight side is the element map's own
locate byte for byte; on curved sides and across joints the pass records are the twin's (tests/wall_alignment_locate_np.py)
evaluated on the blocks each record reports; a perturbed pose comes back to the true one within five times the fp64
twin's own error; the located pose clears the element maps' checks; sizes, failures, the frame path and the ordering
against adds.  Frames are wall_alignment_np.frame's: 4 000 points, 90 sectors, ds 0.25, boxFilterBound 5."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curved_chain_cases as cc  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
N = lc.N
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
SIZES = (0, 3, 4, 5, 63, 64, 65, 1025, 4097, 131071, 131072, 131073, 524288, 524289)   # test_gpu_wall_locate.py's grid edges


def _states(al):
    out = []
    for i in range(al.n_elements):
        m = al.element(i)
        info = m.info()
        out.append((m.read_raw().tobytes(), tuple(info[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))))
    return out


def _pose_is_nan(info):
    return bool(np.all(np.isnan(info["pose"])) and np.all(np.isnan(info["lateral"])) and np.all(np.isnan(info["tilt"])))


def _nst(al, info):
    return [al.element_params(i)[0].n_stations for i in info["side_element"]]


@pytest.mark.parametrize("ref", (aln.DESIGN, aln.MAP))
def test_one_straight_side_is_the_element_maps_locate(gm, ref):
    els = al_np.elements5(n_straight=160, n_clothoid=160, n_arc=160)[:3]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    cloud, pose = al_np.frame(rule, 20.0, N, seed=3)
    pin = lc.perturbed(pose, np.random.default_rng(1))
    lab = (np.arange(N) % 9 == 0).astype(np.uint8)
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        for s in (18.5, 21.5):
            al.add_points(*al_np.frame(rule, s, N, seed=3), outputs=False)
        kw = dict(reference=ref, min_count=1)
        info, res, cell, el = al.locate_points(cloud, pin, labels=lab, **kw)
        own, res0, cell0 = al.element(0).locate_points(cloud, pin, labels=lab, **kw)
        assert info["n_sides"] == 1 and info["side_kind"] == [0] and np.all(el == 0)
        assert info["status"] == _lib.GM_LOCATE_OK and info["pass"][2]["used"] > 0.7 * N
        assert info["bytes"][4:152] == own["bytes"][4:152]                      # everything but struct_size
        for k in range(3):
            a, b = 320 + 376 * k, 152 + 112 * k
            assert info["bytes"][a:a + 112] == own["bytes"][b:b + 112], k
            assert np.array_equal(info["pass"][k]["side"][0].reshape(-1), np.concatenate([own["pass"][k][q] for q in "oauv"]))
        assert np.array_equal(res.view(np.uint32), res0.view(np.uint32)) and np.array_equal(cell, cell0)
        assert al.locate_result(0)["bytes"] == info["bytes"]


@pytest.mark.parametrize("case", lc.RECORD_CASES)
def test_pass_records_against_the_twin(gm, case):
    els, s, sides = lc.record_case(case)
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    cloud, pose = al_np.frame(rule, s, N, seed=11)
    pin = lc.perturbed(pose, np.random.default_rng(7))
    lab = (np.arange(N) % 7 == 0).astype(np.uint8)
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        plan = al.locate_plan(pin)
        assert plan["add"]["n_sides"] == sides
        for ref in ((aln.DESIGN, aln.MAP) if case in lc.MAP_RECORD_CASES else (aln.DESIGN,)):
            raws = None
            if ref == aln.MAP:
                for ds_ in lc.SURVEY_OFFSETS:
                    al.add_points(*al_np.frame(rule, s + ds_, N, seed=11), outputs=False)
                raws = [al.element(i).read_raw() for i in plan["add"]["side_element"]]
            before = _states(al)
            info, res, cell, el = al.locate_points(cloud, pin, labels=lab, reference=ref, min_count=2)
            assert info["status"] == _lib.GM_LOCATE_OK and info["passes"] == 3 and info["n_points"] == N
            assert info["n_sides"] == sides and info["side_element"] == plan["add"]["side_element"]
            assert info["anchor_station"] == plan["add"]["side_anchor"][plan["home"]] and info["element"] == plan["add"]["element"]
            assert np.array_equal(el, al_np.owner32(cloud, dict(n_sides=sides, side_element=info["side_element"],
                                                               joint_o=info["pass"][0]["joint_o"], joint_a=info["pass"][0]["joint_a"])))
            # pass 0's blocks are the plan's images under the start, as the twin forms them (the last bit is the host's)
            b0 = aln.blocks(plan, dict(o=plan["c"], a=plan["d"], u=plan["u"], v=plan["v"]))
            assert np.abs(info["pass"][0]["side"].astype(np.float64) - b0["side"]).max() <= 1e-6
            worst = aln.assert_passes(info, cloud, lab, info, p, _nst(al, info), plan["s0"], raws=raws, min_count=2, res=res, cell=cell,
                                      element=el, start=plan)
            print(f"{case} ref={ref}: worst |step - twin| {worst[0]:.2e}, |rms - twin| {worst[1]:.2e}; used {[q['used'] for q in info['pass']]}")
            assert info["pass"][2]["used"] > 0.5 * N
            assert _states(al) == before


@pytest.mark.parametrize("ref", (aln.DESIGN, aln.MAP))
def test_truth(gm, ref):
    """Every joint frame (1 m before and after each of the five joints) and a frame in mid-arc and in mid-clothoid, located
    from the true pose moved by up to 0.05 m across the axis and 0.5 degrees in yaw and pitch; DESIGN, and MAP against a
    survey of the same wall added at the true poses.  The bounds are wall_alignment_locate_cases.TRUTH_BOUNDS: five times the
    fp64 twin's worst on these inputs, which tests/test_wall_alignment_locate_np.py computes."""
    p = lc.prm()
    lat_b, ang_b, ch_b = lc.TRUTH_BOUNDS[ref]
    worst = [0.0, 0.0, 0.0]
    with gm.GeometricMapping() as c:
        for name, els, s in lc.truth_frames():
            rule = api.WallAlignmentRule(els, **p)
            al = c.wall_alignment(els, **p)
            cloud, true, pin = lc.truth_input(rule, name, s)
            if ref == aln.MAP:
                for ds_ in lc.SURVEY_OFFSETS:
                    al.add_points(*al_np.frame(rule, s + ds_, N, seed=lc.TRUTH_SEED), outputs=False)
            info, _, _, _ = al.locate_points(cloud, pin, reference=ref, min_count=2, outputs=False)
            assert info["status"] == _lib.GM_LOCATE_OK and info["passes"] == 3 and wn.pose_ok(info["pose"])
            lat, ang, ch = lc.pose_errors(rule, info["pose"], true, pin)
            lat0, ang0, _ = lc.pose_errors(rule, pin, true, pin)
            print(f"{name} ref={ref}: in {lat0:.4f} m {ang0:.5f} rad -> out {lat:.2e} m {ang:.2e} rad, chainage moved {ch:.2e} m, "
                  f"used {[q['used'] for q in info['pass']]}")
            worst = [max(a, b) for a, b in zip(worst, (lat, ang, ch))]
            assert lat <= lat_b and ang <= ang_b and ch <= ch_b
            again, _, _, _ = al.locate_points(cloud, info["pose"], reference=ref, min_count=2, outputs=False)
            assert again["status"] == _lib.GM_LOCATE_OK
            assert np.linalg.norm(again["pass"][0]["step"]) <= _lib.GM_FIT_STEP_BOUND
            al.close()
    print(f"ref={ref} worst: lateral {worst[0]:.2e} m, angle {worst[1]:.2e} rad, chainage {worst[2]:.2e} m")


def test_located_pose_clears_the_checks(gm):
    """End to end across the clothoid -> arc joint on the bare wall: under the perturbed pose the element maps' checks report
    changed points, under the located pose none."""
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    ck = dict(threshold=0.03, min_count=2)
    changed_in = changed_out = unchanged_out = 0
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        for k, s in enumerate(np.arange(sj - 4.0, sj + 4.01, 1.0)):
            al.add_points(*al_np.frame(rule, s, N, seed=61, sigma=0.002), outputs=False)
        for k, s in enumerate((sj - 1.0, sj + 1.0)):
            cloud, true = al_np.frame(rule, s + 0.37, N, seed=61, sigma=0.002)
            pin = lc.perturbed(true, np.random.default_rng(70 + k))
            info, _, _, _ = al.locate_points(cloud, pin, reference=aln.MAP, min_count=2, outputs=False)
            assert info["status"] == _lib.GM_LOCATE_OK and info["n_sides"] == 2
            for i in info["side_element"]:
                i0, _, _ = al.element(i).check_points(cloud, pin, outputs=False, **ck)
                i1, _, _ = al.element(i).check_points(cloud, info["pose"], outputs=False, **ck)
                changed_in += i0["changed_pos"] + i0["changed_neg"]
                changed_out += i1["changed_pos"] + i1["changed_neg"]
                unchanged_out += i1["unchanged"]
    print("changed under the perturbed poses:", changed_in, "under the located poses:", changed_out, "unchanged:", unchanged_out)
    assert changed_in > 0 and changed_out == 0 and unchanged_out > N


def test_sizes(gm):
    """n in {0, 3, 4, 5} and the fit grid's edges across the arc -> arc joint, against the twin with its chains in fp64 (as
    tests/test_gpu_wall_locate.py's sweep does): class counts within the twin's ambiguous points, step and rms within 1e-6."""
    els, j = lc.JOINTS["arc_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    base, pose = al_np.frame(rule, sj - 1.0, N, seed=81)
    pin = lc.perturbed(pose, np.random.default_rng(81))
    s0 = rule.locate_plan(pin, 5.0)["s0"]
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        before = _states(al)
        for n in SIZES:
            xyz = np.ascontiguousarray(np.tile(base, ((n + N - 1) // N or 1, 1))[:n])
            lab = (np.arange(n) % 7 == 0).astype(np.uint8)
            info, res, cell, el = al.locate_points(xyz, pin, labels=lab)
            assert info["n_points"] == n and info["n_sides"] == 2
            failed = bool(info["status"] & aln.FAILED_MASK)
            assert failed == _pose_is_nan(info)
            if n < 5:   # (every seventh point is plane: at most three are used)
                assert info["status"] == _lib.GM_LOCATE_DEGENERATE and info["passes"] == 0
                assert info["pass"][0]["plane"] == int(lab.sum()) and np.all(np.isnan(info["pass"][0]["step"]))
                assert info["pass"][1]["used"] == 0 and info["pass"][1]["gate"] == 0.0
                continue
            # (below 64 points the normal equations are too poorly conditioned for a bound on the step: classes alone)
            worst = aln.assert_passes(info, xyz, lab, info, p, _nst(al, info), s0, res=res, element=el, exact=True,
                                      tol=1e-6 if n >= 64 else np.inf)
            print(f"n={n}: status {info['status']} used {[q['used'] for q in info['pass']]} worst {worst}")
            assert n < 64 or not failed
            assert int((~np.isnan(res)).sum()) == info["pass"][info["passes"] if failed else 2]["used"]
            assert np.all(cell == -1)
        assert _states(al) == before


def _guard_alignment(c, g):
    """The single-element alignment whose element map is the guard case's map."""
    p = {k: g["p"][k] for k in ("n_sectors", "station_length", "t_min", "gate", "point", "direction", "radius", "up", "forward")}
    turn = (0.8, -0.6)   # OBLIQUE = 0.8 u + (-0.6) v with u = +z, v = a x u = -y
    n = int(g["p"]["n_stations"])
    if g["kind"] == "arc":
        el = dict(kind="arc", n_stations=n, turn=turn, curvature=1.0 / cc.G_ARC["arc_radius"])
    else:
        el = dict(kind="clothoid", n_stations=n, turn=turn, curvature=0.0, rate=cc.G_RATE)
    return c.wall_alignment([el], **p), p


@pytest.mark.parametrize("name", cc.GUARD_NAMES)
def test_guard_classes_are_gated(gm, name):
    """The guard clouds of tests/curved_chain_cases.py on a single-element alignment: every guard point is gated in every
    pass, and the steps are bit for bit those of the same cloud with the guard points labelled plane: they leave the sums
    untouched."""
    g = cc.guard_case(name)
    with gm.GeometricMapping() as c:
        al, p = _guard_alignment(c, g)
        ep, arc, cl = al.element_params(0)
        m = c.wall_map(arc=g["axis"] if g["kind"] == "arc" else None, clothoid=g["axis"] if g["kind"] != "arc" else None, **g["p"])
        assert bytes(m.prm) == bytes(ep)
        if g["kind"] == "arc":
            assert np.allclose(list(arc.curvature), list(m.arc_struct().curvature), rtol=0, atol=1e-15)
        guard = g["family"] >= 0
        info, res, cell, el = al.locate_points(g["cloud"], g["pose"], labels=g["labels"])
        assert info["status"] == _lib.GM_LOCATE_OK and info["n_sides"] == 1 and info["side_kind"] == [1 if g["kind"] == "arc" else 2]
        assert np.all(np.isnan(res[guard]))
        live_guards = int((guard & (g["labels"] != 1)).sum())
        for k in range(3):
            assert info["pass"][k]["gated"] >= live_guards and info["pass"][k]["plane"] == int((g["labels"] == 1).sum())
        lab2 = np.where(guard, 1, g["labels"]).astype(np.uint8)
        info2, res2, _, _ = al.locate_points(g["cloud"], g["pose"], labels=lab2)
        for k in range(3):
            assert info["pass"][k]["used"] == info2["pass"][k]["used"]
            assert info["pass"][k]["gated"] - info2["pass"][k]["gated"] == live_guards
            assert np.array_equal(info["pass"][k]["step"].view(np.uint64), info2["pass"][k]["step"].view(np.uint64))
        assert np.array_equal(info["pose"].view(np.uint64), info2["pose"].view(np.uint64))
        print(f"{name}: {live_guards} guard points gated; used {[q['used'] for q in info['pass']]}")


def test_failures(gm):
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    cloud, pose = al_np.frame(rule, sj - 1.0, N, seed=91)
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        al.add_points(*al_np.frame(rule, 5.0, N, seed=92), outputs=False)   # (a map that is not empty somewhere else)
        before = _states(al)
        # every point is plane
        info, res, cell, el = al.locate_points(cloud, pose, labels=np.ones(N, np.uint8))
        assert info["status"] == _lib.GM_LOCATE_DEGENERATE and info["passes"] == 0 and _pose_is_nan(info)
        assert info["pass"][0]["plane"] == N and np.all(np.isnan(res)) and set(np.unique(el)) == set(info["side_element"])
        # MAP on maps that are empty here: all unsurveyed
        info, res, cell, el = al.locate_points(cloud, pose, reference=aln.MAP)
        assert info["status"] == _lib.GM_LOCATE_DEGENERATE and _pose_is_nan(info)
        assert info["pass"][0]["unsurveyed"] + info["pass"][0]["outside"] == N and info["pass"][0]["unsurveyed"] > 0.9 * N
        assert np.all(cell[np.isfinite(cloud).all(1)] >= -1) and (cell >= 0).sum() == info["pass"][0]["unsurveyed"]
        # a frame far from the wall: everything gated
        info, _, _, _ = al.locate_points(cloud * np.float32(0.25), pose)
        assert info["status"] == _lib.GM_LOCATE_DEGENERATE and info["pass"][0]["gated"] == N and _pose_is_nan(info)
        assert _states(al) == before
        # refusals
        with pytest.raises(_lib.GmError) as ex:
            al.locate_points(cloud, pose, gate=9.0)
        assert ex.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(_lib.GmError) as ex:
            al.locate_result(1)
        assert ex.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(_lib.GmError) as ex:
            al.locate_frame(0, pose)
        assert ex.value.status == _lib.GM_ERR_NOT_READY
        many = [dict(kind="straight", n_stations=80)] + [dict(kind="arc", n_stations=4, turn=al_np.LEFT, curvature=1.0 / 80.0)] * 6 + \
               [dict(kind="straight", n_stations=80)]
        al6 = c.wall_alignment(many, **p)
        cl6, pose6 = al_np.frame(al6, 23.0, N, seed=23)
        with pytest.raises(_lib.GmError) as ex:
            al6.locate_points(cl6, pose6)
        assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
        with pytest.raises(_lib.GmError) as ex:
            al6.locate_result(0)
        assert ex.value.status == _lib.GM_ERR_NOT_READY


@pytest.mark.parametrize("graph", (False, True))
def test_frame_path_equals_stage_path(gm, graph):
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    cloud, pose = al_np.frame(rule, sj - 1.0, N, seed=41)
    pin = lc.perturbed(pose, np.random.default_rng(41))
    flags = PLANE | (_lib.GM_CFG_GRAPH if graph else 0)
    with gm.GeometricMapping(flags=flags, neighborRadius=synth.fixed_k_radius(N)) as c:
        al = c.wall_alignment(els, **p)
        for ds_ in lc.SURVEY_OFFSETS:
            al.add_points(*al_np.frame(rule, sj - 1.0 + ds_, N, seed=41), outputs=False)
        for ref in (aln.DESIGN, aln.MAP):
            for _ in range(2 if graph else 1):   # (the second frame replays the graph)
                c.process_frame(cloud)
                al.locate_frame(0, pin, reference=ref, min_count=2)
                got = al.locate_result(0)
            xyz, _ = c.cropped_cloud()
            want, _, _, _ = al.locate_points(xyz, pin, labels=c.labels(), reference=ref, min_count=2)
            assert got["n_sides"] == 2 and got["status"] == _lib.GM_LOCATE_OK and got["n_points"] == len(xyz)
            assert got["bytes"] == want["bytes"], ref


def test_ordering_against_adds(gm):
    """A MAP locate on slot 1 sees the alignment add enqueued before it on slot 0; an add enqueued after a locate, on another
    slot and through the element map, does not change its result."""
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    survey = al_np.frame(rule, sj - 1.0, N, seed=43)
    cloud, pose = al_np.frame(rule, sj - 0.5, N, seed=43)
    pin = lc.perturbed(pose, np.random.default_rng(43))
    kw = dict(neighborRadius=synth.fixed_k_radius(N))
    with gm.GeometricMapping(n_slots=2, **kw) as c:
        al = c.wall_alignment(els, **p)
        c.submit_frame(0, survey[0])
        c.submit_frame(1, cloud)
        al.add_frame(0, survey[1])
        al.locate_frame(1, pin, reference=aln.MAP, min_count=1)
        # behind the locate: more of the same wall from slot 0, through the alignment and through an element map
        al.add_frame(0, survey[1])
        al.element(j).add_frame(0, survey[1])
        got = al.locate_result(1)
        for k in range(2):
            c.wait_frame(k)
        al.sync()
        assert got["status"] == _lib.GM_LOCATE_OK and got["n_sides"] == 2
        surveyed = got["n_points"] - got["pass"][0]["unsurveyed"] - got["pass"][0]["outside"]
        print("locate behind the add:", {q: got["pass"][0][q] for q in aln.CLASSES})
        assert surveyed > 0.3 * N                          # the add on slot 0 is in the maps the locate read
        # the same locate against maps that hold the first add alone
        ref = c.wall_alignment(els, **p)
        ref.add_points(c.cropped_cloud(0)[0], survey[1], outputs=False)
        want, _, _, _ = ref.locate_points(c.cropped_cloud(1)[0], pin, reference=aln.MAP, min_count=1, outputs=False)
        assert got["bytes"] == want["bytes"]
