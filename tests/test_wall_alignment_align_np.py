"""CPU tests of the alignment align's twin (tests/wall_alignment_align_np.py), built from include/gm_hip.h: every point in
exactly one (side, class), the truth of shifted poses on a textured wall across two joints (whose worst errors are the
constants the GPU test's bounds come from), the loop the align closes, and three deliberately wrong twins."""
import functools
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_align_np as an  # noqa: E402
import wall_alignment_align_cases as ac  # noqa: E402
import wall_alignment_align_np as aan  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_np as wn  # noqa: E402


@functools.lru_cache(maxsize=None)
def _truth(case):
    """(rule, grid, s, twin survey, the truth frame, its true pose)."""
    rule, grid, s, _ = ac.rule_of(api, case)
    raws = ac.twin_survey(rule, grid, s)
    cloud, true = ac.textured_frame(rule, s, ac.TRUTH_N, seed=ac.TRUTH_SEED)
    return rule, grid, s, raws, cloud, true


@functools.lru_cache(maxsize=None)
def _small(case):
    """The same wall on 4 000-point frames: (rule, grid, s, sides, raws, cloud with labels, true pose)."""
    rule, grid, s, sides = ac.rule_of(api, case)
    raws = ac.twin_survey(rule, grid, s, n=ac.N)
    cloud, true = ac.textured_frame(rule, s, ac.N, seed=ac.TRUTH_SEED)
    return rule, grid, s, sides, raws, cloud, true


@pytest.mark.parametrize("case", ac.PARITY_CASES)
def test_every_point_in_one_side_and_class(case):
    rule, grid, s, sides, raws, cloud, true = _small(case)
    lab = (np.arange(len(cloud)) % 23 == 0).astype(np.uint8)
    far = cloud.copy()
    far[np.arange(len(cloud)) % 11 == 3] *= np.float32(1.25)   # beyond the gate
    pose = ac.moved(rule, s, 1, -1, grid)
    ap = ac.prm(half_patch_stations=12)                        # 3 m of the frame's 4.5: the far points are outside the patch
    out, tab = aan.align(far, lab, rule, pose, ac.BOUND, raws, grid, ap)
    print(case, {q: out[q] for q in an.CLASSES}, out["side_class"].tolist(), out["twin_plan"])
    assert out["n_sides"] == sides and out["plane"] == int(lab.sum())
    assert int(out["side_class"].sum()) == len(cloud) == sum(out[q] for q in an.CLASSES)
    assert all(out[q] > 0 for q in an.CLASSES)
    pts = out["points"]
    assert np.all(pts["cell"][pts["cls"] == aan.BINNED] >= 0) and np.all(pts["cell"][pts["cls"] != aan.BINNED] == -1)
    assert np.all(pts["cell"] < 2 * 12 * grid["n_sectors"])
    if sides >= 2:   # both sides of a joint bin
        assert int((out["side_class"][:, aan.BINNED] > 0).sum()) >= 2
    assert tab.shape == (2 * ap["max_station_shift"] + 1, 2 * ap["max_sector_shift"] + 1)
    # the plan's integers: the rows of the patch are consecutive global stations whichever side bins them
    pl = out["twin_plan"]
    base = aan.bases([rule.element_params(i)[0].n_stations for i in range(rule.n_elements)])
    for k, (i, a) in enumerate(zip(out["add"]["side_element"], out["add"]["side_anchor"])):
        assert pl["row0"][k] == base[i] + a - pl["anchor_global"] + 12


def test_truth_and_the_constants():
    """Whole-cell shifts come back exactly with the flags clear; the worst error over FRACTIONAL is what the constants say."""
    worst = [0.0, 0.0]
    for case in ac.TRUTH_CASES:
        rule, grid, s, raws, cloud, true = _truth(case)
        for sa, sb in ac.WHOLE[:2]:
            out, _ = aan.align(cloud, None, rule, ac.moved(rule, s, sa, sb, grid), ac.BOUND, raws, grid, ac.prm())
            assert (out["status"], out["best_station"], out["best_sector"]) == (an.OK, sa, sb), (case, sa, sb, out["distinction"])
        for sa, sb in ac.FRACTIONAL:
            out, _ = aan.align(cloud, None, rule, ac.moved(rule, s, sa, sb, grid), ac.BOUND, raws, grid, ac.prm())
            es, ek = ac.shift_error(out, sa, sb)
            print(f"{case} ({sa}, {sb}): best ({out['best_station']}, {out['best_sector']}) + ({out['frac_station']:.4f}, "
                  f"{out['frac_sector']:.4f}): errors {es:.4f} station, {ek:.4f} sector; distinction {out['distinction']:.2f}")
            assert not out["status"] & an.FAILED_MASK
            worst = [max(worst[0], es), max(worst[1], ek)]
            # the pose moves the caller onto the true pose: within the shift's error along and around the axis
            dt = np.linalg.norm(out["pose"][:, 3] - true[:, 3])
            assert dt <= (es + 0.01) * grid["station_length"] + 1e-9, (case, dt)
    print("worst:", worst)
    assert worst[0] <= ac.TWIN_WORST_STATION and worst[1] <= ac.TWIN_WORST_SECTOR
    assert worst[0] >= 0.9 * ac.TWIN_WORST_STATION and worst[1] >= 0.9 * ac.TWIN_WORST_SECTOR   # (the constants are these)


def test_closing_the_loop_and_its_constants():
    rule, grid, s, raws, cloud, true = _truth("clothoid_arc:before")
    off = ac.moved(rule, s, *ac.LOOP_SHIFT, grid)
    out, _ = aan.align(cloud, None, rule, off, ac.BOUND, raws, grid, ac.prm())
    assert (out["best_station"], out["best_sector"]) == ac.LOOP_SHIFT
    got = tuple(ac.twin_changed(rule, grid, raws, cloud, p, **ac.LOOP_CHECK) for p in (out["pose"], true, off))
    print("changed under the aligned, the true and the caller's pose:", got)
    assert got == (ac.LOOP_TWIN_ALIGNED, ac.LOOP_TWIN_TRUE, ac.LOOP_TWIN_OFF)
    assert got[2] > 10 * max(got[0], got[1])   # a pose two stations off reports the wall; the aligned one does not


@pytest.mark.parametrize("fault,case", (("row0_of_sensor_side", "straight_clothoid:after"), ("row0_of_sensor_side", "four_sides"),
                                        ("neighbour_rows_none", "clothoid_arc:before"), ("neighbour_rows_none", "three_sides"),
                                        ("pose_on_tangent", "clothoid_arc:before"), ("pose_on_tangent", "arc_arc:after")))
def test_a_wrong_twin_shows(fault, case):
    """Each named fault changes the table or the pose on a joint case."""
    rule, grid, s, sides, raws, cloud, true = _small(case)
    pose = ac.moved(rule, s, 3, 1, grid)
    ap = ac.prm()
    good, gt = aan.align(cloud, None, rule, pose, ac.BOUND, raws, grid, ap)
    bad, bt = aan.align(cloud, None, rule, pose, ac.BOUND, raws, grid, ap, fault=fault)
    if fault == "row0_of_sensor_side":
        assert len(set(good["twin_plan"]["row0"].tolist())) > 1   # (the case's anchors differ: the fault can show)
        assert gt.tobytes() != bt.tobytes()
        assert not np.array_equal(good["points"]["cell"], bad["points"]["cell"])
    elif fault == "neighbour_rows_none":
        assert gt.tobytes() != bt.tobytes()
        assert np.all(bt["n"] <= gt["n"]) and int(bt["n"].sum()) < int(gt["n"].sum())   # the table loses overlap
    else:
        assert gt.tobytes() == bt.tobytes() and good["shift_m"] == bad["shift_m"] != 0.0
        d = np.abs(good["pose"] - bad["pose"]).max()
        print("pose difference:", d)
        assert d > 1e-4                                           # the curve ahead moves the sensor off the tangent
        # ... and only the good pose turns with the axis: the sensor's heading against the true one (a roll error about
        # the axis moves a heading 3 degrees off it by a twentieth of itself)
        heading = lambda q: float(np.linalg.norm(q[:, 0] - true[:, 0]))   # noqa: E731
        print("heading errors:", heading(good["pose"]), heading(bad["pose"]))
        assert heading(good["pose"]) < 0.2 * heading(bad["pose"])


def test_one_straight_side_is_the_element_maps_align():
    """Mid-straight, the image inside the element: the twin of the map's align gives the same table and pose."""
    els = al_np.elements5(n_straight=160, n_clothoid=160, n_arc=160)
    p = dict(n_sectors=90, station_length=al_np.DS, radius=al_np.RADIUS)
    rule = api.WallAlignmentRule(els, **p)
    s = 20.0
    cloud, true = ac.textured_frame(rule, s, ac.N, seed=3)
    raws = ac.twin_survey(rule, dict(p), s, n=ac.N, offsets=(-1.0, 0.0, 1.0))
    pose = ac.moved(rule, s, 2, -1, dict(p))
    ap = ac.prm()
    out, tab = aan.align(cloud, None, rule, pose, ac.BOUND, raws, dict(p), ap)
    assert out["twin_plan"]["own"] == 1 and out["n_sides"] == 1
    ep = rule.element_params(0)[0]
    mp = wn.params(n_stations=ep.n_stations, n_sectors=ep.n_sectors, station_length=ep.station_length, radius=ep.radius,
                   t_min=ep.t_min, point=list(ep.point), direction=list(ep.direction), up=list(ep.up), forward=list(ep.forward))
    frame = wn.add_frame(wn.design_frame(mp), mp, pose)
    assert frame["anchor"] == out["twin_plan"]["anchor_global"]
    pts = out["points"]
    e32 = np.where(np.isnan(pts["e"]), np.float32(0), pts["e"]).astype(np.float32)
    psum, pcnt = an.patch_from(e32, pts["cell"], 2 * ap["half_patch_stations"] * 90)
    mt = an.table(psum, pcnt, raws[0], frame["anchor"], 90, ap)
    assert mt.tobytes() == tab.tobytes()
    sel = an.select(mt, mp, pose, ap)
    assert sel["status"] == out["status"] and np.allclose(sel["pose"], out["pose"], rtol=0.0, atol=1e-12)
    # the image reaching over the element's end into the clothoid: no longer the map's own
    near = ac.moved(rule, 39.0, 0, 0, dict(p))
    pl = rule.align_plan(near, ac.BOUND, **ac.AP)
    assert pl["own"] == 0 and pl["add"]["n_sides"] == 2
