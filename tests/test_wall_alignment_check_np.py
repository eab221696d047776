"""CPU tests of the alignment check's twin (tests/wall_alignment_check_np.py), built from include/gm_hip.h: every point in
exactly one (side, class), the rows of a side against wall_check_np.check of the sub-cloud it owns, and the shared
assertions against two deliberately wrong twins."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_check_np as acn  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_check_np as wc  # noqa: E402
import wall_np as wn  # noqa: E402

N = lc.N
BOUND = 5.0   # boxFilterBound of the alignment tests
CASES = ("clothoid_arc:before", "arc_arc:after", "straight_clothoid:after", "three_sides", "four_sides")


def _case(case, **kw):
    """(cloud with a block of points displaced radially by +-0.3 m, labels, plan, grid, n_stations and raws per side)."""
    els, s, sides = lc.record_case(case)
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    grid = dict(p)
    nst_of = lambda i: rule.element_params(i)[0].n_stations   # noqa: E731
    survey = [al_np.frame(rule, s + d, N, seed=70 + k) for k, d in enumerate((-0.5, 0.0, 0.5))]
    raws_of = aln.survey_raws(survey, rule, grid, nst_of, BOUND, gate=p.get("gate", 0.25))
    cloud, pose = al_np.frame(rule, s, N, seed=71)   # (the middle survey frame's wall, seen again)
    r = np.linalg.norm(cloud[:, 1:], axis=1, keepdims=True)
    k = np.arange(N)
    scale = np.where((k % 16 == 3)[:, None], (r + 0.3) / r, np.where((k % 16 == 11)[:, None], (r - 0.3) / r, 1.0))
    cloud = cloud.copy()
    cloud[:, 1:] = (cloud[:, 1:] * scale).astype(np.float32)   # (about the sensor's x axis, which runs along the tunnel)
    labels = (k % 23 == 0).astype(np.uint8)
    plan = rule.locate_plan(pose, BOUND)
    assert plan["add"]["n_sides"] == sides
    nst = [nst_of(i) for i in plan["add"]["side_element"]]
    raws = [raws_of.get(i, np.zeros(nst_of(i) * p["n_sectors"], wn.RAW_CELL)) for i in plan["add"]["side_element"]]
    return cloud, labels, plan, grid, nst, raws


@pytest.mark.parametrize("reference", (wc.MEAN, wc.ENVELOPE))
@pytest.mark.parametrize("case", CASES)
def test_every_point_in_one_side_and_class(case, reference):
    cloud, labels, plan, grid, nst, raws = _case(case)
    kw = dict(reference=reference, min_count=2, threshold=0.05, gate=1.0)
    t = acn.check(cloud, labels, plan, grid, nst, raws, **kw)
    acn.assert_partition(t, cloud, labels, plan["add"], raws, **kw)
    info = t["info"]
    print(case, {q: info[q] for q in wc.NAMES})
    assert info["plane"] == int(labels.sum())
    # the displaced block shows in both changed classes, and on both sides of a joint
    changed = info["side_class"][:, wc.CHANGED_POS].astype(int) + info["side_class"][:, wc.CHANGED_NEG]
    assert info["changed_pos"] > 50 and info["changed_neg"] > 50 and int((changed > 10).sum()) >= 2
    assert info["unchanged"] > 0.3 * N
    s, c = acn.split_cell(t["rows"])
    assert np.array_equal(s, t["side"][t["rows"]["index"]]) and np.array_equal(c, t["cell"][t["rows"]["index"]])


@pytest.mark.parametrize("fault,case", (("neighbour_table", "clothoid_arc:before"), ("joint_order", "three_sides"),
                                        ("joint_order", "four_sides"), ("neighbour_table", "four_sides")))
def test_a_wrong_twin_fails(fault, case):
    cloud, labels, plan, grid, nst, raws = _case(case)
    kw = dict(reference=wc.MEAN, min_count=2, threshold=0.05, gate=1.0)
    good = acn.check(cloud, labels, plan, grid, nst, raws, **kw)
    acn.assert_partition(good, cloud, labels, plan["add"], raws, log=lambda *_: None, **kw)
    bad = acn.check(cloud, labels, plan, grid, nst, raws, fault=fault, **kw)
    with pytest.raises(AssertionError):
        acn.assert_partition(bad, cloud, labels, plan["add"], raws, log=lambda *_: None, **kw)


def test_one_side_is_the_element_maps_check():
    """With one side the rows carry side 0: the cell field is the element map's, bit for bit."""
    els, s, sides = lc.record_case("arc")
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    cloud, pose = al_np.frame(rule, s, 500, seed=5)
    plan = rule.locate_plan(pose, BOUND)
    nst = [rule.element_params(i)[0].n_stations for i in plan["add"]["side_element"]]
    raws = aln.survey_raws([(cloud, pose)], rule, dict(p), lambda i: nst[0], BOUND)
    raws = [raws[plan["add"]["side_element"][0]]]
    far = cloud.copy()
    far[::5, 1:] *= np.float32(1.1)
    t = acn.check(far, None, plan, dict(p), nst, raws, min_count=1)
    assert sides == 1 and len(t["rows"]) > 50 and np.all(t["rows"]["cell"] >= 0) and np.all(t["rows"]["cell"] < nst[0] * 90)
    ri, rr = wc.check(far, t["e"], t["cell"], raws[0], min_count=1)
    assert rr.tobytes() == t["rows"].tobytes()
