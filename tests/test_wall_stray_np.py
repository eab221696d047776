"""CPU conditions of tests/test_gpu_wall_stray.py, from the device-free plans (api.WallAlignmentRule) and the fp32 twins alone:
the stray clouds hold what each family needs, no stray point is uncertain in its owner's twin, every stray point has the
class its family was built for, and the GPU file's assertions fail on the outputs of five kernels that are wrong in one line.

What the searches found (counted below): on_joint (d == +0.0 exactly) exists on the straight - clothoid joint under the
identity rotation, where aJ' is an axis vector, and on every joint of the three- and four-side plans; on the oblique
planes of the other four two-side plans neither 10^6 draws in the plane nor the aimed lattice (192 032 points) found a
point beside Jo' itself, and the family is left out there.  No point with d == -0.0 was found on any plan: q = p - Jo' has no negative zero
unless a coordinate of Jo' is 0.0.  cy_in_gate and past_centre exist on every END side that is an arc, g_in_gate (the wall a
quarter turn along, inside the gate, stopped by the clothoid chain's `ok` alone: its bound on |g| or a denominator) on every
END side that is a clothoid.  A middle side owns the wedge or slab between its two planes, which holds its own wall only
near the sensor, where cy > 0 and the Newton steps converge: no guard point inside the gate is a middle side's.  On these
transitions of 20 m and less no wall point has cy < -0.05, so cy_in_gate, picked as guard_case's clothoid:turned is, has no
clothoid rows.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curved_chain_cases as cc  # noqa: E402
import test_gpu_wall_alignment as ta  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_stray_cases as sc  # noqa: E402

F = np.float32


def _twin(c, gate=None, fault=None):
    return sc.joint_twin(c["add"], c["sides"], c["cloud"], c["labels"], gate, fault=fault)


def _device_of(tw):
    """A twin's outputs in the shape of a device's: element, res, cell, and the sides' totals over the decidable rows."""
    return tw["element"], tw["e"], tw["cell"], sc.class_rows(tw, ~tw["uncertain"])


def test_the_plans_are_the_alignment_tests():
    assert sorted(ta.JOINTS) == sorted(lc.JOINTS) == list(sc.JOINT_PLANS)
    for k in ta.JOINTS:
        assert ta.JOINTS[k] == lc.JOINTS[k]


@pytest.mark.parametrize("name", sc.PLANS)
def test_case_conditions(name):
    c = sc.case(name)
    n, lab = len(c["cloud"]), c["labels"]
    s, live = sc.stray(c), c["labels"] == 0
    assert n % 64 == 1 and 1000 < n <= 4097 and np.array_equal(lab, cc.labels_of(n))
    assert np.array_equal(np.flatnonzero(s), (np.arange(n // 64)[:, None] * 64 + np.array(sc.LANES)).reshape(-1))   # four in every wave
    print(f"{name}: n = {n}, sides {[S['kind'] for S in c['sides']]}, found {c['found']}, d == -0.0: {c['neg_zeros']}")
    assert set(sc.REQUIRED[name]) <= set(c["names"]), (sc.REQUIRED[name], c["names"])
    for q in c["names"]:   # every family that is there, required or not
        assert (sc.of_family(c, q) & live).sum() >= sc.PER_FAMILY, q
    # owner32 on every row, under errstate: an owner among the plan's sides
    with np.errstate(invalid="ignore", over="ignore"):
        owner = al_np.owner32(c["cloud"], c["add"])
    assert set(np.unique(owner)) <= set(c["add"]["side_element"])
    tw = _twin(c)
    assert np.array_equal(tw["element"], owner)
    for k in range(len(c["sides"])):
        assert ((tw["side"] == k) & s).sum() >= 1 and ((tw["side"] == k) & ~s).sum() >= 100, k
    for gate in (None, sc.CHECK_GATE):
        t = tw if gate is None else _twin(c, gate)
        sc.assert_twin_classes(c, t, gate)
        assert cc.share(t) >= 0.999
        assert (t["cls"][~s] == wn.MAPPED).sum() > (0.5 if gate is None else 0.1) * n
    # what the families are
    ns = c["add"]["n_sides"]
    with np.errstate(all="ignore"):
        assert not np.isfinite(c["cloud"][sc.of_family(c, "not_finite")]).all(axis=1).any()
        assert np.all(np.isnan(tw["e"][sc.of_family(c, "not_finite") & live]))
        for fam_name in ("far_ahead", "far_behind"):
            m = sc.of_family(c, fam_name) & live
            assert np.all(np.abs(tw["e"][m]) <= F(sc.GATE)) and np.all(~(np.abs(tw["jl"][m]) < F(1.0e17)))
            assert not m.any() or ((np.abs(tw["jl"][m]) < F(4.0e18)).sum() >= 2 and (~(np.abs(tw["jl"][m]) < F(4.0e18))).sum() >= 4)
        m = sc.of_family(c, "cy_in_gate") & live
        assert np.all(np.abs(tw["e"][m]) <= F(sc.GATE))
        m = sc.of_family(c, "g_in_gate") & live
        assert np.all(np.abs(tw["e"][m]) <= F(sc.GATE)) and np.all(np.isfinite(tw["jl"][m]))
        kinds = np.array([S["kind"] for S in c["sides"]])[tw["side"]]
        assert np.all(kinds[m] == "clothoid") and np.all(kinds[sc.of_family(c, "cy_in_gate")] == "arc")
        # with every guard off, each of them is mapped or outside: nothing but the guard classes them
        off = _twin(c, fault="no_guard")
        m = (sc.of_family(c, "g_in_gate") | sc.of_family(c, "cy_in_gate")) & live
        assert np.all(np.isin(off["cls"][m], (wn.MAPPED, wn.OUTSIDE)))
        for k, S in enumerate(c["sides"]):   # every end side that is curved owns at least eight
            if S["kind"] != "straight" and k in (0, ns - 1):
                assert (m & (tw["side"] == k)).sum() >= sc.PER_FAMILY, k
        if "plane_nan" in c["names"]:
            m = sc.of_family(c, "plane_nan")
            d = np.array([al_np.joint_d32(c["cloud"][m], c["add"]["joint_o"][j], c["add"]["joint_a"][j]) for j in range(ns - 1)])
            assert np.all(~np.isfinite(d).all(axis=0))
            for j in range(ns - 1):
                assert np.isnan(d[j]).sum() >= 4 and (d[j] == np.inf).sum() >= 2 and (d[j] == -np.inf).sum() >= 2, j
            # a row whose d is NaN at every joint falls to the last side, not to the first
            assert (np.isnan(d).all(axis=0) & (tw["side"][m] == ns - 1)).sum() >= 4
        if "on_joint" in c["names"]:
            m = sc.of_family(c, "on_joint")
            d = np.array([al_np.joint_d32(c["cloud"][m], c["add"]["joint_o"][j], c["add"]["joint_a"][j]) for j in range(ns - 1)])
            at = d == 0.0
            assert np.all(at.sum(axis=0) == 1)
            j = at.argmax(axis=0)
            assert np.all(tw["side"][m] == j + 1)   # the later side
            assert np.all(sc.owner_side(c["cloud"][m], c["add"], "owner_le") != tw["side"][m])


def test_on_joint_exists():
    assert sum("on_joint" in sc.case(name)["names"] for name in sc.PLANS) >= 1


def test_the_single_straight_map_case():
    c = sc.straight_case()
    tw = _twin(c)
    sc.assert_twin_classes(c, tw)
    live = c["labels"] == 0
    for q in c["names"]:
        assert (sc.of_family(c, q) & live).sum() >= sc.PER_FAMILY
    assert (tw["cls"] == wn.MAPPED).sum() > 0.5 * len(c["cloud"])


# which fault each plan can see: the stray families the fault moves
SEES = {
    "owner_le": ("straight_clothoid", "three_sides", "four_sides"),                      # on_joint
    "nan_first": sc.JOINT_PLANS + ("three_sides", "four_sides"),                         # plane_nan
    "no_guard": ("arc_arc", "arc_clothoid", "clothoid_arc", "one_arc",                   # cy_in_gate on arc end sides,
                 "clothoid_straight", "straight_clothoid", "one_clothoid"),              # g_in_gate on clothoid end sides
    "no_4e18": ("straight_clothoid", "three_sides", "four_sides", "one_straight"),       # far_behind, far_ahead
    "nonfinite_outside": sc.PLANS,                                                       # not_finite
}


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_the_assertions_bite(fault):
    """A kernel that is wrong in one line -- the owner rule with d <= 0; a NaN d owned by side 0; a side's guard dropped
    (cy on an arc, the whole `ok` on a clothoid); the 4e18 rule dropped, the conversion saturating and the station clamped into the map; a residual that is not
    finite classed outside -- run as if it were the device against the right twin: the add's, the check's and the align's
    assertions each fail, on every plan whose families the fault can move."""
    for name in SEES[fault]:
        c = sc.case(name)
        right, wrong = _twin(c), _twin(c, fault=fault)
        assert sc.assert_add(c, right, *_device_of(right)) == 0           # the right chain passes its own pins
        with pytest.raises(AssertionError):
            sc.assert_add(c, right, *_device_of(wrong))
        # the check under the map's gate: class 3 stands for any class of a mapped point
        def check_out(tw):
            cls = np.select([tw["cls"] == wn.PLANE, tw["cls"] == wn.BEYOND, tw["cls"] == wn.OUTSIDE], [0, 1, 2], 4).astype(np.uint8)
            ns = len(c["sides"])
            side_class = np.array([[int(((tw["side"] == k) & (cls == q)).sum()) for q in range(7)] for k in range(ns)])
            info = dict(side_class=side_class, n_points=len(cls))
            info.update({q: int(side_class[:, i].sum()) for i, q in
                         enumerate(("plane", "beyond_gate", "outside", "unsurveyed", "unchanged", "changed_pos", "changed_neg"))})
            return dict(element=tw["element"], cls=cls, cell=tw["cell"].astype(np.int32)), info
        sc.assert_check(c, right, *check_out(right))
        with pytest.raises(AssertionError):
            sc.assert_check(c, right, *check_out(wrong))
        # the align over a patch of 36 rows about every side's anchor
        rows = [(18, 36)] * len(c["sides"])

        def align_out(tw):
            cr = sc.class_rows(tw)[:, [3, 2, 1, 0]]
            info = dict(zip(("plane", "beyond_gate", "outside_patch", "binned"), (int(v) for v in cr.sum(axis=0))), side_class=cr)
            return dict(element=tw["element"], e=tw["e"], cell=tw["cell"].astype(np.int32)), info
        ra = sc.joint_twin(c["add"], c["sides"], c["cloud"], c["labels"], rows=rows)
        wr = sc.joint_twin(c["add"], c["sides"], c["cloud"], c["labels"], rows=rows, fault=fault)
        sc.assert_align(c, ra, *align_out(ra))
        with pytest.raises(AssertionError):
            sc.assert_align(c, ra, *align_out(wr))
