"""The wall alignment's device-free rules without a GPU (include/gm_hip.h: a wall alignment): the chaining of the element
maps against the existing gm_wall_arc_frame / gm_wall_clothoid_frame, the round trip of project and point across every
joint, the chainage window, and the fp32 ownership twin of the joint kernel (tests/wall_alignment_np.py) against the fp64
owner within the chain's forward-error bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_np as al_np  # noqa: E402

PRM = dict(n_sectors=90, station_length=al_np.DS, radius=al_np.RADIUS)
VEC = ("point", "direction", "up", "forward")


def _rule(elements=None, **kw):
    return api.WallAlignmentRule(al_np.elements5() if elements is None else elements, **dict(PRM, **kw))


def _end_frame(ep, arc, cl):
    """(o, a, u) at the element's end by the EXISTING rules: gm_wall_arc_frame, gm_wall_clothoid_frame, o + s a."""
    s_end = ep.t_min + float(ep.n_stations) * ep.station_length
    if arc is not None:
        o, a, u, _ = api.wall_arc_frame(ep, arc, s_end)
    elif cl is not None:
        o, a, u, _, _, _ = api.wall_clothoid_frame(ep, cl, s_end)
    else:
        a, u, _ = al_np.design_uv(ep.point[:], ep.direction[:], ep.up[:], ep.forward[:])
        pt = np.array(ep.point[:])
        o = (pt - (pt @ a) * a) + s_end * a
    return o, a, u


@pytest.mark.parametrize("template", [dict(), dict(t_min=5000.0, point=(3.0, -2.0, 1.0), direction=(0.6, 0.8, 0.0), forward=(1.0, 1.0, 0.0),
                                                   up=(0.1, 0.0, 1.0))])
def test_chaining(template):
    els = al_np.elements5()
    A = _rule(**template)
    assert A.check() == _lib.GM_OK
    spans = al_np.spans(els, t_min=template.get("t_min", 0.0))
    prev = None
    for i, e in enumerate(els):
        ep, arc, cl = A.element_params(i)
        assert (arc is not None, cl is not None) == (e["kind"] == "arc", e["kind"] == "clothoid")
        assert ep.n_stations == e["n_stations"] and (ep.n_sectors, ep.station_length, ep.radius) == (90, 0.25, 2.0)
        a, u, v = al_np.design_uv(ep.point[:], ep.direction[:], ep.up[:], ep.forward[:])
        if e["kind"] == "straight":
            # the straight rule's own chainage of `point`; the offset to the alignment's chainage comes back from project
            if i:
                assert ep.t_min == float(np.dot(np.array(ep.point[:]), np.array(ep.direction[:]) / np.sqrt(np.dot(ep.direction[:], ep.direction[:]))))
        else:
            assert ep.t_min == spans[i][0] and (arc or cl).point_chainage == spans[i][0]
            m = -v   # turn = (0, -1), normalised
            got = np.array(arc.curvature[:]) * al_np.ARC_R if arc is not None else np.array(cl.normal[:])
            assert np.abs(got - m).max() <= 1e-15
            if cl is not None:
                assert (cl.curvature, cl.rate) == (e["curvature"], e["rate"])
        if prev is not None:
            o, pa, pu = prev
            # copied: bit for bit
            assert np.array_equal(np.array(ep.point[:]), o) and np.array_equal(np.array(ep.direction[:]), pa)
            assert np.array_equal(np.array(ep.forward[:]), pa) and np.array_equal(np.array(ep.up[:]), pu)
            # the next element's design-frame rule recomputes the carried frame
            assert np.abs(a - pa).max() <= 1e-12 and np.abs(u - pu).max() <= 1e-12
        # the alignment's chainage at the element's start is the span's (1 mm along the tangent: the axis leaves it by
        # kappa^2 s^3 / 3 at the most, 1e-13 m here)
        pt = np.array(ep.point[:])
        start = pt if (i or e["kind"] != "straight") else (pt - (pt @ a) * a) + ep.t_min * a
        el, s, _, _ = A.project(start + 1e-3 * a)
        assert el[0] == i and abs(s[0] - (spans[i][0] + 1e-3)) <= 1e-9
        prev = _end_frame(ep, arc, cl)
    # the sector angle is continuous: v turns with the section too
    P, a, u, v = al_np.axes(A, spans[2][0] + 3.0)
    assert abs(a @ u) <= 1e-12 and abs(np.linalg.norm(u) - 1.0) <= 1e-12 and abs(u[2] - (u @ np.array(A.prm.up[:])) / np.linalg.norm(A.prm.up[:])) <= 0.02


def test_round_trip_across_every_joint():
    """The single-element round trips of tests/test_wall_arc_np.py and tests/test_wall_clothoid_np.py hold 1e-9 (chainage, e,
    rho dphi).  A joint adds no error of its own: the next element starts from the copied end frame, whose re-normalisation
    moves it by rounding alone, so the bound is theirs unchanged."""
    els = al_np.elements5()
    A = _rule()
    total = al_np.spans(els)[-1][1]
    rng = np.random.default_rng(5)
    s = np.sort(np.concatenate([np.linspace(0.013, total - 0.013, 1200)] +
                               [j + rng.uniform(-0.05, 0.05, 60) for _, j in al_np.spans(els)[:-1]]))
    phi = rng.uniform(0.0, 2 * np.pi, len(s))
    rho = al_np.RADIUS + rng.uniform(-0.2, 0.2, len(s))
    x = A.point(s, phi, rho)
    el, s2, phi2, e2 = A.project(x)
    dphi = np.abs(np.mod(phi2 - phi + np.pi, 2 * np.pi) - np.pi)
    worst = (np.abs(s2 - s).max(), np.abs(e2 - (rho - al_np.RADIUS)).max(), (dphi * rho).max())
    print(f"round trip over {len(s)} points: |ds| {worst[0]:.2e} |de| {worst[1]:.2e} rho |dphi| {worst[2]:.2e}")
    assert max(worst) <= 1e-9
    want = np.searchsorted([b for _, b in al_np.spans(els)[:-1]], s, side="right")
    near = np.min(np.abs(s[:, None] - np.array([b for _, b in al_np.spans(els)[:-1]])[None, :]), axis=1) < 1e-9
    assert np.array_equal(el[~near], want[~near]) and np.bincount(el, minlength=5).min() > 100
    # the alignment's axis is continuous in position and direction across the joints
    for _, j in al_np.spans(els)[:-1]:
        P0, a0, u0, _ = al_np.axes(A, j - 1e-7)
        P1, a1, u1, _ = al_np.axes(A, j + 1e-7)
        assert np.abs(P1 - P0).max() <= 3e-7 and np.abs(a1 - a0).max() <= 1e-8 and np.abs(u1 - u0).max() <= 1e-8


def test_window_tiles_an_interval_over_three_elements():
    els = al_np.elements5()
    A = _rule()
    spans = al_np.spans(els)
    s_from, s_to = spans[1][0] - 3.1, spans[3][0] + 2.6      # from inside element 0 over 1 and 2 into 3
    got = A.window(s_from, s_to)
    assert got == al_np.window(els, s_from, s_to)
    assert [g[0] for g in got] == [0, 1, 2, 3]
    lo = hi = None
    for (i, j0, n) in got:
        a, b = spans[i][0] + j0 * 0.25, spans[i][0] + (j0 + n) * 0.25
        assert n > 0 and j0 + n <= els[i]["n_stations"]
        if hi is not None:
            assert a == hi                                   # no gap, no overlap
        lo, hi = (a if lo is None else lo), b
    assert lo <= s_from < lo + 0.25 and hi - 0.25 < s_to <= hi
    three = A.window(spans[1][0] + 0.01, spans[3][1] - 0.01)
    assert three == [(1, 0, 48), (2, 0, 40), (3, 0, 48)]
    assert A.window(-50.0, 1e9) == [(i, 0, e["n_stations"]) for i, e in enumerate(els)]
    assert A.window(spans[2][0], spans[2][0]) == [] and A.window(spans[2][0], spans[2][0] + 1e-9) == [(2, 0, 1)]


TURNS = {
    # one arc of 2.5 rad (143 degrees): a point beyond it lies behind the first joint's plane
    "arc_143_degrees": [dict(kind="straight", n_stations=80), dict(kind="arc", n_stations=800, turn=al_np.LEFT, curvature=1 / 80.0),
                        dict(kind="straight", n_stations=400)],
    # transition, two arcs of 2 rad each (229 degrees in all), transition: the alignment comes back past its own start
    "two_arcs_229_degrees": [dict(kind="straight", n_stations=80),
                             dict(kind="clothoid", n_stations=80, turn=al_np.LEFT, curvature=0.0, rate=1 / (80.0 * 20.0)),
                             dict(kind="arc", n_stations=640, turn=al_np.LEFT, curvature=1 / 80.0),
                             dict(kind="arc", n_stations=640, turn=al_np.LEFT, curvature=1 / 80.0),
                             dict(kind="clothoid", n_stations=80, turn=al_np.LEFT, curvature=1 / 80.0, rate=-1 / (80.0 * 20.0)),
                             dict(kind="straight", n_stations=400)],
}


@pytest.mark.parametrize("name", sorted(TURNS))
def test_owner_on_an_alignment_that_turns_more_than_a_quarter_turn(name):
    """The owner looks at an element's own two joints, so it holds where the alignment has turned past a quarter turn from
    an early joint's normal: project(point) gives the element, the chainage and e back all along, and the plan of an add
    puts the sensor, and the sides, where the sensor is."""
    els = TURNS[name]
    A = _rule(els)
    assert A.check() == _lib.GM_OK
    spans = al_np.spans(els)
    total = spans[-1][1]
    rng = np.random.default_rng(9)
    s = np.sort(rng.uniform(0.01, total - 0.01, 1500))
    phi = rng.uniform(0.0, 2 * np.pi, len(s))
    rho = al_np.RADIUS + rng.uniform(-0.2, 0.2, len(s))
    el, s2, phi2, e2 = A.project(A.point(s, phi, rho))
    ends = np.array([b for _, b in spans[:-1]])
    want = np.searchsorted(ends, s, side="right")
    near = np.min(np.abs(s[:, None] - ends[None, :]), axis=1) < 1e-9
    assert np.array_equal(el[~near], want[~near])
    dphi = np.abs(np.mod(phi2 - phi + np.pi, 2 * np.pi) - np.pi)
    worst = (np.abs(s2 - s).max(), np.abs(e2 - (rho - al_np.RADIUS)).max(), (dphi * rho).max())
    print(f"{name}: round trip over {len(s)} points: |ds| {worst[0]:.2e} |de| {worst[1]:.2e} rho |dphi| {worst[2]:.2e}")
    assert max(worst) <= 1e-9
    assert np.bincount(el, minlength=len(els)).min() > 10
    # the sensor's element and the sides of an add, every 10 m and 1 m either side of every joint
    for sc in list(np.arange(5.0, total, 10.0)) + [j + d for j in ends for d in (-1.0, 1.0)]:
        _, pose = al_np.frame(A, sc, 4, seed=1)
        plan = A.add_plan(pose, 5.0)
        i = int(np.searchsorted(ends, sc, side="right"))
        reach = plan["reach"]
        sides = [k for k, (a, b) in enumerate(spans) if a < sc + reach and b > sc - reach]
        assert plan["element"] == i and abs(plan["chainage"] - sc) <= 1e-9 and plan["side_element"] == sides, (sc, plan)


JOINT_KINDS = {
    "straight_clothoid": (al_np.elements5(80, 80, 80), 0), "clothoid_arc": (al_np.elements5(80, 80, 80), 1),
    "arc_clothoid": (al_np.elements5(80, 80, 80), 2), "clothoid_straight": (al_np.elements5(80, 80, 80), 3),
    "arc_arc": ([dict(kind="arc", n_stations=80, turn=al_np.LEFT, curvature=1 / 80.0),
                 dict(kind="arc", n_stations=80, turn=al_np.LEFT, curvature=1 / 50.0)], 0),
}


@pytest.mark.parametrize("joint", sorted(JOINT_KINDS))
def test_ownership_twin_against_the_fp64_owner(joint):
    """The kernel's fp32 owner (fma32, surf_dot3's order) differs from gm_wall_alignment_project's only where the fp64 |d|
    of a joint lies inside the forward-error bound of the fp32 chain, computed per point; such points are at most 0.1 % of
    a frame (expected: about 1e-6 of the points)."""
    els, j = JOINT_KINDS[joint]
    A = _rule(els)
    sj = al_np.spans(els)[j][1]
    nxt, _, _ = A.element_params(j + 1)
    J = np.array(nxt.point[:])
    aJ, _, _ = al_np.design_uv(nxt.point[:], nxt.direction[:], nxt.up[:], nxt.forward[:])
    for k, s in enumerate((sj - 1.0, sj + 1.0)):
        cloud, pose = al_np.frame(A, s, 4000, seed=70 + k)
        plan = A.add_plan(pose, 5.0)
        assert plan["n_sides"] == 2 and plan["side_element"] == [j, j + 1] and plan["element"] == (j if k == 0 else j + 1)
        assert abs(plan["chainage"] - s) <= 1e-9 and abs(plan["reach"] - (2 * np.sqrt(3) * 5.0 + 0.25)) <= 1e-12
        d64, bound = al_np.joint_d64(cloud, pose, J, aJ)
        # the plane the kernel receives is the fp64 plane rounded once
        Rm, tr = pose[:, :3], pose[:, 3]
        assert np.array_equal(plan["joint_o"][0], (Rm.T @ (J - tr)).astype(np.float32))
        assert np.array_equal(plan["joint_a"][0], (Rm.T @ aJ).astype(np.float32))
        d32 = al_np.joint_d32(cloud, plan["joint_o"][0], plan["joint_a"][0])
        assert np.all(np.abs(d32.astype(np.float64) - d64) <= bound)
        own32 = al_np.owner32(cloud, plan)
        x = cloud.astype(np.float64) @ Rm.T + tr
        own64 = A.project(x)[0]
        inside = np.abs(d64) <= bound
        differ = own32 != own64
        print(f"{joint} frame {k}: {int(differ.sum())} owners differ, {int(inside.sum())} points inside the bound "
              f"(largest bound {bound.max():.2e} m), owned {np.bincount(own32, minlength=len(els))[[j, j + 1]]}")
        assert not np.any(differ & ~inside)
        assert inside.mean() <= 1e-3
        assert min((own32 == j).sum(), (own32 == j + 1).sum()) > 400
