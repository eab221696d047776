"""The arc and clothoid chains of the wall map (arc_residual / arc_sector, clothoid_residual, reached through wall_chain
from the two adds, the two masked adds and the check's predicate) against their fp32 twins, which follow include/gm_hip.h
operation by operation: e bit for bit wherever it does not depend on atan2f, inside the twin's envelope over atan2f's
+-6 ulps elsewhere; class and cell on every point the twin can decide; and the guard classes of the header, which keep a
stray point of a stage call from an integer conversion or a map index.

Every expectation is the twin's, computed from the inputs and the frame the library reports (tests/curved_chain_cases.py
builds the frames and the guard clouds; tests/test_wall_curved_chain_np.py holds them to their conditions on the CPU and
shows that these assertions fail on a subtly wrong chain).  The wave, trip, block and LDS-window edges of the kernels are
pinned in test_gpu_wall_arc.py, test_gpu_wall_clothoid.py and test_gpu_wall_add_edges.py; here one size, 4097 points (a
ragged last wave, a second trip), is enough.  The straight axis has the 4e18 case of wall_station in
test_gpu_wall_add_edges.py::test_both_sides_of_the_lds_window.
"""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curved_chain_cases as cc  # noqa: E402
import wall_add_checked_np as an  # noqa: E402
import wall_arc_np as wa  # noqa: E402

pytestmark = pytest.mark.gpu
COUNTS = ("mapped", "outside", "beyond_gate", "plane")


def _map(ctx, c):
    return ctx.wall_map(**{c["kind"]: c["axis"]}, **c["p"])


def _frame(m, c, pose):
    """The frame the library reports for this map and pose: the twin takes its four vectors, kappa and rate as bits."""
    if c["kind"] == "arc":
        return api.wall_arc_add_frame(m.prm, m.arc_struct(), pose)
    return api.wall_clothoid_add_frame(m.prm, m.clothoid_struct(), pose)


def _counts(info):
    return tuple(int(info[k]) for k in COUNTS)


def _plain_add(ctx, c, r, cloud, pose, labels):
    """One add on a fresh map against the twin r; the counts are those of a map that got the decidable points alone.
    Returns (map, info, res, cell, worst ulps)."""
    m = _map(ctx, c)
    info, res, cell = m.add_points(cloud, pose, labels=labels)
    keep = ~r["uncertain"]
    if keep.all():
        counts = _counts(m.info())
    else:
        with _map(ctx, c) as m2:
            m2.add_points(cloud[keep], pose, labels=None if labels is None else labels[keep], outputs=False)
            counts = _counts(m2.info())
    return m, info, res, cell, cc.assert_chain(c, r, res, cell, counts)


@pytest.mark.parametrize("name", cc.NAMES)
def test_bits_and_launch_sites(gm, name):
    """One ordinary frame through the plain add, the masked add (no row; every third point) and the check (its own gate):
    e against the twin, the same bits at every launch site, class, cell and the four counts on the decidable points."""
    c = cc.case(name)
    cloud, pose, lab = c["cloud"], c["pose"], c["labels"]
    n = len(cloud)
    with gm.GeometricMapping() as ctx:
        m = _map(ctx, c)
        f = _frame(m, c, pose)
        m.close()
        r = cc.twin(c, f, cloud, lab)
        if name.startswith("clothoid"):
            assert bool(r["tangent"]) == ("tangent" in name) == (abs(float(f["kappa"])) < 1e-6)
            assert (float(f["kappa"]) == 0.0) == name.endswith("tangent_zero")
        assert cc.share(r) >= 0.999
        m, info, res, cell, worst = _plain_add(ctx, c, r, cloud, pose, lab)
        assert info["anchor_station"] == f["anchor_station"] and cc.same_bits(info["o"], f["o"]) and cc.same_bits(info["a"], f["a"])
        print(f"{name}: worst device - twin = {worst} ulp of e ({'bits' if cc.exact_e(c, r) else 'envelope'}), "
              f"not uncertain {cc.share(r):.5f}, counts {wa.class_counts(r)}")
        raw = m.read_raw().tobytes()
        # the masked add: without a row it is the plain add; with every third point selected, the add of the rest
        for rows in (np.zeros(0, cc.thirds(n).dtype), cc.thirds(n)):
            _, skipped = an.select(rows, n)
            keep = an.keep(n, skipped)
            assert (~keep).sum() == len(rows)
            with _map(ctx, c) as a:
                ainfo, ares, acell = a.add_points_checked(cloud, pose, rows, labels=lab)
                assert ainfo["skipped"] == len(rows) and np.all(acell[~keep] == -1)
                assert cc.same_bits(ares[keep], res[keep]) and np.array_equal(acell[keep], cell[keep])
                if not len(rows):
                    assert a.read_raw().tobytes() == raw and _counts(a.info()) == _counts(m.info())
                else:
                    with _map(ctx, c) as b:
                        b.add_points(cloud[keep], pose, labels=lab[keep], outputs=False)
                        assert a.read_raw().tobytes() == b.read_raw().tobytes() and _counts(a.info()) == _counts(b.info())
        # the check under its own, narrower gate: the add's bits, the twin's classes and cells under that gate
        rc = cc.twin(c, f, cloud, lab, gate=cc.CHECK_GATE)
        assert cc.share(rc) >= 0.999
        cinfo, _, out = m.check_points(cloud, pose, labels=lab, gate=cc.CHECK_GATE)
        assert cc.same_bits(out["e"], res) and m.read_raw().tobytes() == raw
        cc.assert_check(rc, out, cinfo)
        admitted = (rc["cls"] == wa.MAPPED) & ~rc["uncertain"] & ~r["uncertain"]
        assert admitted.sum() > 1000 and np.array_equal(out["cell"][admitted], cell[admitted])
        m.close()


@pytest.mark.parametrize("name", cc.GUARD_NAMES)
def test_guard_classes(gm, name):
    """A cloud whose guard points (cy <= 0; a Newton denominator <= 0.25; a final |g| above the bound; coordinates of 1e30;
    a phase of 2^20; NaN and infinite coordinates) stand between ordinary ones at wave-interior and wave-edge lanes, some
    labelled.  For the add, the masked add and the check: every guard point has cell -1 and the twin's class, e is NaN or
    not as the twin says and has the twin's bits where it is free of atan2f, the counts add up to n, the map's bytes are
    those of a map that got the ordinary points alone, and a following ordinary add still matches."""
    c = cc.guard_case(name)
    cloud, pose, lab, guard = c["cloud"], c["pose"], c["labels"], c["family"] >= 0
    n = len(cloud)
    with gm.GeometricMapping() as ctx:
        m = _map(ctx, c)
        f = _frame(m, c, pose)
        r = cc.twin(c, f, cloud, lab)
        info, res, cell = m.add_points(cloud, pose, labels=lab)
        worst = cc.assert_guards(c, r, res, cell, _counts(m.info()))
        print(f"{name}: n = {n}, {guard.sum()} guard points, worst device - twin = {worst} ulp of e, counts {wa.class_counts(r)}")
        with _map(ctx, c) as b:
            _, bres, bcell = b.add_points(cloud[~guard], pose, labels=lab[~guard])
            assert m.read_raw().tobytes() == b.read_raw().tobytes()
            assert cc.same_bits(bres, res[~guard]) and np.array_equal(bcell, cell[~guard])
            # a following ordinary add on both
            m.add_points(cloud[~guard], pose, labels=lab[~guard], outputs=False)
            b.add_points(cloud[~guard], pose, labels=lab[~guard], outputs=False)
            assert m.read_raw().tobytes() == b.read_raw().tobytes()
            twice = b.read_raw().tobytes()
        # the masked add, every third point selected
        rows = cc.thirds(n)
        keep = an.keep(n, an.select(rows, n)[1])
        with _map(ctx, c) as a, _map(ctx, c) as b:
            ainfo, ares, acell = a.add_points_checked(cloud, pose, rows, labels=lab)
            assert np.all(acell[guard] == -1) and np.all(acell[~keep] == -1)
            assert cc.same_bits(ares[keep][~np.isnan(res[keep])], res[keep][~np.isnan(res[keep])])
            assert np.array_equal(np.isnan(ares[keep]), np.isnan(res[keep])) and np.array_equal(acell[keep], cell[keep])
            assert ainfo["skipped"] + sum(ainfo[k] for k in COUNTS) == n
            assert _counts(ainfo) == wa.class_counts(r, keep)
            b.add_points(cloud[keep & ~guard], pose, labels=lab[keep & ~guard], outputs=False)
            assert a.read_raw().tobytes() == b.read_raw().tobytes()
        # the check, under the map's gate
        cinfo, _, out = m.check_points(cloud, pose, labels=lab, gate=float(c["p"]["gate"]))
        assert np.array_equal(np.isnan(out["e"]), np.isnan(res)) and cc.same_bits(out["e"][~np.isnan(res)], res[~np.isnan(res)])
        cc.assert_check(r, out, cinfo)
        assert np.all(out["cell"][guard] == -1) and np.all(out["cls"][guard & (lab == 0)] == 1) and np.all(out["cls"][guard & (lab == 1)] == 0)
        assert m.read_raw().tobytes() == twice
        m.close()


@pytest.mark.parametrize("kind", ["arc", "clothoid"])
def test_far_stations_are_outside(gm, kind):
    """wall_station's |jl| < 4e18 on the curved axes: points within the gate 1e18 .. 2e20 stations from the anchor, on
    both sides of the rule and of the anchor, are outside in the add, the masked add and the check, and the map stays
    empty."""
    c = cc.far_station_case(kind)
    cloud, pose = c["cloud"], c["pose"]
    n = len(cloud)
    with gm.GeometricMapping() as ctx:
        m = _map(ctx, c)
        empty = m.read_raw().tobytes()
        r = cc.twin(c, _frame(m, c, pose), cloud, None)
        assert np.all(r["cls"] == wa.OUTSIDE) and not r["uncertain"].any()
        info, res, cell = m.add_points(cloud, pose)
        assert cc.assert_chain(c, r, res, cell, _counts(m.info())) == 0 and _counts(m.info()) == (0, n, 0, 0)
        ainfo, ares, acell = m.add_points_checked(cloud, pose, cc.thirds(n))
        assert cc.same_bits(ares, res) and np.all(acell == -1) and ainfo["outside"] == n - ainfo["skipped"]
        cinfo, _, out = m.check_points(cloud, pose, gate=float(c["p"]["gate"]))
        assert cc.same_bits(out["e"], res) and cinfo["outside"] == n
        cc.assert_check(r, out, cinfo)
        assert m.read_raw().tobytes() == empty
        m.close()
