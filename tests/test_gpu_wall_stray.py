"""Stray points of a stage call on the kernels over a wall alignment's plan and on the single map's locate and align: the
promise of include/gm_hip.h -- a residual that is not finite is beyond_gate (locate: gated), a curved chain's guards class the
point before any integer conversion, a station with |jl| >= 4e18 is outside (align: outside_patch) -- where each kernel
keeps it with a line of its own: the owner rule on a NaN, infinite or exactly zero d (k_wall_add_joint's written-out loop,
joint_owner, joint_owner<false>), the guarded chain ahead of the sides' LDS windows and tables (the joint add, its masked
form, the joint check), the locates' own tests ahead of their table read, and the aligns' range rules.

Every expectation is the twin's (tests/wall_stray_cases.py: the owner by wall_alignment_np.owner32, then the owner's chain
by the chains' fp32 twins on the frame the element's own add reports) or the standalone element map's on the sub-cloud its
side owns, which tests/test_gpu_wall_curved_chain.py pins against the twin.  tests/test_wall_stray_np.py holds the clouds
to their conditions on the CPU and shows that these assertions fail on five kernels that are wrong in one line.

The locate in DESIGN mode consults no station (the header's `target` row), so a point within the gate is used however far
along the axis it lies: far_ahead, far_behind and the `big` rows that the twin leaves finite and inside the gate are given
to the MAP runs, where they are outside, and left out of the DESIGN runs.
"""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curved_chain_cases as cc  # noqa: E402
import test_gpu_wall_alignment as ta  # noqa: E402
import test_gpu_wall_alignment_check as tck  # noqa: E402
import wall_add_checked_np as an  # noqa: E402
import wall_alignment_align_cases as ac  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_stray_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
COUNTS = ("mapped", "outside", "beyond_gate", "plane")
MULTI = sc.JOINT_PLANS + ("three_sides", "four_sides")
ALIGN_PLANS = ("one_straight", "one_arc", "one_clothoid") + sc.JOINT_PLANS + ("four_sides",)
AP = dict(ac.AP, gate=sc.GATE)
SIZES = (0, 1, 63, 64, 65, 1025, 2049, 4097)


def _owner(cloud, plan):
    with np.errstate(invalid="ignore", over="ignore"):
        return al_np.owner32(cloud, plan)


def _raw(al):
    al.sync()
    return [al.element(i).read_raw().tobytes() for i in range(al.n_elements)]


def _totals(al, add):
    al.sync()
    return np.array([[int(al.element(i).info()[q]) for q in COUNTS] for i in add["side_element"]], np.int64)


def _same_plan(plan, add):
    assert sorted(plan) == sorted(add) and all(np.array_equal(plan[q], add[q]) for q in plan), (plan, add)


def _twin(c, gate=None, rows=None):
    return sc.joint_twin(c["add"], c["sides"], c["cloud"], c["labels"], gate, rows)


def _add(ctx, c):
    """The case's cloud through a fresh alignment and, per side, the sub-cloud it owns through a standalone element map:
    (alignment, standalone maps, res, cell, element)."""
    cloud, pose, lab = c["cloud"], c["pose"], c["labels"]
    al = ctx.wall_alignment(c["els"], **lc.prm())
    maps = ta._standalone(ctx, al, lc.prm())
    plan, res, cell, el = al.add_points(cloud, pose, labels=lab)
    _same_plan(plan, c["add"])
    for i in plan["side_element"]:
        sub = el == i
        info, r, cl = maps[i].add_points(cloud[sub], pose, labels=lab[sub])
        assert cc.same_bits(res[sub], r) and np.array_equal(cell[sub], cl), i
        f = c["sides"][plan["side_element"].index(i)]["f"]     # the twin's frame is the one the element's own add reports
        assert info["anchor_station"] == f["anchor_station"] and all(np.array_equal(info[q], f[q]) for q in "oa")
    assert ta._same_maps(al, maps) == len(cloud)
    return al, maps, res, cell, el


@pytest.mark.parametrize("name", sc.PLANS)
def test_joint_add(gm, name):
    """k_wall_add_joint (one side: the element map's own add): the owner on every row, per side the standalone map's bits
    and cells, the twin's e, classes and cells, cell -1 on every stray row, totals that add up to n, the bytes of an
    alignment that got the ordinary points alone, and a following ordinary add on both."""
    c = sc.case(name)
    cloud, pose, lab, s = c["cloud"], c["pose"], c["labels"], sc.stray(c)
    tw = _twin(c)
    keep = ~tw["uncertain"]
    with gm.GeometricMapping() as ctx:
        assert float(ctx.cfg.boxFilterBound) == sc.BOUND
        al, maps, res, cell, el = _add(ctx, c)
        if keep.all():
            totals = _totals(al, c["add"])
        else:
            with ctx.wall_alignment(c["els"], **lc.prm()) as d:
                d.add_points(cloud[keep], pose, labels=lab[keep], outputs=False)
                totals = _totals(d, c["add"])
        worst = sc.assert_add(c, tw, el, res, cell, totals)
        print(f"{name}: n = {len(cloud)}, {s.sum()} stray rows, worst device - twin = {worst} ulp of e, uncertain {int((~keep).sum())}, "
              f"totals {totals.tolist()}")
        with ctx.wall_alignment(c["els"], **lc.prm()) as b:
            _, bres, bcell, bel = b.add_points(cloud[~s], pose, labels=lab[~s])
            assert _raw(al) == _raw(b)
            assert cc.same_bits(bres, res[~s]) and np.array_equal(bcell, cell[~s]) and np.array_equal(bel, el[~s])
            al.add_points(cloud[~s], pose, labels=lab[~s], outputs=False)
            b.add_points(cloud[~s], pose, labels=lab[~s], outputs=False)
            assert _raw(al) == _raw(b)


@pytest.mark.parametrize("name", sc.PLANS)
def test_masked_joint_add(gm, name):
    """k_wall_add_joint_masked with every third row selected: skipped and the four classes add up to n and are the twin's
    over the kept rows, the kept rows have the plain add's bits and cells, the skipped rows no cell, and the bytes are those
    of the add of the kept ordinary points."""
    c = sc.case(name)
    cloud, pose, lab, s = c["cloud"], c["pose"], c["labels"], sc.stray(c)
    n = len(cloud)
    rows = cc.thirds(n)
    keep = an.keep(n, an.select(rows, n)[1])
    assert (~keep).sum() == len(rows) and (s & keep).sum() > 16 and (s & ~keep).sum() > 8
    tw = _twin(c)
    with gm.GeometricMapping() as ctx:
        with ctx.wall_alignment(c["els"], **lc.prm()) as al:
            _, res, cell, el = al.add_points(cloud, pose, labels=lab)
        with ctx.wall_alignment(c["els"], **lc.prm()) as a, ctx.wall_alignment(c["els"], **lc.prm()) as b:
            info, ares, acell, ael = a.add_points_checked(cloud, pose, rows, labels=lab)
            _same_plan(info["plan"], c["add"])
            assert info["skipped"] == len(rows) and info["skipped"] + sum(info[q] for q in COUNTS) == n
            assert np.array_equal(ael, el) and np.array_equal(ael, _owner(cloud, c["add"]))
            assert cc.same_bits(ares[keep], res[keep]) and np.array_equal(acell[keep], cell[keep])
            assert np.all(acell[~keep] == -1) and np.all(acell[s] == -1)
            if not tw["uncertain"].any():
                assert [info[q] for q in COUNTS] == [int(v) for v in sc.class_rows(tw, keep).sum(axis=0)]
                assert np.array_equal(_totals(a, c["add"]), sc.class_rows(tw, keep))
            b.add_points(cloud[keep & ~s], pose, labels=lab[keep & ~s], outputs=False)
            assert _raw(a) == _raw(b)


@pytest.mark.parametrize("name", sc.PLANS)
def test_joint_check(gm, name):
    """The joint check's predicate against the maps the case's own add left, under the map's gate and a narrower one: the
    add's e bits, per point the twin's class and cell on the owner's chain, side_class rows that sum to the summed classes
    and to n, stray rows without a cell and plane, beyond_gate or (far_ahead, far_behind) outside, and untouched maps."""
    c = sc.case(name)
    cloud, pose, lab = c["cloud"], c["pose"], c["labels"]
    with gm.GeometricMapping() as ctx:
        al, maps, res, cell, el = _add(ctx, c)
        before = _raw(al), _totals(al, c["add"]).tolist()
        for gate in (sc.GATE, sc.CHECK_GATE):
            tw = _twin(c, gate)
            info, rows = tck._check_parity(al, maps, cloud, pose, lab, sides=c["add"]["n_sides"], gate=gate, min_count=1)
            _, _, out = al.check_points(cloud, pose, labels=lab, gate=gate, min_count=1)
            assert cc.same_bits(out["e"], res)
            sc.assert_check(c, tw, out, info, gate)
            live = (tw["cls"] == wn.MAPPED) & ~tw["uncertain"]
            assert np.array_equal(out["cell"][live], cell[live])      # what the narrower gate still admits has the add's cell
            print(f"{name} gate {gate}: {[info[q] for q in ('plane', 'beyond_gate', 'outside', 'unsurveyed', 'unchanged')]}")
        assert (_raw(al), _totals(al, c["add"]).tolist()) == before


def _relabelled(c, take):
    """(cloud, labels, labels with the live stray rows relabelled plane, the live stray rows) over the rows of `take`."""
    cloud, lab, s = c["cloud"][take], c["labels"][take], sc.stray(c)[take]
    live = s & (lab == 0)
    lab2 = lab.copy()
    lab2[live] = 1
    return np.ascontiguousarray(cloud), lab, lab2, live


def _design_rows(c):
    """The rows a DESIGN locate gets: all but the stray rows the header's rule would use, which are finite and inside the
    gate 1e17 stations and more along the axis (far_ahead, far_behind, and `big` rows along an a' that is an axis vector)."""
    tw = _twin(c)
    with np.errstate(invalid="ignore"):
        return ~(sc.stray(c) & (tw["cls"] == wn.OUTSIDE))


LOCATE_CLASSES = ("outside", "unsurveyed", "gated")


def _assert_relabelling(got, ref, live, res, first, n_sides=None):
    """A locate of a cloud with stray rows against the same call with those rows relabelled plane.  Per pass: plane is smaller
    by exactly their number and gated + outside + unsurveyed larger by it (in MAP mode the header asks for the station and the
    cell of a finite, guarded e before the gate), used is equal, and rms, step, the blocks, the status and the located pose
    are bit for bit the same: a stray row adds nothing to the sums.  In pass 0, which runs under the caller's pose, outside,
    unsurveyed and gated are each larger by what `first` holds: the twin's count of the live stray rows in that class.
    res is NaN on every stray row."""
    k = int(live.sum())
    assert k > 30 and got["status"] == ref["status"] == _lib.GM_LOCATE_OK and got["passes"] == ref["passes"] == 3
    d0 = [got["pass"][0][q] - ref["pass"][0][q] for q in LOCATE_CLASSES]
    assert sum(first) == k and tuple(d0) == tuple(first), (d0, first)
    for p, q in zip(got["pass"], ref["pass"]):
        assert sum(p[f] - q[f] for f in LOCATE_CLASSES) == k and all(p[f] >= q[f] for f in LOCATE_CLASSES)
        assert p["plane"] + k == q["plane"] and p["used"] == q["used"] > 500
        assert np.float64(p["rms"]).tobytes() == np.float64(q["rms"]).tobytes() and p["step"].tobytes() == q["step"].tobytes()
        for f in ("o", "a", "u", "v", "gate") + (("side", "joint_o", "joint_a") if n_sides else ()):
            assert np.asarray(p[f]).tobytes() == np.asarray(q[f]).tobytes(), f
    for f in ("pose", "lateral", "tilt"):
        assert got[f].tobytes() == ref[f].tobytes(), f
    assert np.all(np.isnan(res[live]))


@pytest.mark.parametrize("ref", (aln.DESIGN, aln.MAP))
@pytest.mark.parametrize("name", MULTI)
def test_alignment_locate(gm, name, ref):
    """k_wall_locate_joint on two, three and four sides, DESIGN and MAP (against a survey of the same wall)."""
    c = sc.case(name)
    take = _design_rows(c) if ref == aln.DESIGN else np.ones(len(c["cloud"]), bool)
    cloud, lab, lab2, live = _relabelled(c, take)
    pose = c["pose"]
    with gm.GeometricMapping() as ctx:
        al = ctx.wall_alignment(c["els"], **lc.prm())
        if ref == aln.MAP:
            for d in (-1.5, 0.0, 1.5):
                al.add_points(*al_np.frame(c["rule"], c["s"] + d, lc.N, seed=61 + sc.PLANS.index(name)), outputs=False)
        before = _raw(al)
        kw = dict(reference=ref, min_count=1)
        got, res, cell, el = al.locate_points(cloud, pose, labels=lab, **kw)
        want, res2, cell2, el2 = al.locate_points(cloud, pose, labels=lab2, **kw)
        # pass 0 in the twin (wall_alignment_locate_np.one_pass on the blocks the record reports): the stray rows' classes
        rec = got["pass"][0]
        raws = [al.element(i).read_raw() for i in got["side_element"]] if ref == aln.MAP else None
        nst = [al.element_params(i)[0].n_stations for i in got["side_element"]]
        t = aln.one_pass(cloud, lab, {q: np.asarray(rec[q], np.float64) for q in ("o", "a", "u", "v")}, al.locate_plan(pose)["s0"],
                         dict(side=rec["side"], joint_o=rec["joint_o"], joint_a=rec["joint_a"]), rec["gate"], got, lc.prm(), nst, raws, 1)
        first = tuple(int((live & (t["cls"] == q)).sum()) for q in (1, 2, 3))     # outside, unsurveyed, gated
        assert not (live & (t["cls"] == 4)).any()
        _assert_relabelling(got, want, live, res, first, c["add"]["n_sides"])
        assert np.array_equal(cell[~live], cell2[~live]) and cc.same_bits(res[~live], res2[~live])
        assert ref == aln.MAP or np.all(cell == -1)
        owner = _owner(cloud, dict(n_sides=got["n_sides"], side_element=got["side_element"], joint_o=got["pass"][0]["joint_o"],
                                   joint_a=got["pass"][0]["joint_a"]))
        assert np.array_equal(el, owner) and np.array_equal(el2, owner)
        # (the locate's planes are images under its state: they are the add's to 1e-17, which an infinite coordinate, a 1e30
        # one and a point exactly on the add's plane tell apart, and nothing else does)
        assert np.array_equal(owner[~sc.stray(c)[take]], _owner(cloud, c["add"])[~sc.stray(c)[take]])
        if ref == aln.MAP:     # the add's far rows are outside here too, not gated, but for those whose e the locate's own
            far = live & (_twin(c)["cls"][take] == wn.OUTSIDE)     # blocks (images under the state, the add's to 1e-17) leave infinite
            assert np.all(np.isin(t["cls"][far], (1, 3))) and ((t["cls"][far] == 1).sum() >= sc.PER_FAMILY or "far_behind" not in c["names"])
        else:
            assert first[:2] == (0, 0) and all(p["outside"] == p["unsurveyed"] == 0 for p in got["pass"])
        print(f"{name} ref={ref}: {int(live.sum())} live stray rows, gated {[p['gated'] for p in got['pass']]}, "
              f"outside {[p['outside'] for p in got['pass']]}, used {[p['used'] for p in got['pass']]}")
        assert _raw(al) == before


@pytest.mark.parametrize("ref", (aln.DESIGN, aln.MAP))
def test_straight_map_locate(gm, ref):
    """k_wall_locate (gm_wall_map_locate_points on a straight map) with not_finite, big, far_ahead and far_behind."""
    c = sc.straight_case()
    take = _design_rows(c) if ref == aln.DESIGN else np.ones(len(c["cloud"]), bool)
    cloud, lab, lab2, live = _relabelled(c, take)
    s = sc.stray(c)
    with gm.GeometricMapping() as ctx:
        m = ctx.wall_map(**c["p"])
        m.add_points(c["cloud"][~s], c["pose"], outputs=False)
        before = m.read_raw().tobytes()
        kw = dict(reference=ref, min_count=1)
        got, res, cell = m.locate_points(cloud, c["pose"], labels=lab, **kw)
        want, res2, cell2 = m.locate_points(cloud, c["pose"], labels=lab2, **kw)
        # a stray row of this cloud whose e is finite lies 1e17 stations and more along the axis: outside in MAP mode
        with np.errstate(invalid="ignore"):
            far = live & np.isfinite(_twin(c)["e"][take])
        first = (int(far.sum()), 0, int((live & ~far).sum())) if ref == aln.MAP else (0, 0, int(live.sum()))
        assert ref == aln.DESIGN or far.sum() >= 4 * sc.PER_FAMILY
        _assert_relabelling(got, want, live, res, first)
        assert np.array_equal(cell[~live], cell2[~live]) and np.all(cell[live] == -1) and cc.same_bits(res[~live], res2[~live])
        assert m.read_raw().tobytes() == before
        m.close()


_INFO_KEYS = ("status", "patch_cells_usable", "anchor_station", "half_patch_stations", "max_station_shift", "max_sector_shift", "overlap",
              "best_station", "best_sector", "frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction")


def _assert_removal(info, tab, info2, tab2):
    """An align against the same call on the cloud with the stray rows removed: the score table, the usable patch cells,
    the overlap, the status, the shift, the roll and the pose byte for byte (integer atomics only: removal is exact)."""
    assert tab.tobytes() == tab2.tobytes()
    for q in _INFO_KEYS:
        assert np.float64(info[q]).tobytes() == np.float64(info2[q]).tobytes(), (q, info[q], info2[q])
    assert info["pose"].tobytes() == info2["pose"].tobytes() and info["binned"] == info2["binned"]


@pytest.mark.parametrize("name", ALIGN_PLANS)
def test_alignment_align(gm, name):
    """k_wall_align_bin_joint (one straight side: k_wall_align_bin through the element map) against a survey of the same
    wall: cell -1 on every stray row, e NaN or not and the four classes per side as the twin says over the patch rows, and
    everything else that of the cloud with the stray rows removed."""
    c = sc.case(name)
    cloud, pose, lab, s = c["cloud"], c["pose"], c["labels"], sc.stray(c)
    with gm.GeometricMapping() as ctx:
        al = ctx.wall_alignment(c["els"], **lc.prm())
        for d in (-1.5, 0.0, 1.5):
            al.add_points(*al_np.frame(c["rule"], c["s"] + d, lc.N, seed=61 + sc.PLANS.index(name)), outputs=False)
        before = _raw(al)
        info, tab, out = al.align_points(cloud, pose, labels=lab, **AP)
        info2, tab2, out2 = al.align_points(cloud[~s], pose, labels=lab[~s], **AP)
        plan = info["align_plan"]
        _same_plan(plan["add"], c["add"])
        P = AP["half_patch_stations"]
        tw = _twin(c, AP["gate"], rows=[(int(r), 2 * P) for r in plan["row0"]])
        sc.assert_align(c, tw, out, info)
        _assert_removal(info, tab, info2, tab2)
        assert np.array_equal(out["cell"][~s], out2["cell"]) and cc.same_bits(out["e"][~s], out2["e"])
        assert info["n_points"] == len(cloud) and info["binned"] > 0.5 * (~s).sum() and int(tab["n"].max()) > 0
        print(f"{name}: {[info[q] for q in ('plane', 'beyond_gate', 'outside_patch', 'binned')]} per side {info['side_class'].tolist()}, "
              f"own {plan['own']}, best {info['best_station']}, {info['best_sector']}")
        assert _raw(al) == before


def test_straight_map_align(gm):
    """k_wall_align_bin on a straight map (gm_wall_map_align_points) with not_finite, big, far_ahead and far_behind."""
    c = sc.straight_case()
    cloud, pose, lab, s = c["cloud"], c["pose"], c["labels"], sc.stray(c)
    with gm.GeometricMapping() as ctx:
        m = ctx.wall_map(**c["p"])
        m.add_points(cloud[~s], pose, outputs=False)
        before = m.read_raw().tobytes()
        info, tab, res, cell = m.align_points(cloud, pose, labels=lab, **AP)
        info2, tab2, res2, cell2 = m.align_points(cloud[~s], pose, labels=lab[~s], **AP)
        P = AP["half_patch_stations"]
        tw = _twin(c, AP["gate"], rows=[(P, 2 * P)])
        sc.assert_align(c, tw, dict(e=res, cell=cell), info)
        _assert_removal(info, tab, info2, tab2)
        assert np.array_equal(cell[~s], cell2) and cc.same_bits(res[~s], res2)
        far = sc.of_family(c, "far_ahead") | sc.of_family(c, "far_behind")
        assert info["outside_patch"] >= int((far & (lab == 0)).sum()) >= 2 * sc.PER_FAMILY and info["binned"] > 0.5 * (~s).sum()
        assert m.read_raw().tobytes() == before
        m.close()


def _size_cloud(rule, s, n_max=4097):
    """Points taken cyclically from one 4000-point joint frame, two stray rows of not_finite / big in every 64 (lanes 5 and
    41), every eleventh point labelled plane: (cloud, pose, labels, stray)."""
    base, pose = al_np.frame(rule, s, lc.N, seed=83)
    big, odd = cc._specials()
    i = np.arange(n_max)
    cloud = base[i % lc.N].copy()
    cloud[i % 64 == 5] = odd[(i[i % 64 == 5] // 64) % len(odd)]
    cloud[i % 64 == 41] = big[(i[i % 64 == 41] // 64) % len(big)]
    return np.ascontiguousarray(cloud), pose, cc.labels_of(n_max), (i % 64 == 5) | (i % 64 == 41)


@pytest.mark.parametrize("name", ("clothoid_arc", "four_sides"))
def test_joint_add_sizes(gm, name, monkeypatch):
    """The ragged last wave, the slot wholly past n and the second trip of a 4096-point block under the owner loop and the
    per-(side, class) ballot rows of k_wall_add_joint and k_wall_add_joint_masked: sub-cloud parity with standalone maps at
    every n; at n = 0 `frames` advances once per side, every total is 0 and the maps keep their bytes."""
    els, s, sides = sc.plan_of(name)
    p = lc.prm()
    cloud, pose, lab, stray = _size_cloud(sc.rule_of(name), s)
    monkeypatch.setenv("GM_WALL_POINTS_PER_BLOCK", "4096")   # read when a map is created
    with gm.GeometricMapping() as ctx:
        for n in SIZES:
            x, l = cloud[:n], lab[:n]
            al, maps, owned = ta._parity(ctx, els, p, [(x, pose)], labels=[l], sides=sides)
            _, cell, el = al.per_frame[0]
            assert np.all(cell[stray[:n]] == -1) and owned.sum() == n
            assert al.info()["frames"] == sides and sum(al.info()[q] for q in COUNTS) == n
            if n == 0:
                empty = ctx.wall_alignment(els, **p)
                assert _raw(al) == _raw(empty)
                empty.close()
            # the masked add, every third row selected: the kept rows through standalone maps per side
            rows = cc.thirds(n)
            keep = an.keep(n, an.select(rows, n)[1]) if n else np.zeros(0, bool)
            a = ctx.wall_alignment(els, **p)
            kept = ta._standalone(ctx, a, p)
            info, ares, acell, ael = a.add_points_checked(x, pose, rows, labels=l)
            assert info["skipped"] == len(rows) and info["skipped"] + sum(info[q] for q in COUNTS) == n
            assert np.array_equal(ael, el) and np.all(acell[~keep] == -1)
            for i in info["plan"]["side_element"]:
                sub = (ael == i) & keep
                _, r, cl = kept[i].add_points(x[sub], pose, labels=l[sub])
                assert cc.same_bits(ares[sub], r) and np.array_equal(acell[sub], cl), (n, i)
            assert ta._same_maps(a, kept) == int(keep.sum())
            assert a.info()["frames"] == sides
            for m in maps + kept:
                m.close()
            al.close()
            a.close()
