"""GPU tests of the wall alignment (gm_wall_alignment_*): an alignment add changes every element map exactly as
gm_wall_map_add_points of the sub-cloud that element owns, every point is owned once, and the owner is the fp32 rule of
tests/wall_alignment_np.py.  Frames are 4 000 points on the alignment's own tube (gm_wall_alignment_point) plus
synth.wall_texture, boxFilterBound 5, 90 sectors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_np as al_np  # noqa: E402

pytestmark = pytest.mark.gpu
N = 4000
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
TOTALS = ("mapped", "outside", "beyond_gate", "plane", "cells_hit", "frames")
K80 = 1.0 / 80.0
T = al_np.LEFT


def _prm(**kw):
    return dict(dict(n_sectors=90, station_length=al_np.DS, radius=al_np.RADIUS), **kw)


def _long5(n=80, ds=al_np.DS):
    """straight - clothoid - arc - clothoid - straight with elements longer than the reach (n stations of ds each)."""
    return al_np.elements5(n_straight=n, n_clothoid=n, n_arc=n, ds=ds)


COMPOUND = [dict(kind="arc", n_stations=80, turn=T, curvature=K80), dict(kind="arc", n_stations=80, turn=T, curvature=1.0 / 50.0)]
# (elements, the joint's index): the sensor sits 1 m before and 1 m after it
JOINTS = {
    "straight_clothoid": (_long5(), 0), "clothoid_arc": (_long5(), 1), "arc_clothoid": (_long5(), 2),
    "clothoid_straight": (_long5(), 3), "arc_arc": (COMPOUND, 0),
}


def _standalone(c, al, p):
    """One plain map per element, created from gm_wall_alignment_element_params."""
    out = []
    for i in range(al.n_elements):
        ep, arc, cl = al.element_params(i)
        kw = {k: (list(getattr(ep, k)) if k in ("point", "direction", "up", "forward") else getattr(ep, k))
              for k in ("n_stations", "n_sectors", "station_length", "t_min", "gate", "point", "direction", "radius", "up", "forward")}
        m = c.wall_map(arc=arc, clothoid=cl, **kw)
        assert bytes(m.prm) == bytes(ep)
        out.append(m)
    return out


def _same_maps(al, maps):
    al.sync()
    total = 0
    for i, m in enumerate(maps):
        e = al.element(i)
        assert e.read_raw().tobytes() == m.read_raw().tobytes(), i
        ie, im = e.info(), m.info()
        for k in TOTALS:
            assert ie[k] == im[k], (i, k)
        total += sum(ie[k] for k in ("mapped", "outside", "beyond_gate", "plane"))
    return total


def _parity(c, elements, p, frames, labels=None, sides=None):
    """Every frame through WallAlignment.add_points, and per side the sub-cloud the device's `element` output assigns to it
    through the plain add_points of a standalone map under the same pose: equal per-point outputs, bytes and totals; the
    device's owner is the twin's.  Returns the alignment, the standalone maps and the owners' counts per element."""
    al = c.wall_alignment(elements, **p)
    maps = _standalone(c, al, p)
    owned = np.zeros(al.n_elements, np.int64)
    al.per_frame = []   # (plan, cell, element) of every frame, for the tests that look at where the points went
    n = 0
    for k, (cloud, pose) in enumerate(frames):
        lab = None if labels is None else labels[k]
        plan, res, cell, el = al.add_points(cloud, pose, labels=lab)
        if sides is not None:
            assert plan["n_sides"] == sides, plan
        host = al.add_plan(pose)   # the device-free plan is the add's
        assert sorted(host) == sorted(plan) and all(np.array_equal(plan[q], host[q]) for q in plan)
        assert np.array_equal(el, al_np.owner32(cloud, plan))
        al.per_frame.append((plan, cell, el))
        for i in plan["side_element"]:
            sub = el == i
            _, r, cl = maps[i].add_points(cloud[sub], pose, labels=None if lab is None else lab[sub])
            assert np.array_equal(res[sub].view(np.uint32), r.view(np.uint32)), i
            assert np.array_equal(cell[sub], cl), i
            owned[i] += int(sub.sum())
        assert set(np.unique(el)) <= set(plan["side_element"])
        n += len(cloud)
    assert _same_maps(al, maps) == n
    return al, maps, owned


def test_one_side(gm):
    """A frame more than the reach from any joint is the element map's own add."""
    els = al_np.elements5(n_straight=160, n_clothoid=160, n_arc=160)[:3]
    p = _prm()
    rule = api.WallAlignmentRule(els, **p)
    with gm.GeometricMapping() as c:
        frames = [al_np.frame(rule, s, N, seed=3 + k) for k, s in enumerate((20.0, 60.0, 100.0))]
        lab = [(np.arange(N) % 9 == 0).astype(np.uint8)] * 3
        al, maps, owned = _parity(c, els, p, frames, labels=lab, sides=1)
        assert list(owned) == [N, N, N]
        i = al.info()
        assert i["n_elements"] == 3 and i["n_stations"] == 480 and (i["chainage_min"], i["chainage_max"]) == (0.0, 120.0)
        assert i["frames"] == 3 and i["mapped"] > 0.8 * 3 * N and i["plane"] == 3 * int(lab[0].sum())


@pytest.mark.parametrize("joint", sorted(JOINTS))
def test_joint_parity(gm, joint):
    els, j = JOINTS[joint]
    p = _prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    with gm.GeometricMapping() as c:
        frames = [al_np.frame(rule, sj - 1.0, N, seed=11), al_np.frame(rule, sj + 1.0, N, seed=12)]
        lab = [None, (np.arange(N) % 7 == 0).astype(np.uint8)]
        al, maps, owned = _parity(c, els, p, frames, labels=lab, sides=2)
        print(f"{joint}: owned {list(owned)}")
        assert owned[j] > 0.2 * 2 * N and owned[j + 1] > 0.2 * 2 * N and owned.sum() == 2 * N
        mapped = [al.element(i).info()["mapped"] for i in (j, j + 1)]
        assert min(mapped) > 0.15 * 2 * N and sum(mapped) > 0.8 * 2 * N


def test_three_and_four_sides(gm):
    p = _prm()
    short = [dict(kind="arc", n_stations=8, turn=T, curvature=K80), dict(kind="clothoid", n_stations=8, turn=T, curvature=K80, rate=-K80 / 2.0)]
    ends = [dict(kind="straight", n_stations=80)]
    with gm.GeometricMapping() as c:
        for els, sides in ((ends + short[:1] + ends, 3), (ends + short + ends, 4)):
            rule = api.WallAlignmentRule(els, **p)
            mid = 20.0 + 0.25 * 4 * (sides - 2)
            frames = [al_np.frame(rule, mid - 1.5, N, seed=21), al_np.frame(rule, mid + 1.5, N, seed=22)]
            al, maps, owned = _parity(c, els, p, frames, sides=sides)
            print(f"{sides} sides: owned {list(owned)}")
            assert np.all(owned > 100)
        # six 1 m elements in a row: more sides than a launch takes
        els = ends + [dict(kind="arc", n_stations=4, turn=T, curvature=K80)] * 6 + ends
        al = c.wall_alignment(els, **p)
        cloud, pose = al_np.frame(al, 23.0, N, seed=23)
        before = [al.element(i).read_raw().tobytes() for i in range(al.n_elements)]
        with pytest.raises(_lib.GmError) as ex:
            al.add_points(cloud, pose)
        assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
        with pytest.raises(_lib.GmError) as ex:
            al.add_plan(pose)
        assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
        c.process_frame(cloud)
        with pytest.raises(_lib.GmError) as ex:
            al.add_frame(0, pose)
        assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
        assert [al.element(i).read_raw().tobytes() for i in range(al.n_elements)] == before
        assert al.info()["frames"] == 0


@pytest.mark.parametrize("ds", [1.0, 0.25, 0.05])
def test_window_split_against_global_path(gm, ds, monkeypatch):
    """At ds = 1 the sides' LDS windows hold the reach, at ds = 0.25 most of the reach is beyond them, and at ds = 0.05 the
    whole table is 2.25 m of stations, so most of the POINTS go to the maps directly; the grid's size changes which block
    sees which point.  The bytes do not move."""
    n = int(round(20.0 / ds))
    els = _long5(n, ds)[1:3]   # clothoid -> arc
    p = _prm(station_length=ds)
    rule = api.WallAlignmentRule(els, **p)
    frames = [al_np.frame(rule, 20.0 - 1.0, N, seed=31), al_np.frame(rule, 20.0 + 1.0, N, seed=32)]
    got = []
    for ppb in (None, "512", "1500"):
        if ppb:
            monkeypatch.setenv("GM_WALL_POINTS_PER_BLOCK", ppb)   # read when a map is created
        with gm.GeometricMapping() as c:
            al, maps, owned = _parity(c, els, p, frames, sides=2)
            got.append(b"".join(al.element(i).read_raw().tobytes() for i in range(2)))
            # a side's window lies inside its own add's window, at most 4096 // 90 = 45 stations around its anchor: a mapped
            # point further from the anchor went to the map directly
            direct = 0
            for plan, cell, el in al.per_frame:
                for k, i in enumerate(plan["side_element"]):
                    rel = cell[(el == i) & (cell >= 0)].astype(np.int64) // 90 - plan["side_anchor"][k]
                    direct += int(((rel < -22) | (rel >= 23)).sum())
            print(f"ds={ds} ppb={ppb}: {direct} mapped points surely outside the LDS windows")
            assert direct == 0 if ds >= 0.25 else direct > 2000
    assert len(set(got)) == 1


def test_frame_path_and_ordering(gm):
    els, j = JOINTS["clothoid_arc"]
    p = _prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    frames = [al_np.frame(rule, sj - 1.0, N, seed=41), al_np.frame(rule, sj + 1.0, N, seed=42)]
    kw = dict(neighborRadius=synth.fixed_k_radius(N))
    # process_frame + add_frame with the plane RANSAC against add_points on the valid cloud and its labels
    with gm.GeometricMapping(flags=PLANE, **kw) as c:
        al = c.wall_alignment(els, **p)
        ref = c.wall_alignment(els, **p)
        for cloud, pose in frames:
            c.process_frame(cloud)
            plan = al.add_frame(0, pose)
            assert plan["n_sides"] == 2
            xyz, _ = c.cropped_cloud()
            ref.add_points(xyz, pose, labels=c.labels(), outputs=False)
        _same_maps(al, [ref.element(i) for i in range(al.n_elements)])
        assert al.info()["mapped"] > 0.5 * 2 * N
    # two slots adding joint frames concurrently against the sequential adds; a check enqueued behind an add sees it
    with gm.GeometricMapping(n_slots=2, **kw) as c:
        al = c.wall_alignment(els, **p)
        for k, (cloud, pose) in enumerate(frames):
            c.submit_frame(k, cloud)
            al.add_frame(k, pose)
        e = al.element(j)
        e.check_frame(0, frames[0][1], min_count=1)
        first = e.check_result(0)[0]
        valid = []
        for k in range(2):
            c.wait_frame(k)
            valid.append(c.cropped_cloud(k)[0])
        al.sync()
        e.check_frame(0, frames[0][1], min_count=1)
        again = e.check_result(0)[0]
        assert first["n_points"] == len(valid[0])
        surveyed = first["n_points"] - first["unsurveyed"] - first["outside"] - first["beyond_gate"] - first["plane"]
        print(f"check behind the add: {first}")
        assert surveyed > 0.2 * N                      # the add's own points are in the map the check reads
        assert first["unsurveyed"] >= again["unsurveyed"]   # (slot 1's add may have landed in between)
        seq = c.wall_alignment(els, **p)
        for xyz, (_, pose) in zip(valid, frames):
            seq.add_points(xyz, pose, outputs=False)
        _same_maps(al, [seq.element(i) for i in range(al.n_elements)])


def test_straight_map_beside_an_alignment(gm):
    drive = synth.tunnel_drive(2, N, seed=5)
    p = dict(n_stations=176, **drive["design"])
    with gm.GeometricMapping() as c:
        alone = c.wall_map(**p)
        for cloud, pose in drive["frames"]:
            alone.add_points(cloud, pose, outputs=False)
        ref, info = alone.read_raw().tobytes(), alone.info()
    els, j = JOINTS["straight_clothoid"]
    rule = api.WallAlignmentRule(els, **_prm())
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **_prm())
        m = c.wall_map(**p)
        jf = al_np.frame(rule, 19.0, N, seed=51)
        for cloud, pose in drive["frames"]:
            al.add_points(*jf, outputs=False)
            m.add_points(cloud, pose, outputs=False)
        assert m.read_raw().tobytes() == ref
        im = m.info()
        for k in TOTALS:
            assert im[k] == info[k], k
        al.close()
        assert m.read_raw().tobytes() == ref


def test_refusals(gm):
    els, _ = JOINTS["straight_clothoid"]
    p = _prm()
    I = _lib.GM_ERR_INVALID_ARG
    with gm.GeometricMapping() as c, gm.GeometricMapping() as other:
        al = c.wall_alignment(els, **p)
        cloud, pose = al_np.frame(al, 19.0, 100, seed=1)
        L = c._L
        dp = pose.ctypes.data_as(C.POINTER(C.c_double))
        assert L.gm_wall_alignment_add_frame(al._al, c._ctx, 0, dp, None) == _lib.GM_ERR_NOT_READY   # no frame in the slot
        assert L.gm_wall_alignment_add_frame(al._al, other._ctx, 0, dp, None) == I                   # a foreign context
        assert L.gm_wall_alignment_add_frame(al._al, c._ctx, 7, dp, None) == I                       # no such slot
        assert L.gm_wall_alignment_add_frame(None, c._ctx, 0, dp, None) == I
        bad = pose.copy()
        bad[0, 0] = np.nan
        with pytest.raises(_lib.GmError) as ex:
            al.add_points(cloud, bad)
        assert ex.value.status == I
        h = C.c_void_p()
        assert L.gm_wall_alignment_map(al._al, 5, C.byref(h)) == I
        with pytest.raises(_lib.GmError) as ex:
            c.wall_alignment([dict(kind="arc", n_stations=8, turn=(0.0, 0.0), curvature=K80)], **p)
        assert ex.value.status == I
        assert al.info()["frames"] == 0
