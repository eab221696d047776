"""The check and the checked add through a wall alignment (gm_wall_alignment_check_*, gm_wall_alignment_add_*_checked)
against standalone element maps: a standalone map created from gm_wall_alignment_element_params and fed the sub-clouds its
element owns holds the element map's bytes, and its own check_points / add_points of the owned sub-cloud is the reference,
bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_add_checked_np as acn  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_check_np as wc  # noqa: E402

pytestmark = pytest.mark.gpu
N = lc.N
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
TOTALS = ("mapped", "outside", "beyond_gate", "plane", "cells_hit", "frames")
FLOATS = ("x", "y", "z", "delta", "e")
CASES = tuple(f"{k}:{w}" for k in sorted(lc.JOINTS) for w in ("before", "after")) + ("three_sides", "four_sides", "arc")


def _standalone(c, al):
    """One plain map per element, created from gm_wall_alignment_element_params."""
    out = []
    for i in range(al.n_elements):
        ep, arc, cl = al.element_params(i)
        kw = {k: (list(getattr(ep, k)) if k in ("point", "direction", "up", "forward") else getattr(ep, k))
              for k in ("n_stations", "n_sectors", "station_length", "t_min", "gate", "point", "direction", "radius", "up", "forward")}
        out.append(c.wall_map(arc=arc, clothoid=cl, **kw))
    return out


def _same_maps(al, maps):
    al.sync()
    for i, m in enumerate(maps):
        e = al.element(i)
        assert e.read_raw().tobytes() == m.read_raw().tobytes(), i
        ie, im = e.info(), m.info()
        for k in TOTALS:
            assert ie[k] == im[k], (i, k)


def _surveyed(c, els, p, s, seed, offsets=(-0.5, 0.0, 0.5)):
    """An alignment that holds a survey of the wall `seed` around chainage s, added through the alignment, and standalone
    maps that hold the same bytes and totals: each was fed the sub-clouds its element owned."""
    al = c.wall_alignment(els, **p)
    maps = _standalone(c, al)
    for d in offsets:
        cloud, pose = al_np.frame(al, s + d, N, seed=seed)
        plan, _, _, el = al.add_points(cloud, pose)
        for i in plan["side_element"]:
            maps[i].add_points(cloud[el == i], pose, outputs=False)
    return al, maps


def _changed_frame(al, s, seed, n=N, every=16):
    """The wall `seed` seen from s with two blocks of points displaced radially (about the sensor's x axis, which runs
    along the tunnel) by +0.3 m and -0.3 m, and every 23rd point labelled plane: (cloud, pose, labels)."""
    cloud, pose = al_np.frame(al, s, n, seed=seed)
    r = np.maximum(np.linalg.norm(cloud[:, 1:], axis=1, keepdims=True), 1e-3)
    k = np.arange(n)
    scale = np.where((k % every == 3)[:, None], (r + 0.3) / r, np.where((k % every == 11)[:, None], (r - 0.3) / r, 1.0))
    cloud = cloud.copy()
    cloud[:, 1:] = (cloud[:, 1:] * scale).astype(np.float32)
    return cloud, pose, (k % 23 == 0).astype(np.uint8)


def _check_parity(al, maps, cloud, pose, lab, sides=None, **kw):
    """al.check_points against check_points of the standalone maps on the owned sub-clouds.  Returns (info, rows)."""
    n = len(cloud)
    info, rows, out = al.check_points(cloud, pose, labels=lab, **kw)
    plan = info["plan"]
    host = al.add_plan(pose)   # the check's plan is the add's
    assert all(np.array_equal(plan[q], host[q]) for q in plan)
    if sides is not None:
        assert plan["n_sides"] == sides
    assert info["n_sides"] == plan["n_sides"] and info["n_points"] == n and info["threshold_q"] == wc.threshold_q(kw.get("threshold", 0.05))
    el = out["element"]
    assert np.array_equal(el, al_np.owner32(cloud, plan))
    assert int(info["side_class"].sum()) == n
    assert [info[q] for q in wc.NAMES] == [int(v) for v in info["side_class"].sum(axis=0)]
    assert np.all(np.diff(rows["index"].astype(np.int64)) > 0) and np.array_equal(rows["row"], rows["index"])
    side, cell = al.split_cell(rows)
    peak_pos = peak_neg = 0
    for k, i in enumerate(plan["side_element"]):
        sub = np.flatnonzero(el == i)
        ri, rr, ro = maps[i].check_points(cloud[sub], pose, labels=None if lab is None else lab[sub], **kw)
        mine = rows[side == k]
        assert len(mine) == len(rr), (i, len(mine), len(rr))
        for q in FLOATS:
            assert np.array_equal(mine[q].view(np.uint32), rr[q].view(np.uint32)), (i, q)
        assert np.array_equal(mine["index"], sub[rr["index"]]) and np.array_equal(mine["row"], sub[rr["row"]]), i
        assert np.array_equal(cell[side == k], rr["cell"]), i
        assert [int(v) for v in info["side_class"][k]] == [ri[q] for q in wc.NAMES], i
        assert np.array_equal(out["e"][sub].view(np.uint32), ro["e"].view(np.uint32)), i
        for q in ("cell", "delta", "cls"):
            assert np.array_equal(out[q][sub], ro[q]), (i, q)
        peak_pos, peak_neg = max(peak_pos, ri["peak_pos"]), min(peak_neg, ri["peak_neg"])
        if plan["n_sides"] == 1:   # the element map's own check: the rows and the shared fields byte for byte
            assert rows.tobytes() == rr.tobytes() and all(info[q] == ri[q] for q in ri if q != "add")
    assert (info["peak_pos"], info["peak_neg"]) == (peak_pos, peak_neg)
    return info, rows


@pytest.mark.parametrize("case", CASES)
def test_parity(gm, case):
    """Every joint (1 m before and after), three and four sides, one side; MEAN and ENVELOPE.  The displaced blocks put
    both changed classes on both sides of a joint."""
    els, s, sides = lc.record_case(case)
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al, maps = _surveyed(c, els, p, s, seed=71)
        before = [m.read_raw().tobytes() for m in maps]
        cloud, pose, lab = _changed_frame(al, s, seed=71)
        for ref in (wc.MEAN, wc.ENVELOPE):
            info, rows = _check_parity(al, maps, cloud, pose, lab, sides=sides, reference=ref, min_count=2, threshold=0.05, gate=1.0)
            print(f"{case} ref={ref}: {[info[q] for q in wc.NAMES]} per side {info['side_class'].tolist()}")
            sc = info["side_class"].astype(int)
            assert info["changed_pos"] > 50 and info["changed_neg"] > 50 and info["plane"] == int(lab.sum())
            if sides >= 2:   # both classes on at least two sides
                assert int((sc[:, wc.CHANGED_POS] > 5).sum()) >= 2 and int((sc[:, wc.CHANGED_NEG] > 5).sum()) >= 2
            assert info["unchanged"] > 0.3 * N
        _same_maps(al, maps)   # no map was changed
        assert [m.read_raw().tobytes() for m in maps] == before


def test_sizes(gm):
    """The compaction's tile is 4096 points, a wave 64: n at every edge of both, across the clothoid -> arc joint; a frame
    in which every mapped point is changed and one in which none is."""
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al, maps = _surveyed(c, els, p, s, seed=72)
        big, pose = al_np.frame(al, s, 9001, seed=72)
        lab = (np.arange(9001) % 23 == 0).astype(np.uint8)
        for n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 9001):
            info, rows = _check_parity(al, maps, big[:n], pose, lab[:n], sides=2, min_count=1, threshold=0.05)
            assert info["n_points"] == n
        r = np.linalg.norm(big[:, 1:], axis=1, keepdims=True)
        out = big.copy()
        out[:, 1:] = (out[:, 1:] * ((r + 0.3) / r)).astype(np.float32)
        info, rows = _check_parity(al, maps, out, pose, None, sides=2, min_count=1, threshold=0.05)
        print("every point displaced:", [info[q] for q in wc.NAMES])
        assert info["unchanged"] == 0 and info["changed_neg"] == 0 and len(rows) == info["changed_pos"] > 0.8 * 9001
        info, rows = _check_parity(al, maps, big, pose, None, sides=2, min_count=1, threshold=8.0)
        assert len(rows) == 0 and info["changed_pos"] == info["changed_neg"] == 0 and info["unchanged"] > 0.8 * 9001


def _frame_rows_equal(frame_rows, stage_rows, input_row):
    """A frame call's rows against the stage call's on the slot's valid cloud: everything but `row`, which is the input row."""
    assert len(frame_rows) == len(stage_rows)
    for q in FLOATS + ("cell", "index"):
        assert frame_rows[q].tobytes() == stage_rows[q].tobytes(), q
    assert np.array_equal(frame_rows["row"], input_row[frame_rows["index"]].view(np.uint32))


def test_frame_path_and_ordering(gm):
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    kw = dict(neighborRadius=synth.fixed_k_radius(N))
    ck = dict(min_count=1, threshold=0.05)
    with gm.GeometricMapping(flags=PLANE, n_slots=3, **kw) as c:
        al, maps = _surveyed(c, els, p, s, seed=73)
        frames = [_changed_frame(al, s + d, seed=73)[:2] for d in (0.0, 0.25, 0.6)]
        # (a) check_frame is check_points of the slot's valid cloud and labels, bit for bit; no map changes
        c.process_frame(frames[0][0])
        plan = al.check_frame(0, frames[0][1], **ck)
        info, rows = al.check_result(0)
        assert plan["n_sides"] == 2 and info["n_sides"] == 2 and len(rows) > 100
        xyz, row = c.cropped_cloud()
        lab = c.labels()
        i2, r2, _ = al.check_points(xyz, frames[0][1], labels=lab, **ck)
        _frame_rows_equal(rows, r2, row)
        assert all(np.array_equal(info[q], i2[q]) for q in info)
        _check_parity(al, maps, xyz, frames[0][1], lab, sides=2, **ck)
        _same_maps(al, maps)
        # (b) add on slot 0, check on slot 1, add on slot 2: the check sees the first add and not the second
        for k in range(3):
            c.submit_frame(k, frames[k][0])
        al.add_frame(0, frames[0][1])
        al.check_frame(1, frames[1][1], **ck)
        al.add_frame(2, frames[2][1])
        valid = []
        for k in range(3):
            c.wait_frame(k)
            valid.append((c.cropped_cloud(k), c.labels(k)))
        info, rows = al.check_result(1)
        al.sync()
        (x0, _), l0 = valid[0]
        (x1, row1), l1 = valid[1]
        (x2, _), l2 = valid[2]
        plan0 = al.add_plan(frames[0][1])
        el0 = al_np.owner32(x0, plan0)
        for i in plan0["side_element"]:
            maps[i].add_points(x0[el0 == i], frames[0][1], labels=l0[el0 == i], outputs=False)
        i1, r1 = _check_parity_ref(maps, al, x1, frames[1][1], l1, **ck)
        _frame_rows_equal(rows, r1, row1)
        assert [info[q] for q in wc.NAMES] == i1 and info["n_points"] == len(x1)
        plan2 = al.add_plan(frames[2][1])
        el2 = al_np.owner32(x2, plan2)
        for i in plan2["side_element"]:
            maps[i].add_points(x2[el2 == i], frames[2][1], labels=l2[el2 == i], outputs=False)
        _same_maps(al, maps)


def _check_parity_ref(maps, al, xyz, pose, lab, **kw):
    """The reference of a check from the standalone maps alone: (the seven summed classes, the rows with side bits)."""
    plan = al.add_plan(pose)
    el = al_np.owner32(xyz, plan)
    cls = np.zeros(len(wc.NAMES), np.int64)
    parts = []
    for k, i in enumerate(plan["side_element"]):
        sub = np.flatnonzero(el == i)
        ri, rr, _ = maps[i].check_points(xyz[sub], pose, labels=lab[sub], outputs=False, **kw)
        cls += [ri[q] for q in wc.NAMES]
        rr = rr.copy()
        rr["index"] = sub[rr["index"]]
        rr["row"] = rr["index"]
        rr["cell"] = (rr["cell"].view(np.uint32) | np.uint32(k << 24)).view(np.int32)
        parts.append(rr)
    rows = np.concatenate(parts)
    return [int(v) for v in cls], rows[np.argsort(rows["index"], kind="stable")]


@pytest.mark.parametrize("skip,min_delta,same_pose", ((acn.SKIP_NEG, 0.0, True), (acn.SKIP_POS, 0.2, True),
                                                      (acn.SKIP_NEG | acn.SKIP_POS, 0.0, False), (acn.SKIP_NEG | acn.SKIP_POS, 0.2, True)))
def test_checked_add(gm, skip, min_delta, same_pose):
    """check_frame then add_frame_checked: every element map is the standalone map's add_points of the owned sub-cloud with
    the skipped indices deleted; add_points_checked with the same rows, shuffled and doubled, gives the same bytes; the counts
    are the twin's over the union."""
    els, s, _ = lc.record_case("clothoid_arc:after")
    p = lc.prm()
    kw = dict(neighborRadius=synth.fixed_k_radius(N))
    ck = dict(min_count=1, threshold=0.05)
    ap = dict(skip=skip, min_delta=min_delta)
    with gm.GeometricMapping(flags=PLANE, **kw) as c:
        al, maps = _surveyed(c, els, p, s, seed=74)
        al2, _ = _surveyed(c, els, p, s, seed=74)
        cloud, pose, _ = _changed_frame(al, s, seed=74)
        pose_add = pose if same_pose else al_np.frame(al, s + 0.125, 8, seed=74)[1]
        c.process_frame(cloud)
        al.check_frame(0, pose, **ck)
        plan = al.add_frame_checked(0, pose_add, **ap)
        got = al.add_checked_result(0)
        _, rows = al.check_result(0)
        xyz, _ = c.cropped_cloud()
        lab = c.labels()
        assert plan["n_sides"] == 2 and all(np.array_equal(plan[q], v) for q, v in al.add_plan(pose_add).items())
        n = len(xyz)
        row_cls, skipped = acn.select(rows, n, **ap)
        print(f"skip={skip} min_delta={min_delta}: {len(rows)} rows, {len(skipped)} skipped of {n}; {got}")
        assert len(skipped) > 50 and (skip == 3 or len(skipped) < len(rows))   # (one sign alone leaves the other's rows kept)
        keep = acn.keep(n, skipped)
        el = al_np.owner32(xyz, plan)
        for i in plan["side_element"]:
            sub = keep & (el == i)
            maps[i].add_points(xyz[sub], pose_add, labels=lab[sub], outputs=False)
        _same_maps(al, maps)
        # the stage call, the rows shuffled and doubled
        rng = np.random.default_rng(5)
        shuffled = np.concatenate([rows, rows[:: 3]])[rng.permutation(len(rows) + len(rows[:: 3]))]
        i2, res, cell, el2 = al2.add_points_checked(xyz, pose_add, shuffled, labels=lab, **ap)
        _same_maps(al2, maps)
        assert np.array_equal(el2, el) and np.all(cell[skipped] == -1)
        gate = float(al.element(0).prm.gate)
        want = acn.info(rows, res, cell, gate, labels=lab, **ap)
        for q in ("min_delta_q", "n_points", "skipped", "plane", "beyond_gate", "outside", "mapped", "n_rows", "rows_neg", "rows_pos",
                  "rows_kept", "rows_rejected"):
            assert got[q] == want[q], (q, got[q], want[q])
        want2 = acn.info(shuffled, res, cell, gate, labels=lab, **ap)
        assert all(i2[q] == want2[q] for q in want2 if q != "status")
        # a check left from an earlier frame is refused
        c.process_frame(cloud)
        with pytest.raises(_lib.GmError) as ex:
            al.add_frame_checked(0, pose_add, **ap)
        assert ex.value.status == _lib.GM_ERR_NOT_READY


def test_checked_add_without_selected_rows_and_mask_edges(gm):
    els, s, _ = lc.record_case("arc_clothoid:before")
    p = lc.prm()
    kw = dict(neighborRadius=synth.fixed_k_radius(N))
    with gm.GeometricMapping(**kw) as c:
        al, maps = _surveyed(c, els, p, s, seed=75)
        ref, _ = _surveyed(c, els, p, s, seed=75)
        cloud, pose, _ = _changed_frame(al, s, seed=75)
        # no row is selected (every |delta| < 8 m): the result is add_frame's
        c.process_frame(cloud)
        al.check_frame(0, pose, min_count=1)
        al.add_frame_checked(0, pose, min_delta=8.0)
        got = al.add_checked_result(0)
        assert got["skipped"] == 0 and got["rows_kept"] == got["n_rows"] > 100
        c.process_frame(cloud)
        ref.add_frame(0, pose)
        _same_maps(al, [ref.element(i) for i in range(al.n_elements)])
        xyz, _ = c.cropped_cloud()
        plan = al.add_plan(pose)
        el = al_np.owner32(xyz, plan)
        for i in plan["side_element"]:
            maps[i].add_points(xyz[el == i], pose, outputs=False)
        _same_maps(al, maps)
        # rows that name the first and the last point of a mask word and of the cloud
        for n in (65, 4097):
            sub = np.ascontiguousarray(np.tile(xyz, (2, 1))[:n])
            idx = sorted({0, 63, 64, n - 1})
            rows = np.zeros(len(idx) + 1, api.WALL_CHECK_POINT)
            rows["index"] = idx + [n]   # (the last one is rejected: index >= n_points)
            rows["delta"] = [0.5 if q % 2 else -0.5 for q in range(len(rows))]
            info, res, cell, e2 = al.add_points_checked(sub, pose, rows)
            assert info["skipped"] == len(idx) and info["rows_rejected"] == 1 and info["rows_pos"] + info["rows_neg"] == len(idx)
            assert np.all(cell[idx] == -1) and np.all(np.isfinite(res[idx]))
            keep = acn.keep(n, idx)
            for i in plan["side_element"]:
                m = keep & (e2 == i)
                maps[i].add_points(sub[m], pose, outputs=False)
            _same_maps(al, maps)


def test_the_loop_end_to_end(gm):
    """locate -> check with the located pose -> checked add, across the clothoid -> arc joint, on the frame and with the
    thresholds of the alignment-locate test (test_located_pose_clears_the_checks): under a pose 5 cm / 0.5 degrees off the
    check reports many changed points, under the located pose none beyond the planted ones, and the checked add leaves
    exactly those out."""
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    rule = api.WallAlignmentRule(els, **p)
    sj = al_np.spans(els)[j][1]
    ck = dict(threshold=0.03, min_count=2)
    excess = 0
    with gm.GeometricMapping(neighborRadius=synth.fixed_k_radius(N)) as c:
        al = c.wall_alignment(els, **p)
        for s in np.arange(sj - 4.0, sj + 4.01, 1.0):
            al.add_points(*al_np.frame(rule, s, N, seed=61, sigma=0.002), outputs=False)
        for k, s in enumerate((sj - 1.0, sj + 1.0)):
            cloud, true = al_np.frame(rule, s + 0.37, N, seed=61, sigma=0.002)
            planted = np.arange(N) % 40 == 7
            r = np.linalg.norm(cloud[:, 1:], axis=1, keepdims=True)
            cloud = cloud.copy()
            cloud[planted, 1:] = (cloud[planted, 1:] * ((r[planted] - 0.3) / r[planted])).astype(np.float32)
            pin = lc.perturbed(true, np.random.default_rng(70 + k))
            c.process_frame(cloud)
            _, row = c.cropped_cloud()
            al.locate_frame(0, pin, reference=aln.MAP, min_count=2)
            loc = al.locate_result(0)
            assert loc["status"] == _lib.GM_LOCATE_OK and loc["n_sides"] == 2
            al.check_frame(0, pin, **ck)
            off, _ = al.check_result(0)
            al.check_frame(0, loc["pose"], **ck)
            on, rows = al.check_result(0)
            frames_before = al.info()["frames"]
            al.add_frame_checked(0, loc["pose"])
            added = al.add_checked_result(0)
            n_planted = int(planted[row].sum())
            print(f"s={s}: changed under the perturbed pose {off['changed_pos'] + off['changed_neg']}, under the located pose "
                  f"{len(rows)} of {n_planted} planted; skipped {added['skipped']}")
            assert off["changed_pos"] + off["changed_neg"] > n_planted   # (points of the bare wall are reported as changed)
            excess += off["changed_pos"] + off["changed_neg"] - n_planted
            assert np.all(planted[row[rows["index"]]]) and 0.9 * n_planted <= len(rows) <= n_planted
            assert on["changed_pos"] == 0 and on["changed_neg"] == len(rows)
            assert added["skipped"] == len(rows) and added["n_points"] == len(row)
            assert al.info()["frames"] == frames_before + 2
    # 2.5 cm of lateral error plus half a degree over a 4 m half-frame is 3 to 5 cm at the frame's ends: beyond the 3 cm
    # threshold on a good part of the wall
    assert excess > 100
