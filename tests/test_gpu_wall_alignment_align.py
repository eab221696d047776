"""GPU tests of the align on a wall alignment (gm_wall_alignment_align_*, csrc/k_wall_align_joint.hip +
gm_wall_alignment_align.hip): the score table byte for byte against the twin (tests/wall_alignment_align_np.py) fed the
device's own (e, cell) pairs and the element maps' raw cells; the class counts per side, the per-point residual, cell and
element against the check's kernel on the same chains and against the twin's chain; the plan's integers; the edges of the
bin kernel, of the patch, of the joint's place in the patch and of the map image; the delegation to an element map; the
truth of shifted poses across two joints; a smooth wall; the check the align repairs; the frame path and the ordering."""
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_align_np as an  # noqa: E402
import wall_alignment_align_cases as ac  # noqa: E402
import wall_alignment_align_np as aan  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402

pytestmark = pytest.mark.gpu
N = lc.N
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
# The twin's chain takes the sector from an fp64 atan2 of the device's fp32 (yc, z): a point within rounding of a cell's edge
# may fall in the neighbouring cell.  test_gpu_wall_align.py's cap for the same ambiguity.
AMBIGUOUS_CAP = 0.02
SWEEP = dict(half_patch_stations=12, min_count=2, min_frame_count=1)   # 3 m of a frame's 4.5: far points leave the patch


def _kinds(al):
    eps = [al.element_params(i) for i in range(al.n_elements)]
    return ([int(e[0].n_stations) for e in eps],
            [aln.CLOTHOID if e[2] is not None else (aln.ARC if e[1] is not None else aln.STRAIGHT) for e in eps])


def _survey(c, els, p, s, n=N, offsets=(-3.0, -1.5, 0.0, 1.5, 3.0), tex=ac.TEX):
    """An alignment that holds a survey of the textured wall around s, added through the alignment."""
    al = c.wall_alignment(els, **p)
    for cloud, pose in ac.survey_frames(al, s, n, offsets, tex):
        al.add_points(cloud, pose, outputs=False)
    al.sync()
    return al


def _raws(al):
    al.sync()
    return [al.element(i).read_raw() for i in range(al.n_elements)]


def _sweep_frame(al, s, n=N, seed=11, half=4.5):
    """The wall seen from s: every 23rd point a plane point, every 11th pushed a quarter further from the sensor."""
    cloud, true = ac.textured_frame(al, s, n, seed=seed, half=half)
    cloud = cloud.copy()
    cloud[np.arange(n) % 11 == 3] *= np.float32(1.25)
    return cloud, (np.arange(n) % 23 == 0).astype(np.uint8), true


def against_twin(al, grid, cloud, lab, pose, raws, per_point=True, **kw):
    """One stage call against the twin.  Returns (info, table)."""
    ap = an.prm(**kw)
    nsec = int(grid["n_sectors"])
    n = len(cloud)
    info, tab, out = al.align_points(cloud, pose, labels=lab, **kw)
    plan = info["align_plan"]
    add = plan["add"]
    nst, kinds = _kinds(al)
    # the plan: the add's, and the twin's integers exactly
    host = al.add_plan(pose)
    assert all(np.array_equal(add[q], host[q]) for q in host) and all(np.array_equal(info["plan"][q], host[q]) for q in host)
    tp = aan.plan(add, nst, kinds, ap)
    assert (plan["anchor_global"], plan["total"], plan["home"], plan["own"]) == (tp["anchor_global"], tp["total"], tp["home"], tp["own"])
    assert plan["row0"].tolist() == tp["row0"].tolist() and plan["pieces"] == tp["pieces"]
    assert (info["anchor_global"], info["element"], info["n_sides"], info["chainage"]) == (tp["anchor_global"], add["element"], add["n_sides"],
                                                                                           add["chainage"])
    assert info["anchor_station"] == add["side_anchor"][tp["home"]] and info["n_points"] == n
    res, cell, el = out["e"], out["cell"], out["element"]
    labs = np.zeros(n, np.uint8) if lab is None else lab
    # the owner, exactly
    assert np.array_equal(el, al_np.owner32(cloud, add))
    side = el - add["side_element"][0]
    # the classes from the device's pairs, summed and per side
    plane = labs == 1
    gate = np.float32(ap["gate"])
    with np.errstate(invalid="ignore"):
        beyond = ~plane & ~(np.abs(res) <= gate)
    binned = cell >= 0
    assert not np.any(binned & (plane | beyond)) and np.all(np.isnan(res[plane]))
    assert np.all(cell[binned] < 2 * ap["half_patch_stations"] * nsec)
    cls = np.where(plane, aan.PLANE, np.where(beyond, aan.BEYOND, np.where(binned, aan.BINNED, aan.OUTSIDE)))
    want = np.array([[int(((side == k) & (cls == q)).sum()) for q in range(4)] for k in range(add["n_sides"])], np.uint32)
    assert np.array_equal(info["side_class"], want), (info["side_class"].tolist(), want.tolist())
    assert [info[q] for q in an.CLASSES] == [int(v) for v in want.sum(axis=0)]
    # the patch, the table and the selection
    psum, pcnt = an.patch_from(res, cell, 2 * ap["half_patch_stations"] * nsec)
    assert info["patch_cells_usable"] == int((pcnt >= ap["min_frame_count"]).sum())
    twin = an.table(psum, pcnt, aan.concat_raw(raws, nst, nsec), tp["anchor_global"], nsec, ap)
    assert tab.tobytes() == twin.tobytes()
    sel = aan.select(twin, al, pose, add, tp, grid, ap)
    for k in ("status", "anchor_station", "overlap", "best_station", "best_sector"):
        assert info[k] == sel[k], (k, info[k], sel[k])
    for k in ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction"):
        assert np.isclose(info[k], sel[k], rtol=1e-14, atol=0.0, equal_nan=True), (k, info[k], sel[k])
    assert np.allclose(info["pose"], sel["pose"], rtol=0.0, atol=1e-12, equal_nan=True)
    if info["status"] & _lib.GM_ALIGN_FAILED_MASK:
        assert np.all(np.isnan(info["pose"]))
    if per_point and n and not tp["own"]:
        # the same chains in the check's kernel under the same gate: e bit for bit, and the cell of every point the check maps
        ci, _, co = al.check_points(cloud, pose, labels=lab, gate=ap["gate"], min_count=1)
        assert np.array_equal(co["element"], el)
        assert np.array_equal(co["e"].view(np.uint32)[~plane], res.view(np.uint32)[~plane])
        mapped = co["cell"] >= 0
        jr = co["cell"][mapped] // nsec - np.asarray(add["side_anchor"], np.int64)[side[mapped]] + tp["row0"][side[mapped]]
        inside = (jr >= 0) & (jr < 2 * ap["half_patch_stations"])
        assert np.array_equal(cell[mapped], np.where(inside, jr * nsec + co["cell"][mapped] % nsec, -1))
        # the twin's chain on the plan's blocks: the owner exactly, the cell but for a cell's edge cases (the neighbouring
        # sector of the same row, or the same sector of the neighbouring row)
        t = aan.chains(cloud, lab, al.locate_plan(pose), tp["row0"], grid, ap)
        assert np.array_equal(t["side"], side)
        differ = t["cell"] != cell
        assert differ.mean() <= AMBIGUOUS_CAP, differ.mean()
        both = differ & (t["cell"] >= 0) & (cell >= 0)
        dk = np.abs(t["cell"][both] % nsec - cell[both] % nsec)
        dr = np.abs(t["cell"][both] // nsec - cell[both] // nsec)
        assert np.all(((dr == 0) & ((dk == 1) | (dk == nsec - 1))) | ((dr == 1) & (dk == 0)))
    return info, tab


# ---- 1. table parity ----

@pytest.mark.parametrize("case", ac.PARITY_CASES)
def test_table_parity(gm, case):
    els, s, sides = lc.record_case(case)
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        raws = _raws(al)
        before = [r.tobytes() for r in raws]
        cloud, lab, _ = _sweep_frame(al, s)
        pose = ac.moved(al, s, 1, -1, dict(p))
        info, tab = against_twin(al, dict(p), cloud, lab, pose, raws, **SWEEP)
        print(case, {q: info[q] for q in an.CLASSES}, info["side_class"].tolist(), "best", info["best_station"], info["best_sector"],
              "overlap", info["overlap"], f"distinction {info['distinction']:.2f}")
        assert info["n_sides"] == sides and all(info[q] > 0 for q in an.CLASSES)
        assert (info["best_station"], info["best_sector"]) == (1, -1) and not info["status"] & _lib.GM_ALIGN_FAILED_MASK
        if sides >= 2:
            assert int((info["side_class"][:, aan.BINNED] > 0).sum()) >= 2
        assert [r.tobytes() for r in _raws(al)] == before   # no map was changed


# ---- 2. edges ----

@pytest.mark.parametrize("n", (0, 1, 65, 2049, 4097))
def test_sizes(gm, n):
    """A wave's edge, the unroll's edge and the second block, across the clothoid -> arc joint."""
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        cloud, lab, _ = _sweep_frame(al, s, n=4097)
        info, _ = against_twin(al, dict(p), cloud[:n], lab[:n], ac.moved(al, s, 1, -1, dict(p)), _raws(al), **SWEEP)
        assert info["n_points"] == n and info["n_sides"] == 2
        if n < 64:
            assert info["status"] == _lib.GM_ALIGN_NO_OVERLAP and np.all(np.isnan(info["pose"]))


@pytest.mark.parametrize("half_patch", (64, 63))
def test_largest_patch(gm, half_patch):
    """2P n_sectors = 8192 and the next size below on 64 sectors (8192 - n_sectors is no multiple of 2 n_sectors: 8064)."""
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm(n_sectors=64)
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        cloud, lab, _ = _sweep_frame(al, s)
        info, _ = against_twin(al, dict(p), cloud, lab, ac.moved(al, s, 1, -1, dict(p)), _raws(al), half_patch_stations=half_patch,
                               min_count=2, min_frame_count=1)
        assert 2 * half_patch * 64 in (8192, 8064) and info["binned"] > 0.5 * N and info["n_sides"] == 2


@pytest.mark.parametrize("row", ("0", "P-1", "P", "2P-1"))
def test_joint_at_patch_row(gm, row):
    """The clothoid -> arc joint at the patch's first row, on both sides of its middle and at its last row."""
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    P = ac.AP["half_patch_stations"]
    r = dict([("0", 0), ("P-1", P - 1), ("P", P), ("2P-1", 2 * P - 1)])[row]
    sj = al_np.spans(els)[j][1]
    s = sj + (P - r) * al_np.DS + 0.1          # the sensor's station is P - r stations past the joint's
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        cloud, lab, _ = _sweep_frame(al, s)
        pose = ac.moved(al, s, 0, 0, dict(p))
        info, _ = against_twin(al, dict(p), cloud, lab, pose, _raws(al), **ac.AP)
        plan = info["align_plan"]
        base_arc = [q for q in plan["pieces"] if q[0] == j + 1][0][1]
        assert base_arc - (plan["anchor_global"] - P) == r and info["n_sides"] >= 2


@pytest.mark.parametrize("side", (-0.0005, 0.0005))
def test_sensor_within_a_millimetre_of_a_joint(gm, side):
    els, j = lc.JOINTS["straight_clothoid"]
    p = lc.prm()
    s = al_np.spans(els)[j][1] + side
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        cloud, lab, true = _sweep_frame(al, s)
        _, pose = al_np.frame(al, s, 1, seed=0, lateral=(0.0, 0.0), yaw_deg=0.0)   # the sensor on the axis, at s exactly
        world = cloud.astype(np.float64) @ true[:, :3].T + true[:, 3]
        cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(np.float32)
        info, _ = against_twin(al, dict(p), cloud, lab, pose, _raws(al), **SWEEP)
        assert info["element"] == (j if side < 0 else j + 1) and info["n_sides"] == 2
        assert np.all(info["side_class"][:, aan.BINNED] > 500)


@pytest.mark.parametrize("s", (1.0, 39.0))
def test_rows_outside_the_alignment(gm, s):
    """Two arcs of 20 m: near the start the image and the patch have rows before station 0, near the end past `total`."""
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, lc.COMPOUND, p, s)
        cloud, lab, _ = _sweep_frame(al, s)
        info, tab = against_twin(al, dict(p), cloud, lab, ac.moved(al, s, 1, -1, dict(p)), _raws(al), **ac.AP)
        plan = info["align_plan"]
        g0, g1 = plan["anchor_global"] - 18 - 6, plan["anchor_global"] + 18 + 6
        assert (g0 < 0) if s < 20.0 else (g1 > plan["total"])
        assert info["binned"] > 0.5 * N and (info["best_station"], info["best_sector"]) == (1, -1)


def test_pieces_that_are_not_sides(gm):
    """Two arcs of four stations beyond the add's reach (17.6 m) but inside P + A = 109 stations: one straight side, four
    pieces, and the rows of the short elements enter the table (a frame of 10 m of reach: its patch rows up to station 44
    meet the arcs' stations 76 .. 83 at the shifts from 32 on)."""
    short = dict(kind="arc", n_stations=4, turn=lc.T, curvature=lc.K80)
    els = [dict(kind="straight", n_stations=76), short, short, dict(kind="straight", n_stations=80)]
    p = lc.prm()
    kw = dict(half_patch_stations=45, max_station_shift=64, max_sector_shift=2, min_count=2, min_frame_count=1)
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        for d in (1.0, 4.0, 8.0, 12.0, 16.0, 19.0, 20.5, 23.0):
            al.add_points(*ac.textured_frame(al, d, N, seed=int(10 * d)), outputs=False)
        raws = _raws(al)
        cloud, lab, _ = _sweep_frame(al, 1.0, half=10.0)
        pose = ac.moved(al, 1.0, 0, 0, dict(p))
        info, tab = against_twin(al, dict(p), cloud, lab, pose, raws, **kw)
        plan = info["align_plan"]
        assert info["n_sides"] == 1 and plan["own"] == 0 and [q[0] for q in plan["pieces"]] == [0, 1, 2, 3]
        # without the short elements' rows the outer shifts lose overlap
        hollow = [r if i in (0, 3) else None for i, r in enumerate(raws)]
        psum, pcnt = an.patch_from(*[al.align_points(cloud, pose, labels=lab, **kw)[2][q] for q in ("e", "cell")], 2 * 45 * 90)
        nst, _ = _kinds(al)
        less = an.table(psum, pcnt, aan.concat_raw(hollow, nst, 90), plan["anchor_global"], 90, an.prm(**kw))
        assert int(less["n"].sum()) < int(tab["n"].sum())


@pytest.mark.parametrize("kw", (dict(max_sector_shift=0), dict(max_station_shift=0), dict(max_station_shift=0, max_sector_shift=0)))
def test_one_row_or_one_column_of_shifts(gm, kw):
    els, s, _ = lc.record_case("arc_clothoid:after")
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s)
        cloud, lab, _ = _sweep_frame(al, s)
        info, tab = against_twin(al, dict(p), cloud, lab, ac.moved(al, s, 0, 0, dict(p)), _raws(al), **dict(SWEEP, **kw))
        assert tab.shape == (2 * info["max_station_shift"] + 1, 2 * info["max_sector_shift"] + 1)
        assert (info["best_station"], info["best_sector"]) == (0, 0) and not info["status"] & _lib.GM_ALIGN_AT_BORDER


def test_the_table_does_not_depend_on_the_score_blocks(gm, monkeypatch):
    """GM_WALL_ALIGN_ROWS (read when a map is created) at two values: the same bytes."""
    els, s, _ = lc.record_case("clothoid_arc:after")
    p = lc.prm()
    got = []
    for rows in ("3", "16"):
        monkeypatch.setenv("GM_WALL_ALIGN_ROWS", rows)
        with gm.GeometricMapping() as c:
            al = _survey(c, els, p, s)
            cloud, lab, _ = _sweep_frame(al, s)
            info, tab, _ = al.align_points(cloud, ac.moved(al, s, 2, 1, dict(p)), labels=lab, **ac.AP)
            got.append((tab.tobytes(), info["bytes"]))
    assert got[0] == got[1] and np.frombuffer(got[0][0], an.SCORE)["n"].max() > 1000


# ---- 3. delegation ----

def test_delegation_to_the_element_map(gm):
    """Mid-straight the align is the element map's own; with the image reaching over the element's end it is not, and the
    outer shifts gain overlap from the neighbour's rows."""
    els = al_np.elements5(n_straight=160, n_clothoid=160, n_arc=160)
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = c.wall_alignment(els, **p)
        for d in np.arange(14.0, 46.1, 2.0):
            al.add_points(*ac.textured_frame(al, d, N, seed=int(d)), outputs=False)
        raws = _raws(al)
        m0 = al.element(0)
        cloud, lab, _ = _sweep_frame(al, 20.0)
        pose = ac.moved(al, 20.0, 2, -1, dict(p))
        info, tab, out = al.align_points(cloud, pose, labels=lab, **ac.AP)
        mi, mt, mres, mcell = m0.align_points(cloud, pose, labels=lab, **ac.AP)
        assert info["align_plan"]["own"] == 1 and info["n_sides"] == 1
        assert tab.tobytes() == mt.tobytes() and info["bytes"][4:] == mi["bytes"][4:]
        assert info["pose"].tobytes() == mi["pose"].tobytes()
        assert out["e"].tobytes() == mres.tobytes() and np.array_equal(out["cell"], mcell) and np.all(out["element"] == 0)
        assert info["side_class"].tolist() == [[mi[q] for q in an.CLASSES]]
        against_twin(al, dict(p), cloud, lab, pose, raws, **ac.AP)
        # the same element, two metres before its end: the map's own align loses the rows past the end
        s = 38.0
        cloud, lab, _ = _sweep_frame(al, s)
        pose = ac.moved(al, s, 2, -1, dict(p))
        info, tab = against_twin(al, dict(p), cloud, lab, pose, raws, **ac.AP)
        mi, mt, _, _ = m0.align_points(cloud, pose, labels=lab, **ac.AP)
        assert info["align_plan"]["own"] == 0 and info["element"] == 0
        assert tab.tobytes() != mt.tobytes() and np.all(tab["n"] >= mt["n"])
        assert int(tab["n"][-1].sum()) > int(mt["n"][-1].sum())   # the outermost forward shifts


# ---- 4. truth ----

@pytest.mark.parametrize("case", ac.TRUTH_CASES)
def test_truth(gm, case):
    els, s, _ = lc.record_case(case)
    p = lc.prm()
    grid = dict(p)
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s, n=ac.SURVEY_N, offsets=ac.SURVEY_OFFSETS)
        cloud, true = ac.textured_frame(al, s, ac.TRUTH_N, seed=ac.TRUTH_SEED)
        for sa, sb in ac.WHOLE:
            info, _, _ = al.align_points(cloud, ac.moved(al, s, sa, sb, grid), outputs=False, **ac.AP)
            print(f"{case} ({sa}, {sb}): status {info['status']:#x} distinction {info['distinction']:.2f}")
            assert (info["status"], info["best_station"], info["best_sector"]) == (_lib.GM_ALIGN_OK, sa, sb)
        for sa, sb in ac.FRACTIONAL:
            info, _, _ = al.align_points(cloud, ac.moved(al, s, sa, sb, grid), outputs=False, **ac.AP)
            es, ek = ac.shift_error(info, sa, sb)
            print(f"{case} ({sa}, {sb}): errors {es:.4f} station, {ek:.4f} sector")
            assert not info["status"] & _lib.GM_ALIGN_FAILED_MASK
            assert es <= ac.BOUND_STATION and ek <= ac.BOUND_SECTOR
            dt = np.linalg.norm(info["pose"][:, 3] - true[:, 3])
            assert dt <= (ac.BOUND_STATION + 0.01) * al_np.DS + 1e-9   # the pose lands on the true one, within the shift's error


# ---- 5. a smooth wall; an anchor far outside ----

def test_a_smooth_wall_is_ambiguous_and_a_far_anchor_has_no_overlap(gm):
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s, tex=None)
        cloud, _ = ac.textured_frame(al, s, N, seed=3, tex=None)
        info, _, _ = al.align_points(cloud, ac.moved(al, s, 1, 0, dict(p)), **ac.AP)
        print(f"smooth: status {info['status']:#x} distinction {info['distinction']:.3f}")
        assert info["status"] & _lib.GM_ALIGN_AMBIGUOUS and not info["status"] & _lib.GM_ALIGN_FAILED_MASK
        # 60 m past the end of the alignment: every image row is outside [0, total)
        far = al_np.frame(al, 160.0, 1, seed=0)[1]
        info, tab, _ = al.align_points(cloud, far, **ac.AP)
        assert info["status"] == _lib.GM_ALIGN_NO_OVERLAP and info["align_plan"]["n_pieces"] == 0 and not tab["n"].any()
        for q in ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction"):
            assert np.isnan(info[q]), q
        assert np.all(np.isnan(info["pose"])) and info["binned"] > 0


# ---- 6. closing the loop ----

def test_closing_the_loop(gm):
    case = "clothoid_arc:before"
    els, s, _ = lc.record_case(case)
    p = lc.prm()
    with gm.GeometricMapping() as c:
        al = _survey(c, els, p, s, n=ac.SURVEY_N, offsets=ac.SURVEY_OFFSETS)
        cloud, true = ac.textured_frame(al, s, ac.TRUTH_N, seed=ac.TRUTH_SEED)
        off = ac.moved(al, s, *ac.LOOP_SHIFT, dict(p))
        changed = lambda pose: (lambda i: i["changed_pos"] + i["changed_neg"])(al.check_points(cloud, pose, outputs=False, **ac.LOOP_CHECK)[0])  # noqa: E731
        n_off = changed(off)
        info, _, _ = al.align_points(cloud, off, outputs=False, **ac.AP)
        n_on, n_true = changed(info["pose"]), changed(true)
        print(f"changed under the caller's pose {n_off} (twin {ac.LOOP_TWIN_OFF}), under the aligned pose {n_on} "
              f"(twin {ac.LOOP_TWIN_ALIGNED}), under the true pose {n_true} (twin {ac.LOOP_TWIN_TRUE})")
        assert (info["best_station"], info["best_sector"]) == ac.LOOP_SHIFT
        assert n_off > 10 * max(ac.LOOP_TWIN_ALIGNED, ac.LOOP_TWIN_TRUE)          # the wall is reported
        assert n_on <= 2 * ac.LOOP_TWIN_ALIGNED + n_true


# ---- 7. frame path and ordering ----

@pytest.mark.parametrize("graph", (False, True))
def test_frame_path_is_the_stage_path(gm, graph):
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    flags = PLANE | (_lib.GM_CFG_GRAPH if graph else 0)
    with gm.GeometricMapping(flags=flags, neighborRadius=synth.fixed_k_radius(N)) as c:
        al = _survey(c, els, p, s)
        raws = _raws(al)
        cloud, _, _ = _sweep_frame(al, s)
        pose = ac.moved(al, s, 1, -1, dict(p))
        c.process_frame(cloud)
        plan = al.align_frame(0, pose, **SWEEP)
        info, tab = al.align_result(0)
        xyz, _ = c.cropped_cloud()
        lab = c.labels()
        i2, t2, _ = al.align_points(xyz, pose, labels=lab, **SWEEP)
        assert plan["add"]["n_sides"] == 2 and all(np.array_equal(plan[q], i2["align_plan"][q]) for q in plan if q != "add")
        assert tab.tobytes() == t2.tobytes() and info["bytes"] == i2["bytes"] and info["n_points"] == len(xyz) > 0.5 * N
        assert np.array_equal(info["side_class"], i2["side_class"])
        assert [r.tobytes() for r in _raws(al)] == [r.tobytes() for r in raws]


def test_ordering_against_adds_on_pieces_that_are_not_sides(gm):
    """An align on slot 1 sees an add enqueued before it on slot 0 to a piece's map that is no side of the align, and not
    one enqueued after it on slot 2."""
    short = dict(kind="arc", n_stations=4, turn=lc.T, curvature=lc.K80)
    els = [dict(kind="straight", n_stations=76), short, short, dict(kind="straight", n_stations=80)]
    p = lc.prm()
    # (the crop leaves a frame 5 m of reach: patch rows up to station 24 meet the arcs' stations 76 .. 83 at the shifts from 52 on)
    kw = dict(half_patch_stations=45, max_station_shift=64, max_sector_shift=2, min_count=2, min_frame_count=1)
    with gm.GeometricMapping(n_slots=3, neighborRadius=synth.fixed_k_radius(N)) as c:
        al = c.wall_alignment(els, **p)
        ref = c.wall_alignment(els, **p)
        for d in (1.0, 4.0, 8.0, 12.0, 16.0):
            for a in (al, ref):
                a.add_points(*ac.textured_frame(al, d, N, seed=int(10 * d)), outputs=False)
        f0 = ac.textured_frame(al, 23.0, N, seed=230)   # lands on the short arcs and the last straight: pieces, not sides
        f1 = ac.textured_frame(al, 1.0, N, seed=11)
        f2 = ac.textured_frame(al, 21.0, N, seed=210)
        for k, f in enumerate((f0, f1, f2)):
            c.submit_frame(k, f[0])
        a0 = al.add_frame(0, f0[1])
        plan = al.align_frame(1, f1[1], **kw)
        al.add_frame(2, f2[1])
        valid = []
        for k in range(3):
            c.wait_frame(k)
            valid.append(c.cropped_cloud(k)[0])
        info, tab = al.align_result(1)
        al.sync()
        beyond = set(a0["side_element"]) - set(plan["add"]["side_element"])   # the add's maps that are no side of the align
        assert plan["add"]["n_sides"] == 1 and plan["own"] == 0 and len(beyond) >= 2 and beyond <= {q[0] for q in plan["pieces"]}
        # the reference: the first add alone, then the same align as a stage call
        ref.add_points(valid[0], f0[1], outputs=False)
        ri, rt, _ = ref.align_points(valid[1], f1[1], **kw)
        assert tab.tobytes() == rt.tobytes() and info["bytes"] == ri["bytes"]
        later = an.table(*an.patch_from(*[ref.align_points(valid[1], f1[1], **kw)[2][q] for q in ("e", "cell")], 2 * 45 * 90),
                          aan.concat_raw(_raws(al), _kinds(al)[0], 90), plan["anchor_global"], 90, an.prm(**kw))
        assert later.tobytes() != tab.tobytes()   # (the second add would have shown: `al` holds it by now)
        ref.add_points(valid[2], f2[1], outputs=False)
        assert [r.tobytes() for r in _raws(al)] == [r.tobytes() for r in _raws(ref)]
