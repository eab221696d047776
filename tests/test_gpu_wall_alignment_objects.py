"""GPU tests of a check's objects on a wall alignment (gm_wall_alignment_check_objects / _check_objects_rows,
csrc/k_wall_objects_joint.hip + gm_wall_alignment_objects.hip): crafted rows with side bits on a short alignment whose
joints fall inside blocks, byte for byte against the integer twin (tests/wall_alignment_objects_np.py), against
gm_wall_check_objects on ONE straight map of `total` stations fed the rewritten rows, under a shuffled row order and two
tile shapes; the one-side case against the element map's own call; and one frame across the clothoid -> arc joint through
check_frame -> check_objects."""
import contextlib
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_alignment_objects_np as an  # noqa: E402
import wall_objects_np as on  # noqa: E402

pytestmark = pytest.mark.gpu

N_STATIONS, NSEC = [12, 17, 12, 9], 10   # bases 0, 12, 29, 41 (29 and 41 are no multiples of 3); total 50
TOTAL = 50
ELEMENTS = [dict(kind="straight", n_stations=12), dict(kind="arc", n_stations=17, turn=al_np.LEFT, curvature=0.01),
            dict(kind="clothoid", n_stations=12, turn=al_np.LEFT, curvature=0.01, rate=-1e-4), dict(kind="straight", n_stations=9)]
PRM = dict(n_sectors=NSEC, station_length=0.25)
FOUR = dict(element=1, side_element=[0, 1, 2, 3], side_anchor=[22, 10, -7, -19])   # G_f = 22
BLOCKS = [(bs, bk) for bs in (1, 3) for bk in (1, 2)]


@contextlib.contextmanager
def tile(shape):
    old = os.environ.pop("GM_WALL_OBJECT_TILE", None)
    if shape:
        os.environ["GM_WALL_OBJECT_TILE"] = shape
    try:
        yield
    finally:
        os.environ.pop("GM_WALL_OBJECT_TILE", None)
        if old is not None:
            os.environ["GM_WALL_OBJECT_TILE"] = old


def rows_of(cells, per=1, delta=-0.25, seed=0):
    """`per` rows in each (side, station, sector) of the list; deltas of one sign with varying magnitude."""
    rng = np.random.default_rng(seed)
    side = np.repeat([s for s, _, _ in cells], per)
    cell = np.repeat([j * NSEC + k for _, j, k in cells], per)
    rows = on.make_rows(cell, (delta * rng.uniform(0.5, 1.5, len(cell))).astype(np.float32), seed=seed + 1)
    return an.with_sides(rows, side)


def join(*parts):
    rows = np.concatenate(parts)
    rows["index"] = np.arange(len(rows))
    rows["row"] = rows["index"]
    return rows


def _same(got, want, keys=an.INFO_KEYS):
    ginfo, gobj, grow = got[0], got[1], got[-1]
    winfo, wobj, wrow = want[0], want[1], want[-1]
    for k in keys:
        assert ginfo[k] == winfo[k], (k, ginfo[k], winfo[k])
    assert sum(ginfo[k] for k in on.CLASSES) == ginfo["n_rows"]
    assert len(gobj) == len(wobj)
    for i in range(len(wobj)):
        assert gobj[i].tobytes() == wobj[i].tobytes(), (i, gobj[i], wobj[i])
    assert np.array_equal(grow, wrow)


class Rig:
    """One context: the alignment under the default tile and under a tile smaller than the window (4 x 4 blocks: with
    bs = 1 a tile border falls on the joint at global station 12, and 29 and 41 lie inside one), and the straight map of
    `total` stations."""

    def __init__(self, c):
        self.al = c.wall_alignment(ELEMENTS, **PRM)
        with tile("4x4"):
            self.small = c.wall_alignment(ELEMENTS, **PRM)
        self.straight = c.wall_map(n_stations=TOTAL, **PRM)

    def run(self, rows, plan, **op):
        """The stage call against the twin, the straight map, a shuffled order and the small tile; returns the result."""
        got = self.al.objects_of_rows(rows, plan, **op)
        want = an.objects(rows, N_STATIONS, NSEC, plan, **op)
        _same(got, want)
        g, _, _, _ = an.rewrite(rows, N_STATIONS, NSEC, plan)
        _same(got, self.straight.objects_of_rows(g, want[0]["anchor_global"], **op), keys=on.INFO_KEYS)
        perm = np.random.default_rng(len(rows)).permutation(len(rows))
        shuffled = self.al.objects_of_rows(rows[perm], plan, **op)
        _same((shuffled[0], shuffled[1], shuffled[3]), (want[0], want[1], want[2][perm]))
        _same(self.small.objects_of_rows(rows, plan, **op), want)
        return got


@pytest.fixture(scope="module")
def rig(gm):
    with gm.GeometricMapping() as c:
        yield Rig(c)


@pytest.mark.parametrize("bs,bk", BLOCKS)
def test_objects_across_joints(rig, bs, bk):
    op = dict(block_stations=bs, block_sectors=bk, min_block_points=2, min_points=8, connectivity=8)
    # (a) across the joint at 12, four rows on each side: an object only with both halves (min_points 8)
    a = rows_of([(0, 10, 2), (0, 11, 2), (1, 0, 2), (1, 1, 2)], per=2, seed=1)
    # (b) stations 28 (element 1) and 29 (element 2) at sectors 9 and 0: across the joint and the sector seam at once; with
    #     bs = 3 both stations lie in ONE block row J = 9, whose blocks hold stations of two elements
    b = rows_of([(1, 16, 9), (2, 0, 9), (1, 16, 0), (2, 0, 0)], per=2, delta=0.3, seed=2)
    # (c) across the joint at 41 on side 3, diagonally through the seam: (2, 11, 9) and (3, 0, 0)
    d = rows_of([(2, 11, 9), (3, 0, 0)], per=4, seed=3)
    # (d) the window's edges at global 0 and at total
    e = rows_of([(0, 0, 5), (0, 1, 5), (3, 7, 5), (3, 8, 5)], per=4, seed=4)
    rows = join(a, b, d, e)
    info, obj, met, of_row = rig.run(rows, FOUR, **op)
    print(bs, bk, {k: info[k] for k in an.INFO_KEYS}, obj[["label", "sign", "points", "station_min", "station_max"]])
    assert info["rejected"] == 0 and info["side_rows"] == [12, 8, 8, 12] and info["total"] == TOTAL and info["side_first"] == [0, 12, 29, 41]
    first = obj[of_row[0]]
    assert (first["station_min"], first["station_max"], first["points"], first["sign"]) == (10, 13, 8, -1)
    assert set(of_row[:len(a)]) == {of_row[0]} and met[of_row[0]]["element_from"] == 0 and met[of_row[0]]["element_to"] == 1
    across = obj[of_row[len(a) + len(b) + len(d) - 1]]
    assert across["station_min"] == 40 < 41 == across["station_max"] and across["points"] == 8
    assert (across["sector_min"], across["sector_max"], across["sector_max_turned"] - across["sector_min_turned"]) == (0, 9, 1)
    assert obj["station_min"].min() == 0 and obj["station_max"].max() == 49
    sel = slice(len(a), len(a) + len(b))
    seam = obj[of_row[len(a)]]
    assert len(set(of_row[sel])) == 1 and (seam["sign"], seam["points"], seam["station_min"], seam["station_max"]) == (1, 8, 28, 29)
    assert (seam["sector_min"], seam["sector_max"], seam["blocks"]) == (0, 9, 4 if bs == 1 else 2)
    # one row on each side of the joint at 29: with bs = 3 they flag their common block only together
    pair = rig.run(rows_of([(1, 16, 4), (2, 0, 4)], per=1, seed=5), FOUR, **dict(op, min_points=2))
    assert (pair[0]["objects"], pair[0]["sparse"]) == ((1, 0) if bs == 3 else (0, 2))


@pytest.mark.parametrize("bs,bk", BLOCKS)
def test_window_edges_and_rejections(rig, bs, bk):
    op = dict(block_stations=bs, block_sectors=bk, min_block_points=2, min_points=4, connectivity=4, half_window_stations=5)
    e = rows_of([(0, 0, 5), (0, 6, 5), (0, 7, 5), (3, 2, 5), (3, 3, 5), (3, 8, 5)], per=4, seed=5)
    lo = rig.run(e, dict(FOUR, element=0, side_anchor=[2, 0, 0, 0]), **op)    # G_f = 2: stations [0, 7) and their block rows
    hi = rig.run(e, dict(FOUR, element=3, side_anchor=[0, 0, 0, 7]), **op)    # G_f = 48: stations [43, 50)
    assert lo[0]["station0"] == 0 and hi[0]["station0"] + hi[0]["n_stations"] == TOTAL
    assert lo[0]["in_object"] == (8 if bs == 1 else 12) and hi[0]["in_object"] == 12
    for far in (-40, 90):                                                     # an empty window: nothing is launched
        out = rig.run(e, dict(FOUR, side_anchor=[0, far, 0, 0]), **op)
        assert out[0]["blocks_stations"] == 0 and out[0]["outside_window"] == len(e) and out[0]["side_rows"] == [12, 0, 0, 12]
    # two sides, elements 1 (170 cells) and 2 (120 cells): side 2 and side 3 do not exist; cell 150 is valid for side 0
    # and lies past side 1's cells; cell 170 is past both
    two = dict(element=2, side_element=[1, 2], side_anchor=[20, 3])
    bad = an.with_sides(on.make_rows([150, 150, 170, 170, 5, 5, 119, 120], np.full(8, 0.3, np.float32), seed=6), [0, 1, 0, 1, 2, 3, 1, 1])
    good = rows_of([(0, 16, 3), (1, 0, 3)], per=4, delta=0.3, seed=7)
    rows = join(bad, good, rows_of([(255, 0, 0)], per=2, seed=8))
    info, obj, _, of_row = rig.run(rows, two, **dict(op, half_window_stations=64))
    assert info["rejected"] == 8 and info["side_rows"] == [1 + 4, 1 + 4] and np.all(of_row[[1, 2, 3, 4, 5, 7, 16, 17]] == -1)
    assert info["objects"] == 1 and (obj[0]["station_min"], obj[0]["station_max"], obj[0]["points"]) == (28, 29, 8)
    rows = join(good, rows_of([(0, 3, 1)], per=3, delta=0.0, seed=9), rows_of([(1, 3, 1)], per=1, delta=np.nan, seed=10))
    rows["y"][2] = np.inf
    info = rig.run(rows, two, **op)[0]
    assert info["rejected"] == 5 and info["side_rows"] == [3, 4]


@pytest.mark.parametrize("bs", (1, 3))
def test_one_side_is_the_element_maps_call_shifted(rig, bs):
    """Element 0: the element map's records byte for byte.  Element 1 (base 12, a multiple of bs): label shifted by
    (12 / bs) NK, the station extents by 12."""
    op = dict(block_stations=bs, block_sectors=2, min_block_points=2, min_points=4)
    rng = np.random.default_rng(bs)
    for e, base in ((0, 0), (1, 12)):
        nst = N_STATIONS[e]
        j = np.clip(np.rint(rng.normal(nst / 2, 2.5, 160)), 0, nst - 1).astype(np.int64)
        k = rng.integers(0, NSEC, 160)
        rows = on.make_rows(j * NSEC + k, (rng.choice([-1.0, 1.0], 160) * rng.uniform(0.1, 0.5, 160)).astype(np.float32), seed=e)
        anchor = nst - 2
        got = rig.run(rows, dict(element=e, side_element=[e], side_anchor=[anchor]), **op)
        want = rig.al.element(e).objects_of_rows(rows, anchor, **op)
        assert got[0]["objects"] == want[0]["objects"] >= 2
        shifted = want[1].copy()
        shifted["label"] += (base // bs) * 5
        shifted["station_min"] += base
        shifted["station_max"] += base
        assert got[1].tobytes() == shifted.tobytes() and np.array_equal(got[3], want[3])
        for q in on.CLASSES + ("flagged_pos", "flagged_neg", "components"):
            assert got[0][q] == want[0][q], q


def test_the_first_call_allocates_and_a_repeat_takes_other_parameters(gm):
    with gm.GeometricMapping() as c:
        before = int(_lib.load().gm_debug_live_buffers())
        al = c.wall_alignment(ELEMENTS, **PRM)
        created = int(_lib.load().gm_debug_live_buffers())
        with pytest.raises(_lib.GmError) as ex:
            al.check_objects(0)
        assert ex.value.status == _lib.GM_ERR_NOT_READY
        # (the element maps allocate their tables; the alignment's own object scratch does not exist yet)
        rows = rows_of([(0, 11, 2), (1, 0, 2)], per=4, seed=1)
        assert int(_lib.load().gm_debug_live_buffers()) == created > before
        one = al.objects_of_rows(rows, FOUR, min_points=8)
        assert int(_lib.load().gm_debug_live_buffers()) > created
        live = int(_lib.load().gm_debug_live_buffers())
        two = al.objects_of_rows(rows, FOUR, min_points=5, connectivity=4, block_stations=3)
        again = al.objects_of_rows(rows, FOUR, min_points=8)
        assert int(_lib.load().gm_debug_live_buffers()) == live
        assert one[0]["objects"] == 1 and two[0]["objects"] == 1 and two[1][0]["label"] != one[1][0]["label"]
        assert again[1].tobytes() == one[1].tobytes()


def _frame_with_box(A, s, n, seed, s_box, phi_box, depth, half=4.5):
    """wall_alignment_np.frame's frame (the same draws), with the points of the box chainage x angle moved `depth` toward
    the axis: (cloud, pose, the box's point indices)."""
    rng = np.random.default_rng([int(seed), 0xA11])
    P, a, u, v = al_np.axes(A, s)
    y = np.deg2rad(3.0)
    ax = np.cos(y) * a - np.sin(y) * v
    Rm = np.stack([ax, np.cross(u, ax), u], axis=1)
    tr = P - 0.2 * v - 0.1 * u
    sp = s + rng.uniform(-half, half, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rho = al_np.RADIUS + synth.wall_texture(sp, phi, seed=seed, length=200.0) + rng.normal(0.0, 0.005, n)
    box = (sp >= s_box[0]) & (sp < s_box[1]) & (phi >= phi_box[0]) & (phi < phi_box[1])
    x = A.point(sp, phi, np.where(box, rho - depth, rho))
    return ((x - tr) @ Rm).astype(np.float32), np.concatenate([Rm, tr.reshape(3, 1)], axis=1), np.flatnonzero(box)


def test_a_box_across_the_clothoid_arc_joint_is_one_object(gm):
    els, s, _ = lc.record_case("clothoid_arc:before")
    p = lc.prm()
    n_st = [e["n_stations"] for e in els]
    base = an.bases(n_st)[0]
    s_joint = al_np.spans(els)[1][1]
    op = dict(block_stations=3, block_sectors=4, min_block_points=2, min_points=8)
    ck = dict(min_count=1, threshold=0.05)
    with gm.GeometricMapping(neighborRadius=synth.fixed_k_radius(lc.N)) as c:
        al = c.wall_alignment(els, **p)
        for d in (-0.5, 0.0, 0.5):
            cloud, pose = al_np.frame(al, s + d, lc.N, seed=81)
            al.add_points(cloud, pose, outputs=False)
        al.sync()
        before = [al.element(i).read_raw().tobytes() for i in range(al.n_elements)]
        cloud, pose, box = _frame_with_box(al, s, lc.N, 81, (s_joint - 1.0, s_joint + 1.0), (0.4, 1.3), 0.3)
        c.process_frame(cloud)
        plan = al.check_frame(0, pose, **ck)
        cinfo, rows = al.check_result(0)
        assert plan["n_sides"] == 2 and plan["side_element"] == [1, 2] and base[2] % 3 != 0
        got = al.check_objects(0, rows=True, **op)
        info, obj, met, of_row = got
        print({k: info[k] for k in an.INFO_KEYS}, obj[["label", "sign", "points", "station_min", "station_max"]], len(box), len(rows))
        _same(got, an.objects(rows, n_st, p["n_sectors"], plan, **op))                       # the twin
        _same(got, al.objects_of_rows(rows, plan, **op))                                     # the stage call, the get_check rows
        again = al.check_objects(0, rows=True, **dict(op, min_points=20))                    # a repeat with other parameters
        _same(again, an.objects(rows, n_st, p["n_sectors"], plan, **dict(op, min_points=20)))
        assert info["n_rows"] == len(rows) == len(of_row) and info["rejected"] == 0
        side, cell = al.split_cell(rows)
        assert info["side_rows"] == [int((side == 0).sum()), int((side == 1).sum())] and min(info["side_rows"]) > 10
        neg = obj[obj["sign"] == -1]
        big = neg[np.argmax(neg["points"])]
        assert big["station_min"] < base[2] <= big["station_max"] and big["points"] > 0.6 * len(box)
        m = al.object_metrics(big)
        assert (m["element_from"], m["element_to"]) == (1, 2) and m["chainage_from"] < s_joint < m["chainage_to"]
        assert m["chainage_from"] > s_joint - 1.6 and m["chainage_to"] < s_joint + 1.6 and -0.35 < m["mean_m"] < -0.2
        # object_of_row agrees with check_result()'s rows: the box's rows, and no others, are the object's
        pos = int(np.flatnonzero((obj["label"] == big["label"]) & (obj["sign"] == -1))[0])
        xyz, input_row = c.cropped_cloud()
        in_box = np.isin(input_row[rows["index"]], box)
        assert np.all(in_box[of_row == pos]) and (of_row == pos).sum() == big["points"]
        assert np.all(rows["delta"][of_row == pos] < 0)
        # the per-element split gives two: each side's rows alone, on its own element map
        halves = 0
        for k, e in enumerate(plan["side_element"]):
            r = rows[side == k].copy()
            r["cell"] = cell[side == k]
            _, o, _ = on.objects(r, n_st[e], p["n_sectors"], plan["side_anchor"][k], **op)
            halves += int(((o["sign"] == -1) & (o["points"] > 0.2 * len(box))).sum())
        assert halves == 2
        assert [al.element(i).read_raw().tobytes() for i in range(al.n_elements)] == before and al.check_result(0)[1].tobytes() == rows.tobytes()


def test_one_side_slot_call_and_not_ready_after_the_element_maps_own_check(gm):
    els, s, sides = lc.record_case("arc")
    p = lc.prm()
    n_st = [e["n_stations"] for e in els]
    op = dict(block_stations=4, block_sectors=4, min_block_points=2, min_points=8)
    ck = dict(min_count=1, threshold=0.05)
    with gm.GeometricMapping(neighborRadius=synth.fixed_k_radius(lc.N)) as c:
        al = c.wall_alignment(els, **p)
        cloud, pose = al_np.frame(al, s, lc.N, seed=82)
        al.add_points(cloud, pose, outputs=False)
        cloud, pose, box = _frame_with_box(al, s, lc.N, 82, (s - 0.8, s + 0.8), (2.0, 3.0), -0.3)
        c.process_frame(cloud)
        plan = al.check_frame(0, pose, **ck)
        assert plan["n_sides"] == sides == 1
        e = plan["element"]
        base = an.bases(n_st)[0][e]
        assert e > 0 and base % 4 == 0
        got = al.check_objects(0, rows=True, **op)
        _, rows = al.check_result(0)
        _same(got, an.objects(rows, n_st, p["n_sectors"], plan, **op))
        _same(got, al.objects_of_rows(rows, plan, **op))
        want = al.element(e).check_objects(0, rows=True, **op)      # the element map's own call on the same staged rows
        shifted = want[1].copy()
        shifted["label"] += (base // 4) * want[0]["blocks_sectors"]
        shifted["station_min"] += base
        shifted["station_max"] += base
        assert got[0]["objects"] == want[0]["objects"] >= 1 and got[1].tobytes() == shifted.tobytes() and np.array_equal(got[3], want[3])
        assert got[0]["side_rows"] == [len(rows)] and got[1]["sign"].max() == 1
        al.element(e).check_frame(0, pose, **ck)                     # replaces the rows the alignment's check staged there
        with pytest.raises(_lib.GmError) as ex:
            al.check_objects(0, **op)
        assert ex.value.status == _lib.GM_ERR_NOT_READY
        al.check_frame(0, pose, **ck)
        _same(al.check_objects(0, rows=True, **op), got)
