"""GPU tests of the check's objects (gm_wall_map_check_objects / gm_wall_check_objects, csrc/k_wall_objects.hip +
gm_wall_slot.hip): crafted rows through the stage call at every row count, grid, shape, threshold, window and tie edge, byte
for byte against the integer twin (tests/wall_objects_np.py: info, records, object_of_row); independence of the tile shape
and of the row order; the slot call against the stage call over every pipeline path; analytic truth of a drive with
world-fixed patches; the results' lifetime and the refusals."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_np as wn  # noqa: E402
import wall_objects_np as on  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _same(got, want):
    ginfo, gobj, gmet, grow = got
    winfo, wobj, wrow = want
    for k in on.INFO_KEYS:
        assert ginfo[k] == winfo[k], (k, ginfo[k], winfo[k])
    assert sum(ginfo[k] for k in on.CLASSES) == ginfo["n_rows"]
    assert len(gobj) == len(wobj)
    for i in range(len(wobj)):
        assert gobj[i].tobytes() == wobj[i].tobytes(), (i, gobj[i], wobj[i])
    assert np.array_equal(grow, wrow)


def _run(m, rows, anchor, **op):
    """The stage call against the twin; returns the call's result."""
    got = m.objects_of_rows(rows, anchor, **op)
    _same(got, on.objects(rows, m.n_stations, m.n_sectors, anchor, **op))
    return got


def _blocks_to_rows(blocks, ns, bs=1, bk=1, per=1, delta=0.25, seed=0):
    """`per` rows in each block (J, K) of the list: the block's first cell, deltas of one sign with varying magnitude."""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.array([J * bs * ns + K * bk for J, K in blocks], np.int64), per)
    d = (delta * rng.uniform(0.5, 1.5, len(cell))).astype(np.float32)
    return on.make_rows(cell, d, seed=seed + 1)


def _clusters(rng, n, n_stations, ns, j_lo, j_hi):
    """n random rows: clusters of both signs around random cells (wrapping in k), some uniform noise, a few rows outside
    [j_lo, j_hi) and a few that the rule rejects."""
    centres = [(rng.integers(j_lo, j_hi), rng.integers(0, ns), rng.choice([-1.0, 1.0])) for _ in range(max(2, n // 40))]
    which = rng.integers(0, len(centres), n)
    j = np.array([centres[w][0] for w in which]) + np.rint(rng.normal(0, 2.0, n)).astype(np.int64)
    k = (np.array([centres[w][1] for w in which]) + np.rint(rng.normal(0, 3.0, n)).astype(np.int64)) % ns
    sign = np.array([centres[w][2] for w in which])
    noise = rng.random(n) < 0.15
    j = np.where(noise, rng.integers(0, n_stations, n), np.clip(j, 0, n_stations - 1))
    k = np.where(noise, rng.integers(0, ns, n), k)
    delta = (sign * rng.uniform(0.06, 0.6, n)).astype(np.float32)
    rows = on.make_rows(j * ns + k, delta, index=rng.permutation(n), seed=int(rng.integers(1 << 30)))
    bad = np.flatnonzero(rng.random(n) < 0.03)
    for t, i in enumerate(bad):
        if t % 5 == 0:
            rows["cell"][i] = -1
        elif t % 5 == 1:
            rows["cell"][i] = n_stations * ns
        elif t % 5 == 2:
            rows["delta"][i] = 0.0
        elif t % 5 == 3:
            rows["delta"][i] = np.nan
        else:
            rows["x"][i] = np.inf
    return rows


GRIDS = {
    "90x1": dict(n_stations=400, n_sectors=90, bk=1),
    "90x7": dict(n_stations=400, n_sectors=90, bk=7),        # a ragged last block, NK = 13
    "4096x1": dict(n_stations=400, n_sectors=4096, bk=1),    # several tiles across K plus the wrap seam
}
ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_row_counts_and_grids(gm, grid):
    g = GRIDS[grid]
    ns, nst = g["n_sectors"], g["n_stations"]
    rng = np.random.default_rng(len(grid) + ns)
    objects = 0
    with gm.GeometricMapping() as c:
        m = c.wall_map(n_stations=nst, n_sectors=ns)
        for n in ROW_COUNTS:
            rows = _clusters(rng, n, nst, ns, 60, 340)            # the window of anchor 200 is stations 72 .. 327
            for op in (dict(), dict(min_block_points=1, min_points=3, connectivity=4, block_stations=2)):
                got = _run(m, rows, 200, block_sectors=g["bk"], **op)
                objects += got[0]["objects"]
                print(grid, n, op, {k: got[0][k] for k in on.INFO_KEYS})
        assert objects > 10


def test_shapes(gm):
    one = dict(min_block_points=1, min_points=1)
    with gm.GeometricMapping() as c:
        m = c.wall_map(n_stations=400, n_sectors=90)
        # a window longer than one tile in J: one column of blocks over 200 stations
        info, obj, met, _ = _run(m, _blocks_to_rows([(J, 10) for J in range(80, 280)], 90), 200, **one)
        assert info["objects"] == 1 and obj[0]["blocks"] == 200 and (obj[0]["station_min"], obj[0]["station_max"]) == (80, 279)
        assert info["blocks_stations"] == 256 > _lib.GM_WALL_OBJECT_TILE[0]
        # a ring over every sector, with 7-sector blocks too
        for bk in (1, 7):
            rows = on.make_rows(150 * 90 + np.arange(90), np.full(90, -0.3, np.float32))
            info, obj, met, _ = _run(m, rows, 200, block_sectors=bk, **one)
            assert info["objects"] == 1 and obj[0]["sign"] == -1 and obj[0]["blocks"] == -(-90 // bk)
            assert (obj[0]["sector_min"], obj[0]["sector_max"], obj[0]["sector_min_turned"], obj[0]["sector_max_turned"]) == (0, 89, 0, 89)
            assert (met[0]["angle_from_deg"], met[0]["angle_to_deg"]) == (0.0, 360.0)
        # two blocks joined only diagonally across the seam: one object at connectivity 8, two at 4
        rows = _blocks_to_rows([(100, 89), (101, 0)], 90, per=3)
        info, obj, met, of_row = _run(m, rows, 200, connectivity=8, min_points=1)
        assert info["objects"] == 1 and obj[0]["label"] == 100 * 90 + 89 and set(of_row) == {0}
        assert (met[0]["angle_from_deg"], met[0]["angle_to_deg"]) == (356.0, 4.0)                  # across 0
        info, obj, _, of_row = _run(m, rows, 200, connectivity=4, min_points=1)
        assert info["objects"] == 2 and of_row.tolist() == [0, 0, 0, 1, 1, 1]
        # positive and negative rows in the same blocks: two objects of one label, the negative one first
        blocks = [(120, 5), (120, 6), (121, 6)]
        rows = np.concatenate([_blocks_to_rows(blocks, 90, per=4, delta=0.2, seed=3), _blocks_to_rows(blocks, 90, per=3, delta=-0.2, seed=4)])
        rows["index"] = np.arange(len(rows))
        info, obj, _, of_row = _run(m, rows, 200)
        assert info["objects"] == 2 and obj["label"].tolist() == [120 * 90 + 5] * 2 and obj["sign"].tolist() == [-1, 1]
        assert obj["points"].tolist() == [9, 12] and of_row.tolist() == [1] * 12 + [0] * 9
    with gm.GeometricMapping() as c:
        # a spiral over many tiles of a 4096-sector grid, winding through the seam: one object
        m = c.wall_map(n_stations=400, n_sectors=4096)
        blocks = []
        for turn in range(12):
            J = 100 + 4 * turn
            ks = [(3500 + t) % 4096 for t in range(1200)]           # sectors 3500 .. 4095, 0 .. 603: through the seam
            blocks += [(J, K) for K in ks]
            end = ks[-1] if turn % 2 == 0 else ks[0]
            if turn < 11:
                blocks += [(J + d, end) for d in (1, 2, 3)]
        rows = _blocks_to_rows(blocks, 4096, seed=9)
        rng = np.random.default_rng(5)
        rows = rows[rng.permutation(len(rows))]
        info, obj, met, _ = _run(m, rows, 200, **one)
        assert info["objects"] == 1 and obj[0]["blocks"] == len(blocks) and obj[0]["label"] == 100 * 4096
        assert obj[0]["sector_max_turned"] - obj[0]["sector_min_turned"] == 1199 and obj[0]["sector_max"] - obj[0]["sector_min"] == 4095


def test_threshold_edges(gm):
    with gm.GeometricMapping() as c:
        m = c.wall_map(n_stations=400, n_sectors=90)
        # cnt = min_block_points - 1 and exactly min_block_points: the middle block of a row of three splits it or not
        for mid, want in ((2, 2), (3, 1)):
            cell = np.repeat(np.array([150 * 90 + 20, 150 * 90 + 21, 150 * 90 + 22]), [4, mid, 4])
            info, obj, _, _ = _run(m, on.make_rows(cell, np.full(len(cell), 0.2, np.float32)), 200, min_block_points=3, min_points=4)
            assert info["objects"] == want and info["sparse"] == (2 if mid == 2 else 0)
        # points = min_points - 1 and exactly min_points
        for pts, want in ((7, 0), (8, 1)):
            cell = np.repeat(np.array([160 * 90 + 3, 160 * 90 + 4]), [4, pts - 4])
            info, obj, _, of_row = _run(m, on.make_rows(cell, np.full(pts, -0.2, np.float32)), 200)
            assert info["objects"] == want and info["components"] == 1 and info["small"] == (pts if not want else 0)
            assert set(of_row) == ({0} if want else {-1})
        # the same edges on the positive and the negative plane of one block at once
        cell = np.full(5, 170 * 90 + 40)
        rows = on.make_rows(cell, np.float32([0.2, 0.2, -0.2, 0.2, -0.2]))
        info, obj, _, of_row = _run(m, rows, 200, min_block_points=3, min_points=3)
        assert info["objects"] == 1 and obj[0]["sign"] == 1 and info["sparse"] == 2 and of_row.tolist() == [0, 0, -1, 0, -1]


@pytest.mark.parametrize("bs", (1, 3))
def test_window_edges(gm, bs):
    nst, ns, H, jf = 400, 90, 50, 200
    with gm.GeometricMapping() as c:
        m = c.wall_map(n_stations=nst, n_sectors=ns)
        stations = [jf - H - 1, jf - H, jf + H - 1, jf + H] + ([jf - H - 2, jf - H - 3, jf + H + 1, jf + H + 2] if bs == 3 else [])
        cell = np.repeat(np.array(stations) * ns + 7, 8)
        rows = on.make_rows(cell, np.full(len(cell), 0.3, np.float32))
        info, obj, _, of_row = _run(m, rows, jf, block_stations=bs, half_window_stations=H)
        J0, J1 = (jf - H) // bs, (jf + H - 1) // bs
        inside = [J0 <= s // bs <= J1 for s in stations]
        assert (info["station0"], info["n_stations"], info["blocks_stations"]) == (J0 * bs, (J1 + 1) * bs - J0 * bs, J1 - J0 + 1)
        assert info["outside_window"] == 8 * inside.count(False) and (of_row.reshape(-1, 8)[:, 0] >= 0).tolist() == inside
        if bs == 1:
            assert inside == [False, True, True, False]
        else:
            assert inside == [False, True, True, True, False, False, True, False]   # whole block rows: stations 150 .. 251
        # anchors at the map's ends and far away
        ends = on.make_rows(np.repeat(np.array([0, H - 1, H, nst - H - 1, nst - H, nst - 1]) * ns + 11, 8), np.full(48, -0.3, np.float32))
        info, _, _, of_row = _run(m, ends, 0, half_window_stations=H)
        assert (info["station0"], info["n_stations"]) == (0, H) and (of_row.reshape(-1, 8)[:, 0] >= 0).tolist() == [True, True] + [False] * 4
        info, _, _, of_row = _run(m, ends, nst - 1, block_stations=bs, half_window_stations=H)
        assert info["station0"] + info["n_stations"] == nst and (of_row.reshape(-1, 8)[:, 0] >= 0).tolist()[-2:] == [True, True]
        bad = ends.copy()
        bad["delta"][:3] = 0.0
        for far in (10 ** 9, -10 ** 9, nst + H, -H):
            info, obj, _, of_row = _run(m, bad, far, block_stations=bs, half_window_stations=H)
            assert info["blocks_stations"] == 0 and info["outside_window"] == 45 and info["rejected"] == 3 and len(obj) == 0
            assert np.all(of_row == -1)


def test_peak_ties_and_rejections(gm):
    with gm.GeometricMapping() as c:
        m = c.wall_map(n_stations=400, n_sectors=90)
        # equal |dq| at two indices (the smaller index wins, wherever it stands) and at opposite signs (two objects)
        cell = np.full(16, 150 * 90 + 30)
        d = np.float32([0.5, 0.25, 0.5, 0.125, 0.25, 0.5, 0.125, 0.25] + [-0.5, -0.25, -0.5, -0.125, -0.25, -0.5, -0.125, -0.25])
        rows = on.make_rows(cell, d, index=[9, 1, 4, 2, 3, 7, 5, 6, 19, 11, 14, 12, 13, 17, 15, 16])
        info, obj, met, _ = _run(m, rows, 200)
        assert obj["sign"].tolist() == [-1, 1] and obj["peak"].tolist() == [-(1 << 19), 1 << 19] and obj["peak_index"].tolist() == [14, 4]
        assert [x["peak_m"] for x in met] == [-0.5, 0.5]
        # every way to be rejected, among rows that form one object
        rows = on.make_rows(np.full(14, 151 * 90 + 31), np.full(14, 0.2, np.float32))
        rows["cell"][0] = -1
        rows["cell"][1] = 400 * 90
        rows["delta"][2] = 0.0
        rows["delta"][3] = np.nan
        rows["x"][4] = np.inf
        rows["delta"][5] = 2.0 ** -22                                # rounds to dq = 0
        info, obj, _, of_row = _run(m, rows, 200)
        assert info["rejected"] == 6 and info["in_object"] == 8 and of_row.tolist() == [-1] * 6 + [0] * 8
        for f, v in (("y", -np.inf), ("z", np.nan), ("e", np.inf)):
            r2 = rows.copy()
            r2[f][13] = v
            info, obj, _, of_row = _run(m, r2, 200)
            assert info["rejected"] == 7 and info["small"] == 7 and len(obj) == 0
        # saturation: a delta beyond the int32 range of 2^-20 m
        rows = on.make_rows(np.full(8, 152 * 90 + 32), np.float32([3000.0] * 4 + [-3000.0] * 4))
        info, obj, _, _ = _run(m, rows, 200, min_points=4)
        assert obj["peak"].tolist() == [-(1 << 31), (1 << 31) - 1]


INDEP = {"90": dict(n_stations=400, n_sectors=90, n=3000), "4096": dict(n_stations=300, n_sectors=4096, n=6000)}


@pytest.mark.parametrize("grid", sorted(INDEP))
def test_independent_of_tile_and_row_order(gm, grid):
    g = INDEP[grid]
    rng = np.random.default_rng(77)
    rows = _clusters(rng, g["n"], g["n_stations"], g["n_sectors"], 30, 270)
    # plus a long snake so that components cross many tiles
    snake = _blocks_to_rows([(40 + J, (80 + 3 * J) % g["n_sectors"]) for J in range(200)] + [(40 + J, (81 + 3 * J) % g["n_sectors"]) for J in range(200)]
                            + [(40 + J, (82 + 3 * J) % g["n_sectors"]) for J in range(200)], g["n_sectors"], per=2, seed=2)
    snake["index"] += 100000
    rows = np.concatenate([rows, snake])
    op = dict(min_block_points=2, min_points=6)
    want = on.objects(rows, g["n_stations"], g["n_sectors"], 150, **op)
    assert want[0]["objects"] > 3 and want[0]["components"] > want[0]["objects"]
    perm = rng.permutation(len(rows))
    for shape in (None, "64x64", "1x4096", "4096x1", "3x5"):
        with tile(shape), gm.GeometricMapping() as c:
            m = c.wall_map(n_stations=g["n_stations"], n_sectors=g["n_sectors"])
            got = m.objects_of_rows(rows, 150, **op)
            _same(got, want)
            shuffled = m.objects_of_rows(rows[perm], 150, **op)
            _same(shuffled[:3] + (None,), want[:2] + (None,))
            assert np.array_equal(shuffled[3], want[2][perm])


# ---- the slot call ----

N_FRAME = 30_000
CK = dict(threshold=0.08, min_count=4)
OP = dict(block_stations=2, block_sectors=2)
PATCHES = ((10.0, 12.0, 20.0, 44.0, 0.15), (25.0, 27.0, 316.0, 340.0, -0.5))


def _map_state(m):
    i = m.info()
    return m.read_raw().tobytes(), tuple(i[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))


def test_slot_call_equals_stage_call(gm):
    survey = synth.tunnel_drive(6, N_FRAME, seed=31, patches=())
    drive = synth.tunnel_drive(6, N_FRAME, seed=31, patches=PATCHES)
    p = wn.params(n_stations=192, **drive["design"])
    kw = dict(neighborRadius=synth.fixed_k_radius(N_FRAME))
    clouds, poses = [f[0] for f in drive["frames"]], [f[1] for f in drive["frames"]]
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        baseline = m.read_raw()

    def stage(m, slot, anchor):
        """The slot call, twice with different parameters, against the stage call on the check's own rows."""
        before = _map_state(m)
        info, rec = m.check_result(slot)
        for op in (OP, dict(min_points=3)):
            got = m.check_objects(slot, rows=True, **op)
            assert got[0]["n_rows"] == len(rec) and got[0]["rejected"] == 0
            want = m.objects_of_rows(rec, anchor, **op)
            _same(got, (want[0], want[1], want[3]))
            _same(got, on.objects(rec, m.n_stations, m.n_sectors, anchor, **op))
            assert m.check_objects(slot, **op)[1].tobytes() == got[1].tobytes()          # without object_of_row
        info2, rec2 = m.check_result(slot)
        assert info2 == info and rec2.tobytes() == rec.tobytes() and _map_state(m) == before
        return m.check_objects(slot, **OP)[0]["objects"]

    for flags in (_lib.GM_CFG_DEFAULT, _lib.GM_CFG_DEFAULT | _lib.GM_CFG_GRAPH):
        objects = 0
        with gm.GeometricMapping(flags=flags, **kw) as c:
            m = c.wall_map(**p)
            m.add_raw(baseline)
            for k in range(3):
                c.process_frame(clouds[k])
                add = m.check_frame(0, poses[k], **CK)
                objects += stage(m, 0, add["anchor_station"])
        assert objects >= 1
    # four slots, no synchronisation between the submits: each slot's objects are those of its own check
    with gm.GeometricMapping(n_slots=4, **kw) as c:
        m = c.wall_map(**p)
        m.add_raw(baseline)
        anchors = []
        for k in range(4):
            c.submit_frame(k, clouds[k])
            anchors.append(m.check_frame(k, poses[k], **CK)["anchor_station"])
        objects = sum(stage(m, k, anchors[k]) for k in (2, 0, 3, 1))
        assert objects >= 2


TRUTH_PATCHES = PATCHES + ((14.0, 15.0, 100.0, 140.0, 0.15), (11.0, 12.5, 200.0, 224.0, -0.5))
TRUTH_CK = dict(threshold=0.04, min_count=4)      # 4 sigma of the frame's noise: a few stray changed rows per frame


def test_analytic_truth(gm):
    """World-fixed patches of +0.15 m and -0.5 m (things standing in the profile, inside the check's default 1 m gate),
    two of each, against a survey of the bare wall, 2 x 2-cell blocks, a threshold low enough for stray changed rows: in
    every frame every object has its patch's sign and station and sector extents inside that patch, and every patch wholly
    within the frame's reach gives exactly one object -- with up to three patches and the speckle in one frame.  Through
    the CPU twins alone (wall_np.points, wall_check_np.check, wall_objects_np.objects) seed 21 gives 384, 530, 471, 466,
    354, 192, 228, 212 changed rows in the eight frames, 2, 3, 3, 3, 2, 1, 1, 1 objects and 1, 1, 1, 0, 0, 2, 1, 0 sparse
    rows (no small one): the stray rows never make an object."""
    PATCHES, CK = TRUTH_PATCHES, TRUTH_CK
    survey = synth.tunnel_drive(8, 20_000, seed=21, patches=())
    drive = synth.tunnel_drive(8, 20_000, seed=21, patches=PATCHES)
    p = wn.params(n_stations=192, **drive["design"])
    seen = []
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in survey["frames"]:
            m.add_points(cloud, pose, outputs=False)
        for i, (cloud, pose) in enumerate(drive["frames"]):
            info, rec, _ = m.check_points(cloud, pose, outputs=False, **CK)
            oinfo, obj, met, of_row = m.check_objects(0, rows=True, **OP)
            _same((oinfo, obj, met, of_row), on.objects(rec, m.n_stations, m.n_sectors, info["add"]["anchor_station"], **OP))
            s = 6.0 + 3.5 * i                                                    # tunnel_drive: start + i step, reach 7
            per = [0] * len(PATCHES)
            for o in obj:
                hit = None
                for k, (t0, t1, a0, a1, dr) in enumerate(PATCHES):
                    j0, j1, k0, k1 = round(t0 / 0.25), round(t1 / 0.25) - 1, round(a0 / 4.0), round(a1 / 4.0) - 1
                    if ((o["sign"] > 0) == (dr > 0) and j0 <= o["station_min"] and o["station_max"] <= j1 and k0 <= o["sector_min"]
                            and o["sector_max"] <= k1):
                        hit = k
                assert hit is not None, (i, o)
                per[hit] += 1
            for k, (t0, t1, _a0, _a1, _dr) in enumerate(PATCHES):
                if t0 >= s - 7.0 and t1 <= s + 7.0:
                    assert per[k] == 1, (i, k, per)
            seen.append((len(rec), oinfo["objects"], oinfo["sparse"], oinfo["small"]))
            for o, x in zip(obj, met):                                           # the metrics speak of the patch
                assert abs(x["mean_m"] - PATCHES[0 if o["sign"] > 0 else 1][4]) < 0.02
    print("analytic truth:", seen)
    assert sum(s_[1] for s_ in seen) == 16 and max(s_[1] for s_ in seen) == 3


def test_lifetime_and_refusals(gm):
    drive = synth.tunnel_drive(2, 5_000, seed=2)
    (cloud, pose), (cloud1, pose1) = drive["frames"]
    p = wn.params(n_stations=80, **drive["design"])
    L = _lib.load()
    info, got = _lib.WallObjectsInfo(), C.c_uint32(7)
    buf = np.zeros(4096, api.WALL_OBJECT)
    bp = buf.ctypes.data_as(C.POINTER(_lib.WallObject))
    bad, cap = _lib.GM_ERR_INVALID_ARG, _lib.GM_ERR_CAPACITY
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(5_000)) as c:
        m = c.wall_map(**p)
        m.add_points(cloud, pose, outputs=False)
        ok = api.WallMap.object_params()
        # before any check; a slot out of range; NULL info
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 0) == _lib.GM_ERR_NOT_READY
        assert got.value == 0
        assert L.gm_wall_map_check_objects(m._map, 7, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 0) == bad
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(ok), None, None, 0, C.byref(got), None, 0) == bad
        c.process_frame(cloud1)
        m.check_frame(0, pose1, threshold=0.03, min_count=1)
        assert L.gm_wall_map_check_objects(m._map, 1, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 0) == _lib.GM_ERR_NOT_READY
        # each parameter outside its limits, on both calls
        rows = on.make_rows(np.full(9, 40 * 90 + 3), np.full(9, 0.2, np.float32))
        rp = rows.ctypes.data_as(C.POINTER(_lib.WallCheckPoint))
        for k, v in (("struct_size", 28), ("block_stations", 0), ("block_sectors", 0), ("min_block_points", 0), ("min_points", 0),
                     ("connectivity", 6), ("connectivity", 0), ("half_window_stations", 0), ("half_window_stations", (1 << 20) + 1)):
            q = api.WallMap.object_params()
            setattr(q, k, v)
            assert L.gm_wall_map_check_objects(m._map, 0, C.byref(q), C.byref(info), None, 0, C.byref(got), None, 0) == bad, (k, v)
            assert L.gm_wall_check_objects(m._map, rp, 9, 40, C.byref(q), C.byref(info), None, 0, C.byref(got), None) == bad, (k, v)
        assert L.gm_wall_check_objects(m._map, None, 9, 40, C.byref(ok), C.byref(info), None, 0, C.byref(got), None) == bad
        assert L.gm_wall_check_objects(m._map, rp, 9, 40, C.byref(ok), C.byref(info), None, 3, C.byref(got), None) == bad
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 5) == bad
        # a count query; a short capacity writes no record; then the list
        q = api.WallMap.object_params(min_points=2, min_block_points=1)
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(q), C.byref(info), None, 0, C.byref(got), None, 0) == _lib.GM_OK
        n1 = got.value
        assert 1 < n1 <= 4096 and info.objects == n1 and info.struct_size == C.sizeof(_lib.WallObjectsInfo) and info.reserved == 0
        assert info.rejected + info.outside_window + info.sparse + info.small + info.in_object == info.n_rows > 0
        got.value = 0
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(q), C.byref(info), bp, n1 - 1, C.byref(got), None, 0) == cap
        assert got.value == n1 and info.objects == n1 and buf.tobytes() == bytes(buf.nbytes)
        of_row = np.full(info.n_rows, 7, np.int32)
        op_ = of_row.ctypes.data_as(C.POINTER(C.c_int32))
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(q), C.byref(info), bp, n1, C.byref(got), op_, info.n_rows - 1) == cap
        assert np.all(of_row == 7)
        assert L.gm_wall_map_check_objects(m._map, 0, C.byref(q), C.byref(info), bp, n1, C.byref(got), op_, info.n_rows) == _lib.GM_OK
        assert np.all(np.diff(buf["label"][:n1].astype(np.int64) * 2 + (buf["sign"][:n1] > 0)) > 0) and of_row.max() == n1 - 1
        # the stage call: count query and short capacity
        assert L.gm_wall_check_objects(m._map, rp, 9, 40, C.byref(ok), C.byref(info), None, 0, C.byref(got), None) == _lib.GM_OK
        assert got.value == 1
        buf[:] = 0
        two = np.concatenate([rows, on.make_rows(np.full(9, 50 * 90 + 3), np.full(9, 0.2, np.float32))])
        tp = two.ctypes.data_as(C.POINTER(_lib.WallCheckPoint))
        assert L.gm_wall_check_objects(m._map, tp, 18, 40, C.byref(ok), C.byref(info), bp, 1, C.byref(got), None) == cap
        assert got.value == 2 and buf.tobytes() == bytes(buf.nbytes)
        # a window above 2^20 blocks (a check on a 4096-sector map, 1-cell blocks, H = 129)
        big = c.wall_map(n_stations=400, n_sectors=4096)
        q = api.WallMap.object_params(half_window_stations=129)
        assert L.gm_wall_check_objects(big._map, rp, 9, 200, C.byref(q), C.byref(info), None, 0, C.byref(got), None) == bad
        q2 = api.WallMap.object_params(half_window_stations=129, block_sectors=2)
        assert L.gm_wall_check_objects(big._map, rp, 9, 200, C.byref(q2), C.byref(info), None, 0, C.byref(got), None) == _lib.GM_OK
        # the same refusal from the slot call: a check on that map whose anchor lies 200 stations in
        ahead = pose1.copy()
        ahead[0, 3] = 200 * 0.25 + 0.1
        add = big.check_points(cloud1[:100], ahead, outputs=False)[0]["add"]
        assert add["anchor_station"] == 200
        assert L.gm_wall_map_check_objects(big._map, 0, C.byref(q), C.byref(info), None, 0, C.byref(got), None, 0) == bad
        assert L.gm_wall_map_check_objects(big._map, 0, C.byref(q2), C.byref(info), None, 0, C.byref(got), None, 0) == _lib.GM_OK
        assert (info.blocks_stations, info.blocks_sectors) == (258, 2048)
        c.process_frame(cloud1)                                      # (the stage call took slot 0's frame)
        # a frame without changed points; a map closed with objects asked for
        m.check_frame(0, pose1, threshold=8.0, gate=8.0)
        oi, obj, _, of_row = m.check_objects(0, rows=True)
        assert oi["n_rows"] == 0 and len(obj) == 0 and len(of_row) == 0
        m.close()
