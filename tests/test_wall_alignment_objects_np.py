"""The twin of gm_wall_alignment_check_objects (tests/wall_alignment_objects_np.py) against a brute-force reading of the
rule on random small alignments, and its teeth: three deliberately wrong variants of the twin, each of which must change
the result on a case built for it.  No library, no GPU."""
import numpy as np
import pytest

import wall_alignment_objects_np as an
import wall_check_np as kn
import wall_objects_np as on


def brute(rows, n_stations, n_sectors, plan, p):
    """(object_of_row, [(label, sign, points, station_min, station_max)]) by the rule read directly: the global station of
    every row, the flagged (plane, J, K), their adjacency matrix and its closure by repeated squaring."""
    base, total = an.bases(n_stations)
    se = [int(x) for x in plan["side_element"]]
    bs, bk, H = p["block_stations"], p["block_sectors"], p["half_window_stations"]
    NK = -(-n_sectors // bk)
    home = int(plan["element"]) - se[0]
    Gf = base[se[home]] + int(plan["side_anchor"][home])
    lo, hi = max(0, Gf - H), min(total, Gf + H)
    J0, J1 = (lo // bs, (hi - 1) // bs) if lo < hi else (0, -1)
    dq = kn.fix(rows["delta"])
    live = []
    for i, r in enumerate(rows):
        c = int(np.uint32(r["cell"]))
        side, cell = c >> 24, c & 0xFFFFFF
        if side >= len(se) or cell >= n_stations[se[side]] * n_sectors or dq[i] == 0:
            continue
        if not all(np.isfinite(r[f]) for f in ("x", "y", "z", "e")):
            continue
        G, k = base[se[side]] + cell // n_sectors, cell % n_sectors
        if J0 <= G // bs <= J1:
            live.append((i, int(dq[i] > 0), G // bs, k // bk, G))
    count = {}
    for _, pl, J, K, _ in live:
        count[(pl, J, K)] = count.get((pl, J, K), 0) + 1
    nodes = sorted(b for b, c in count.items() if c >= p["min_block_points"])
    at = {b: q for q, b in enumerate(nodes)}
    A = np.eye(len(nodes), dtype=bool)
    for (pl, J, K), q in at.items():
        for dj in (-1, 0, 1):
            for dk in (-1, 0, 1):
                if (dj or dk) and (p["connectivity"] == 8 or not (dj and dk)):
                    nb = (pl, J + dj, (K + dk) % NK)
                    if J0 <= J + dj <= J1 and nb in at:
                        A[q, at[nb]] = True
    for _ in range(max(len(nodes), 1).bit_length()):
        A = (A.astype(np.int64) @ A.astype(np.int64)) > 0
    comp = {}
    for q in range(len(nodes)):
        comp.setdefault(int(np.flatnonzero(A[q])[0]), []).append(nodes[q])
    found = []
    for blocks in comp.values():
        mine = [(i, G) for i, pl, J, K, G in live if (pl, J, K) in set(blocks)]
        if len(mine) >= p["min_points"]:
            found.append((min(J * NK + K for _, J, K in blocks), 1 if blocks[0][0] else -1, len(mine),
                          min(G for _, G in mine), max(G for _, G in mine), [i for i, _ in mine]))
    found.sort(key=lambda t: (t[0], t[1]))
    of_row = np.full(len(rows), -1, np.int32)
    for pos, t in enumerate(found):
        of_row[t[5]] = pos
    return of_row, [t[:5] for t in found]


def random_case(seed):
    rng = np.random.default_rng(seed)
    ne = int(rng.integers(1, 6))
    n_stations = [int(x) for x in rng.integers(1, 9, ne)]
    n_sectors = int(rng.integers(3, 9))
    ns = int(rng.integers(1, min(ne, 4) + 1))
    first = int(rng.integers(0, ne - ns + 1))
    se = list(range(first, first + ns))
    plan = dict(element=int(rng.choice(se)), side_element=se, side_anchor=[int(x) for x in rng.integers(-3, 12, ns)])
    n = 120
    side = rng.integers(0, ns + 1, n)   # (a side == n_sides now and then)
    cell = np.array([rng.integers(0, n_stations[se[min(s, ns - 1)]] * n_sectors + 2) for s in side])
    rows = an.with_sides(on.make_rows(cell, rng.choice([-0.5, -0.25, 0.0, 0.25, 0.5], n, p=[0.3, 0.15, 0.05, 0.2, 0.3]), seed=seed), side)
    rows["x"][rng.integers(0, n)] = np.inf
    p = dict(on.DEFAULTS, block_stations=int(rng.integers(1, 4)), block_sectors=int(rng.integers(1, 3)), min_block_points=int(rng.integers(1, 3)),
             min_points=int(rng.integers(1, 6)), connectivity=int(rng.choice([4, 8])), half_window_stations=int(rng.integers(2, 20)))
    return rows, n_stations, n_sectors, plan, p


@pytest.mark.parametrize("seed", range(40))
def test_twin_equals_the_brute_force_reading(seed):
    rows, n_stations, n_sectors, plan, p = random_case(seed)
    info, obj, of_row = an.objects(rows, n_stations, n_sectors, plan, **p)
    want_rows, want = brute(rows, n_stations, n_sectors, plan, p)
    assert np.array_equal(of_row, want_rows)
    assert [(int(o["label"]), int(o["sign"]), int(o["points"]), int(o["station_min"]), int(o["station_max"])) for o in obj] == want
    assert sum(info[c] for c in on.CLASSES) == len(rows)
    assert sum(info["side_rows"]) == len(rows) - info["rejected"]


def test_some_random_case_has_an_object_across_a_joint():
    hits = 0
    for seed in range(40):
        rows, n_stations, n_sectors, plan, p = random_case(seed)
        _, obj, _ = an.objects(rows, n_stations, n_sectors, plan, **p)
        edges = an.bases(n_stations)[0][1:]
        hits += sum(1 for o in obj for b in edges if o["station_min"] < b <= o["station_max"])
    assert hits >= 5


# ---- teeth ----

N_STATIONS, NSEC = [5, 7, 5], 6   # bases 0, 5, 12: neither joint on a block border for bs = 3
PLAN = dict(element=1, side_element=[0, 1, 2], side_anchor=[8, 3, -4])
P = dict(block_stations=3, block_sectors=2, min_block_points=2, min_points=4, connectivity=4, half_window_stations=64)


def _rows(side_station_sector, delta=-0.5):
    side = [s for s, _, _ in side_station_sector]
    cell = [j * NSEC + k for _, j, k in side_station_sector]
    return an.with_sides(on.make_rows(cell, np.full(len(cell), delta, np.float32), seed=3), side)


def _differs(rows, variant):
    good, bad = an.objects(rows, N_STATIONS, NSEC, PLAN, **P), an.objects(rows, N_STATIONS, NSEC, PLAN, variant=variant, **P)
    return not (np.array_equal(good[1], bad[1]) and np.array_equal(good[2], bad[2]) and
                all(good[0][k] == bad[0][k] for k in on.CLASSES))


def test_blocks_anchored_per_element_change_the_result():
    """Global stations 4 (element 0) and 5 (element 1) share the block J = 1; anchored per element they fall into two
    blocks of one row each, neither of which is flagged."""
    rows = _rows([(0, 4, 0), (1, 0, 0), (0, 4, 1), (1, 0, 1)])
    info, obj, _ = an.objects(rows, N_STATIONS, NSEC, PLAN, **dict(P, min_block_points=4))
    assert info["objects"] == 1 and obj["blocks"][0] == 1 and (obj["station_min"][0], obj["station_max"][0]) == (4, 5)
    good = an.objects(rows, N_STATIONS, NSEC, PLAN, **dict(P, min_block_points=4))
    bad = an.objects(rows, N_STATIONS, NSEC, PLAN, variant="per_element_blocks", **dict(P, min_block_points=4))
    assert bad[0]["objects"] == 0 and good[0]["objects"] == 1


def test_a_joint_left_open_changes_the_result():
    """Two rows on either side of the joint at global station 12, in the neighbouring blocks J = 3 and J = 4: one object of
    four rows; with the joint open two components of two, both below min_points."""
    rows = _rows([(1, 6, 0), (1, 6, 1), (2, 0, 0), (2, 0, 1)])
    info, obj, of_row = an.objects(rows, N_STATIONS, NSEC, PLAN, **P)
    assert info["objects"] == 1 and obj["points"][0] == 4 and obj["station_min"][0] < 12 <= obj["station_max"][0]
    assert _differs(rows, "open_joint")
    assert an.objects(rows, N_STATIONS, NSEC, PLAN, variant="open_joint", **P)[0]["objects"] == 0


def test_a_cell_limit_taken_from_side_0_changes_the_result():
    """Stations 5 and 6 of element 1 exist (7 stations) but lie past side 0's 5 x 6 cells."""
    rows = _rows([(1, 5, 0), (1, 5, 1), (1, 6, 0), (1, 6, 1)])
    info, obj, _ = an.objects(rows, N_STATIONS, NSEC, PLAN, **P)
    assert info["rejected"] == 0 and info["objects"] == 1
    bad = an.objects(rows, N_STATIONS, NSEC, PLAN, variant="cells_of_side0", **P)
    assert bad[0]["rejected"] == 4 and _differs(rows, "cells_of_side0")


def test_rejections_of_side_and_cell():
    rows = _rows([(3, 0, 0), (0, 5, 0), (1, 6, 5), (1, 7, 0), (2, 4, 5), (2, 5, 0)])
    info, _, of_row = an.objects(rows, N_STATIONS, NSEC, PLAN, **P)
    assert info["rejected"] == 4 and info["side_rows"] == [0, 1, 1] and np.all(of_row == -1)
