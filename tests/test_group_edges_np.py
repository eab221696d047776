"""The sharded frame at slab edges, the CPU half (tests/group_cut_np.py; the GPU half is tests/test_gpu_group_edges.py).

No GPU and none of the library: the numpy twin of the slab cut on the integer tie clouds of tests/normals_np.py, whose
neighbour predicate is exact.  Asserted here, so that the GPU test cannot pass vacuously:
  * the twin reproduces the hand-derived case of host/gm_group_cut_test.cpp and the table of cases below (edges, rows
    owned and sent, pairs with d2 < M across an edge, pairs at exactly d2 = M across an edge);
  * per case: every inner edge inside the cloud has >= 10 000 straddling neighbour pairs, the case has >= 50 straddling
    ties, every row is owned by exactly one rank, every owned row finds all of its exact neighbours among the rows sent
    to its rank, and the neighbourhood kernel's plan of some rank's rows has a tile of halo rows only and a tile that
    mixes halo and owned rows;
  * the checks that the GPU test applies to the library's output (check_counts, check_ownership) pass on a rank simulated
    from the true cut and FAIL on four perturbed cuts: a halo of 0.9 r, ownership closed at the upper edge, an edge one
    float low, and a halo-only skip that also drops mixed tiles;
  * the conditions of the constructed clouds of the further GPU cases (rows on the lattice planes and at edge +- halo, a
    1-NN tie across an edge, ranks with nothing).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binning_np as bn  # noqa: E402
import group_cut_np as gc  # noqa: E402
import normals_np as nn  # noqa: E402

BOUND = 5.0
TABLE, CASES, IDS = gc.TABLE, gc.CASES, gc.IDS
PERTURBED = (7, 0.125, 4)


@functools.lru_cache(maxsize=None)
def case_cut(q, leaf, R):
    xyz, radius = nn.case(f"tie_q{q}")
    return gc.cut(xyz, BOUND, leaf, radius, R)


@functools.lru_cache(maxsize=None)
def exact(q):
    return nn.tie_counts(q, False)


def test_the_twin_reproduces_the_headers_hand_derived_case():
    xyz = np.stack([np.arange(-1.75, 2.0, 0.5), np.zeros(8), np.zeros(8)], axis=1)
    e = gc.edges_of(xyz, 5.0, 0.5, 4)
    assert np.array_equal(e, [-np.inf, -1.0, 0.0, 1.0, np.inf])
    c = gc.cut(xyz, 5.0, 0.5, 0.1, 4)
    assert [s.tolist() for s in c.sent] == [[0, 1], [2, 3], [4, 5], [6, 7]] and c.halo == 1.01 * 0.1
    assert np.array_equal(gc.edges_of(np.zeros((0, 3)), 5.0, 0.5, 4), [-np.inf, 0.0, 0.0, 0.0, np.inf])


@pytest.mark.parametrize("leaf", [0.5, 0.3, 0.25, 0.125, 0.1])
def test_lattice_plane_is_the_smallest_float_of_its_cell(leaf):
    lo, hi = int(gc.lattice_cell(gc.F(-BOUND), leaf)), int(gc.lattice_cell(gc.F(BOUND), leaf))
    for k in range(lo + 1, hi + 1):
        t = gc.lattice_plane(k, leaf)
        assert t.dtype == np.float32 and gc.lattice_cell(t, leaf) == k and gc.lattice_cell(gc._below(t), leaf) == k - 1, (leaf, k, t)
    if leaf in (0.5, 0.25, 0.125):          # a power of two: the planes are the multiples of the leaf
        assert all(float(gc.lattice_plane(k, leaf)) == k * leaf for k in range(lo + 1, hi + 1))
    else:                                    # otherwise some plane is NOT the float nearest k * leaf
        assert any(gc.lattice_plane(k, leaf) != gc.F(k * leaf) for k in range(lo + 1, hi + 1)), leaf


@pytest.mark.parametrize("q,leaf,R", CASES, ids=IDS)
def test_case_table(q, leaf, R):
    xyz, radius = nn.case(f"tie_q{q}")
    P, u = nn.tie_points(q)
    M = nn.TIE_M[q]
    c = case_cut(q, leaf, R)                 # (edges_of asserts the on-lattice branch with shift 0)
    edges, owned, pairs, ties = TABLE[(q, leaf, R)]
    assert c.edges[1:-1].tolist() == edges and gc.inside_box(xyz, BOUND).all()
    assert [int(o.sum()) for o in c.owned] == owned
    if (q, leaf, R) == (7, 0.5, 4):
        assert [len(s) for s in c.sent] == [3733, 1503, 3770, 741]
    per_edge = [gc.straddling_pairs(P, u, M, e) for e in c.edges[1:-1]]
    assert sum(p for p, _ in per_edge) == pairs and sum(t for _, t in per_edge) == ties
    # not vacuous: pairs across every edge that cuts the cloud, ties across some edge
    x = xyz[:, 0]
    for e, (p, _) in zip(c.edges[1:-1], per_edge):
        if x.min() < e <= x.max():
            assert p >= 10000, (e, p)
    assert any(x.min() < e <= x.max() for e in c.edges[1:-1]) and ties >= 50
    # every row owned once; every owned row sees all of its neighbours among the rows sent to its rank
    assert np.array_equal(np.sum(c.owned, axis=0), np.ones(len(xyz), np.int64))
    some_halo_only = some_mixed = False
    for r in range(R):
        sent = c.sent[r]
        own = c.owned[r][sent]
        assert (c.owned[r].sum() == own.sum())                     # a rank is sent what it owns
        cnt, valid = gc.simulate_rank(P, M, sent, own)
        assert np.array_equal(cnt[own], exact(q)[sent][own]), r
        if len(sent):
            h, m, _, _ = gc.tile_census(xyz[sent], own, BOUND, radius)
            some_halo_only |= h > 0
            some_mixed |= m > 0
    assert some_halo_only and some_mixed


# ---------------------------------------------------------------- the checks bite

def simulated(edges, halo, upper_closed=False, drop_mixed=False):
    """What the ranks of a group that cuts tie_q7 by (edges, halo) would report: [(rows, owned, counts, valid rows)]."""
    q, leaf, R = PERTURBED
    xyz, radius = nn.case(f"tie_q{q}")
    P, _ = nn.tie_points(q)
    out = []
    for r in range(R):
        sent = gc.sent_rows(xyz[:, 0], edges, halo, r)
        own = gc.owned_mask(xyz[:, 0], edges, r)[sent]
        if upper_closed:
            own = own | (xyz[sent, 0].astype(np.float64) == edges[r + 1])
        dropped = gc.tile_census(xyz[sent], own, BOUND, radius)[3] if drop_mixed else None
        cnt, valid = gc.simulate_rank(P, nn.TIE_M[q], sent, own, dropped)
        out.append((sent, own, cnt, valid))
    return out


def apply_checks(ranks):
    """Assertions 1 and 2 of the GPU test on simulated ranks, against the TRUE cut."""
    c = case_cut(*PERTURBED)
    ex = exact(PERTURBED[0])
    for r, (sent, own, cnt, valid) in enumerate(ranks):
        assert np.array_equal(sent, gc.sent_inside(c, r)), ("rows sent", r, len(sent), len(gc.sent_inside(c, r)))
        gc.check_counts(sent, c.owned[r][sent], cnt, ex, tag=r)
    gc.check_ownership(c, [v for _, _, _, v in ranks], np.flatnonzero(ex >= 3))


def test_the_checks_pass_on_the_true_cut():
    c = case_cut(*PERTURBED)
    apply_checks(simulated(c.edges, c.halo))


def test_a_halo_of_0_9_r_fails_the_checks():
    c = case_cut(*PERTURBED)
    _, radius = nn.case("tie_q7")
    ranks = simulated(c.edges, 0.9 * radius)
    with pytest.raises(AssertionError, match="rows sent"):
        apply_checks(ranks)
    # and with the row lists aside, the counts themselves: owned rows beside an edge miss neighbours
    ex = exact(7)
    with pytest.raises(AssertionError, match="owned rows with a wrong count"):
        for sent, own, cnt, _ in ranks:
            gc.check_counts(sent, own, cnt, ex)


def test_ownership_closed_at_the_upper_edge_fails_the_checks():
    c = case_cut(*PERTURBED)
    xyz, _ = nn.case("tie_q7")
    assert all((xyz[:, 0] == e).sum() >= 5 for e in c.edges[1:-1])          # rows ON every inner edge
    with pytest.raises(AssertionError, match="valid rows"):
        apply_checks(simulated(c.edges, c.halo, upper_closed=True))


def test_mixed_tiles_dropped_with_the_halo_only_ones_fails_the_checks():
    c = case_cut(*PERTURBED)
    with pytest.raises(AssertionError, match="owned rows with a wrong count"):
        apply_checks(simulated(c.edges, c.halo, drop_mixed=True))


def test_an_edge_one_float_low_fails_the_checks():
    """On the 2^-7 lattice itself no row lies in the one-float gap below an edge, so the pure tie cloud cannot see this
    perturbation (asserted).  The GPU suite therefore plants rows at the float below every lattice plane; here the tie
    cloud gets, at every inner edge, a copy of a row ON the edge moved to the float below it -- in units of 2^-22 the
    cloud is still an integer one, and count_exact still exact -- and the ownership check fails."""
    q, leaf, R = PERTURBED
    xyz, radius = nn.case("tie_q7")
    c = case_cut(q, leaf, R)
    low = c.edges.copy()
    low[1:-1] = [float(gc._below(e)) for e in c.edges[1:-1]]
    assert all(not ((xyz[:, 0] >= a) & (xyz[:, 0] < b)).any() for a, b in zip(low[1:-1], c.edges[1:-1]))
    apply_checks(simulated(low, c.halo))                                       # blind on the pure lattice
    P7, u7 = nn.tie_points(7)
    fine = 1 << 15                                                             # 2^-7 -> 2^-22
    P, M = P7 * fine, nn.TIE_M[7] * fine * fine
    add = []
    for e in c.edges[1:-1]:
        src = int(np.flatnonzero(xyz[:, 0] == e)[0])
        p = P[src].copy()
        p[0] = int(round(float(gc._below(e)) * 2.0 ** 22))
        assert p[0] * 2.0 ** -22 == float(gc._below(e)) and p[0] < P[src][0]
        add.append(p)
    P = np.vstack([P, add])
    X = (P * 2.0 ** -22).astype(np.float32)
    assert np.array_equal(X.astype(np.float64) * 2.0 ** 22, P) and np.array_equal(gc.edges_of(X, BOUND, leaf, R), c.edges)
    ex = nn.count_exact(P, M)
    kept = np.flatnonzero(ex >= 3)
    assert (ex[len(P7):] >= 3).all()
    true = gc.cut(X, BOUND, leaf, radius, R)

    def ranks(edges):
        out = []
        for r in range(R):
            sent = gc.sent_rows(X[:, 0], edges, true.halo, r)
            out.append(gc.simulate_rank(P, M, sent, gc.owned_mask(X[:, 0], edges, r)[sent])[1])
        return out

    gc.check_ownership(true, ranks(true.edges), kept)
    with pytest.raises(AssertionError, match="valid rows"):
        gc.check_ownership(true, ranks(low), kept)


# ---------------------------------------------------------------- the constructed clouds of the further GPU cases

@pytest.mark.parametrize("leaf", [0.5, 0.3])
@pytest.mark.parametrize("R", [2, 4])
def test_planes_cloud_has_a_row_on_every_plane_and_at_every_halo_limit(leaf, R):
    radius = 0.3
    base = nn.tunnel_n(20000, 20000)
    pl = gc.planes_cloud(base, BOUND, leaf, radius, R)
    xyz = pl.xyz
    c = gc.cut(xyz, BOUND, leaf, radius, R)
    assert np.array_equal(c.edges, pl.edges) and c.inside.all()
    assert len(pl.plane_rows) >= 9.5 / leaf
    for k, row in pl.plane_rows.items():
        x, xb = xyz[row, 0], xyz[pl.below_rows[k], 0]
        assert gc.lattice_cell(x, leaf) == k and gc.lattice_cell(xb, leaf) == k - 1 and xb == gc._below(x)
    planes = {float(xyz[row, 0]): k for k, row in pl.plane_rows.items()}
    for g in range(1, R):                                # the row ON edge g is the upper rank's, the float below the lower's
        k = planes[c.edges[g]]
        assert c.owned[g][pl.plane_rows[k]] and c.owned[g - 1][pl.below_rows[k]]
    # rows at the floats around edge +- halo: of each pair one is sent to the rank across the edge and one is not
    hx = xyz[pl.halo_rows, 0].astype(np.float64)
    for g in range(1, R):
        lo, hi = c.edges[g] - c.halo, c.edges[g] + c.halo
        assert (hx < lo).any() and (hx >= lo).any() and (hx < hi).any() and (hx >= hi).any()
        near_lo, near_hi = hx[np.abs(hx - lo) < 1e-6], hx[np.abs(hx - hi) < 1e-6]
        assert len(near_lo) >= 2 and len(near_hi) >= 2
        sent_up, sent_dn = set(c.sent[g].tolist()), set(c.sent[g - 1].tolist())
        for row in pl.halo_rows:
            x = float(xyz[row, 0])
            if abs(x - lo) < 1e-6:
                assert (row in sent_up) == (x >= lo)
            if abs(x - hi) < 1e-6:
                assert (row in sent_dn) == (x < hi)
    assert all(o.sum() > 1000 for o in c.owned)


def test_nn_tie_cloud_ties_across_the_edge():
    t = gc.NN_TIE
    for swapped in (False, True):
        xyz, a, b0, C = gc.nn_tie_cloud(swapped)
        c = gc.cut(xyz, t["bound"], t["leaf"], t["radius"], t["R"])
        assert c.edges[1] == 0.0 and c.owned[0][a] and c.owned[1][b0] and c.inside.all()
        # validity: >= 3 neighbours (exact in units of 2^-6) that are not collinear, for the tied points and the voxel's own
        P = np.round(xyz.astype(np.float64) * 64).astype(np.int64)
        M = int(round(t["radius"] * t["radius"] * 4096 - 0.5)) + 1     # d2 < r^2 <=> d2_int < 368.64 <=> d2_int <= 368
        assert M - 1 < t["radius"] ** 2 * 4096 < M
        cnt = nn.count_exact(P, M)
        valid = np.flatnonzero(cnt >= 3)
        for row in (a, b0, 2, 3):
            d = P - P[row]
            nb = d[((d * d).sum(axis=1) < M)]
            assert cnt[row] >= 4 and np.linalg.matrix_rank(nb) == 3, row
        # the voxel of C holds exactly rows b0, 2, 3 of the valid cloud, and their mean is C
        cell = gc.lattice_cell(xyz, t["leaf"])
        in_v = np.flatnonzero((cell == gc.lattice_cell(C, t["leaf"])).all(axis=1))
        assert sorted(in_v.tolist()) == sorted([b0, 2, 3]) and set(in_v) <= set(valid)
        assert np.array_equal(xyz[in_v].astype(np.float64).mean(axis=0).astype(np.float32), C)
        # the tie: equal fp32 d2 bits as nearest_brute computes them, no valid point closer, the lower input row wins
        v = xyz[valid]
        d = C[None, :] - v
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        ia, ib = int(np.searchsorted(valid, a)), int(np.searchsorted(valid, b0))
        assert d2[ia].view(np.uint32) == d2[ib].view(np.uint32) == d2.min().view(np.uint32) and (d2 == d2.min()).sum() == 2
        assert bn.nearest_brute(v, C[None, :])[0] == min(ia, ib) == (ib if swapped else ia)


def test_clouds_of_the_ranks_with_nothing():
    radius, leaf, R = 0.3, 0.5, 4
    a = gc.sheet(2000, 0.3, 0.45, 1)
    c = gc.cut(a, BOUND, leaf, radius, R)
    assert c.edges[1:-1].tolist() == [0.5, 0.5, 0.5]
    assert [int(o.sum()) for o in c.owned] == [2000, 0, 0, 0] and [len(s) for s in c.sent] == [2000] * 4
    b = a - np.array([0.3, 0, 0], np.float32)
    assert (b[:, 0] >= 0).all()
    c = gc.cut(b, BOUND, leaf, radius, R)
    assert c.edges[1:-1].tolist() == [0.5, 0.5, 0.5] and [len(s) for s in c.sent] == [2000, 0, 0, 0]
