"""Plain numpy twin of a group's slab cut (csrc/gm_group_cut.hpp, DESIGN.md par. 6), written from the cut's RULE and not
from the header's loops, and the checks that tests/test_group_edges_np.py (CPU) and tests/test_gpu_group_edges.py (GPU)
share.  No GPU and none of the code under test.

The rule, on-lattice branch with shift 0 (every case asserts that it is in it):
  lattice_cell(x)   floor(fp32(x * fp32(1 / fp32(leaf)))): pcl::VoxelGrid's index of a coordinate, in fp32 as the kernels.
  lattice_plane(k)  the smallest float of cell k.  The cell map is monotone over the floats, so the plane is found by
                    bisection over the floats' total order (their bits as a monotone integer) -- no stepping.
  edge g            behind the first x cell of the box at which run * R >= n_in * g, `run` the in-box rows up to and
                    including that cell, n_in all in-box rows.  An empty frame: every inner edge at 0.
  halo              1.01 * radius, in double.
  sent to rank r    the rows with x >= edge[r] - halo and x < edge[r + 1] + halo, in double (in-box or not; NaN fails both).
  owned by rank r   edge[r] <= x < edge[r + 1].
The pieces (edges_of, sent_rows, owned_mask) are separate so that a test can perturb one of them.

Checks shared with the GPU test:
  check_counts      assertion 1: a rank's neighbour counts, in the order of the rows sent, are the exact counts on owned
                    rows and 0 or in [1, exact] on halo rows.
  check_ownership   assertion 2 (the ranks' half): every rank's valid rows are the rows it owns among those the unsharded
                    frame kept -- so every kept row comes out of exactly one rank.
  simulate_rank     what a rank that follows a (possibly perturbed) cut reports on an integer lattice cloud, by
                    normals_np.count_exact: the counting reference of the perturbation tests.
"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_np as nn  # noqa: E402

F = np.float32
HALO = 1.01

# The cases of the sharded tie clouds (bound 5, the cloud's own radius), computed on the CPU and asserted by
# tests/test_group_edges_np.py.  # (q, leaf, R): inner edges, rows owned per rank, straddling pairs with d2 < M (summed over the inner edges), with d2 == M
TABLE = {
    (7, 0.125, 4): ([3.625, 4.0, 4.625], [1871, 1138, 1855, 1136], 251294, 958),
    (7, 0.25, 3): ([3.75, 4.5], [2230, 2242, 1528], 174744, 677),
    (7, 0.5, 2): ([4.0], [3009, 2991], 76745, 285),
    (7, 0.5, 4): ([4.0, 4.0, 5.0], [3009, 0, 2991, 0], 153490, 570),
    (14, 0.125, 4): ([3.625, 4.125, 4.5], [1935, 1521, 1172, 1514], 262645, 188),
    (14, 0.25, 2): ([4.25], [3824, 2318], 90632, 83),
}
CASES = list(TABLE)
IDS = [f"tie_q{q}-leaf{leaf}-R{R}" for q, leaf, R in CASES]


def inv_leaf(leaf):
    inv = F(1.0) / F(leaf)
    assert inv.dtype == np.float32
    return inv


def lattice_cell(x, leaf):
    """int64 cell of every x (fp32 product, then floor)."""
    t = np.asarray(x, dtype=np.float32) * inv_leaf(leaf)
    assert t.dtype == np.float32
    return np.floor(t).astype(np.int64)


def _ordinal(f):
    """A float's place in the total order of the floats, as an int (monotone: -0.0 and +0.0 share 0)."""
    b = int(np.asarray(f, dtype=np.float32).view(np.int32))
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def _float_at(o):
    return np.array(o if o >= 0 else (-o) | 0x80000000, dtype=np.uint32).view(np.float32)[()]


def lattice_plane(k, leaf):
    """The smallest float t with lattice_cell(t) >= k."""
    far = F(2.0 ** 40) * F(max(float(leaf), 1.0))        # |cell| reaches 2^40 there and the product stays finite
    lo, hi = _ordinal(-far), _ordinal(far)
    assert lattice_cell(_float_at(lo), leaf) < k <= lattice_cell(_float_at(hi), leaf)
    while hi - lo > 1:                                   # cell(lo) < k <= cell(hi)
        mid = (lo + hi) // 2
        if lattice_cell(_float_at(mid), leaf) >= k:
            hi = mid
        else:
            lo = mid
    return _float_at(hi)


def inside_box(xyz, bound):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.isfinite(xyz).all(axis=1) & (np.abs(xyz) <= F(bound)).all(axis=1)


def edges_of(xyz, bound, leaf, R):
    """[R + 1] doubles, -inf and +inf at the ends.  Asserts the on-lattice branch with shift 0."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    c_lo, c_hi = int(lattice_cell(F(-bound), leaf)), int(lattice_cell(F(bound), leaf))
    ncell = c_hi - c_lo + 1
    assert 4 * R <= ncell <= (1 << 20), "the twin covers the on-lattice branch with shift 0 only"
    cells = lattice_cell(xyz[inside_box(xyz, bound), 0], leaf) - c_lo
    n_in = len(cells)
    e = np.empty(R + 1, np.float64)
    e[0], e[R] = -np.inf, np.inf
    if n_in == 0:
        e[1:R] = 0.0
        return e
    run = np.cumsum(np.bincount(cells, minlength=ncell))
    for g in range(1, R):
        b = int(np.flatnonzero(run * R >= n_in * g)[0])
        e[g] = float(lattice_plane(c_lo + b + 1, leaf))
    assert (np.diff(e[1:R]) >= 0).all()
    return e


def sent_rows(x, edges, halo, r):
    """Input rows sent to rank r, ascending."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((x >= edges[r] - halo) & (x < edges[r + 1] + halo))


def owned_mask(x, edges, r):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (x >= edges[r]) & (x < edges[r + 1])


Cut = collections.namedtuple("Cut", "R edges halo inside sent owned")
# sent[r]: input rows sent to rank r (ascending); owned[r]: bool over ALL input rows


def cut(xyz, bound, leaf, radius, R):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    e = edges_of(xyz, bound, leaf, R)
    halo = HALO * float(radius)
    return Cut(R, e, halo, inside_box(xyz, bound), [sent_rows(xyz[:, 0], e, halo, r) for r in range(R)],
               [owned_mask(xyz[:, 0], e, r) for r in range(R)])


def sent_inside(c, r):
    """The rows of rank r that pass its crop, ascending: what its per-point outputs are indexed by."""
    return c.sent[r][c.inside[c.sent[r]]]


# ---------------------------------------------------------------- the checks the CPU and the GPU tests share

def check_counts(rows, owned, got, exact, tag=""):
    """Assertion 1 for one rank.  rows: the input rows behind `got` (the in-box rows sent, ascending); owned: bool per
    entry of rows; exact: the reference count of every INPUT row.  Returns the number of halo rows that reported 0."""
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == (len(rows),), (tag, got.dtype, got.shape, len(rows))
    want = np.asarray(exact)[rows]
    bad = np.flatnonzero(owned & (got != want))
    assert len(bad) == 0, (tag, "owned rows with a wrong count", len(bad), rows[bad[:8]], got[bad[:8]], want[bad[:8]])
    halo = ~owned
    bad = np.flatnonzero(halo & (got != 0) & ((got < 1) | (got > want)))
    assert len(bad) == 0, (tag, "halo rows with a count outside [1, exact]", len(bad), rows[bad[:8]], got[bad[:8]], want[bad[:8]])
    return int((halo & (got == 0)).sum())


def check_ownership(c, rank_valid_rows, kept, tag=""):
    """Assertion 2, the ranks' half.  rank_valid_rows[r]: the input rows of rank r's valid cloud; kept: the input rows
    the unsharded frame kept (ascending)."""
    kept = np.asarray(kept, dtype=np.int64)
    is_kept = np.zeros(len(c.inside), bool)
    is_kept[kept] = True
    seen = np.zeros(len(c.inside), np.int64)
    for r in range(c.R):
        got = np.sort(np.asarray(rank_valid_rows[r], dtype=np.int64))
        want = np.flatnonzero(c.owned[r] & is_kept)
        assert np.array_equal(got, want), (tag, "rank", r, "valid rows", len(got), "owned and kept", len(want),
                                           np.setdiff1d(got, want)[:8], np.setdiff1d(want, got)[:8])
        np.add.at(seen, got, 1)
    assert np.array_equal(seen, is_kept.astype(np.int64)), (tag, "a kept row comes out of no rank or of several")


def simulate_rank(P_int, M, sent, owned, dropped=None):
    """(counts over the rows sent, the input rows of the rank's valid cloud) of a rank that is sent `sent` and owns
    `owned` (bool over the rows sent) of the integer cloud P_int.  dropped: bool over the rows sent, rows of tiles that
    the rank skips (count 0, no output).  A row is valid with >= 3 neighbours, as in the frame."""
    sent = np.asarray(sent)
    cnt = nn.count_exact(np.asarray(P_int)[sent], M) if len(sent) else np.zeros(0, np.int32)
    if dropped is not None:
        cnt = np.where(dropped, 0, cnt).astype(np.int32)
    return cnt, sent[owned & (cnt >= 3)]


def tile_census(xyz_sent, owned, bound, radius):
    """(tiles of halo rows only, tiles that mix halo and owned rows, tiles of owned rows only, bool per row sent: the
    row lies in a mixed tile) of the neighbourhood kernel's plan on a rank's rows (normals_np.plan)."""
    p = nn.plan(xyz_sent, bound, radius)
    halo_only = mixed = own_only = 0
    in_mixed = np.zeros(len(xyz_sent), bool)
    for t in p["tiles"]:
        rows = p["order"][t["s"]:t["s"] + t["qn"]]
        k = int(owned[rows].sum())
        if k == 0:
            halo_only += 1
        elif k == len(rows):
            own_only += 1
        else:
            mixed += 1
            in_mixed[rows] = True
    return halo_only, mixed, own_only, in_mixed


def straddling_pairs(P_int, u, M, edge):
    """(pairs with d2 < M, pairs with d2 == M) of the integer cloud P_int (unit u) with one point on each side of the
    plane x = edge; unordered pairs, integer arithmetic."""
    P, _ = nn._by_x(P_int)
    side = (P[:, 0] * u) >= edge
    below = ties = 0
    for a, b, lo, hi, d2 in nn._windows(P, M):
        cross = side[a:b, None] != side[None, lo:hi]
        below += int((cross & (d2 < int(M))).sum())
        ties += int((cross & (d2 == int(M))).sum())
    assert below % 2 == 0 and ties % 2 == 0
    return below // 2, ties // 2


# ---------------------------------------------------------------- constructed clouds of the further cases

def _below(f):
    return np.nextafter(F(f), F(-np.inf))


def _above(f):
    return np.nextafter(F(f), F(np.inf))


def floats_around(v):
    """The nearest floats on both sides of the double v: (the largest float <= v, the smallest float >= v), and when v is a
    float itself its two neighbours besides."""
    a = F(v)
    if float(a) == v:
        return [_below(a), a, _above(a)]
    return [a, _above(a)] if float(a) < v else [_below(a), a]


COMPANIONS = np.array([[0.0, 0.0, 0.0], [0.0, 0.03125, 0.0], [0.0, 0.0, 0.03125], [0.0, -0.03125, -0.03125]], np.float32)


def _plant(base, xs):
    """Rows at the given x, each with three companions at the SAME x (so that all four lie on the same side of every
    plane) 1/32 away in y / z: four points that are not collinear, valid at any radius above 0.05.  y and z are those
    of the base point nearest in x.  Returns ([4 len(xs), 3] rows, the index of each planted row among them)."""
    xs = np.asarray(xs, dtype=np.float32)
    near = np.abs(base[None, :, 0].astype(np.float64) - xs[:, None].astype(np.float64)).argmin(axis=1)
    rows = np.repeat(base[near], 4, axis=0).astype(np.float32)
    rows[:, 0] = np.repeat(xs, 4)
    rows += np.tile(COMPANIONS, (len(xs), 1))
    return rows, 4 * np.arange(len(xs))


Planted = collections.namedtuple("Planted", "xyz n_base plane_rows below_rows halo_rows edges")
# plane_rows / below_rows: {k: input row of the row at lattice_plane(k) / at the float below it}; halo_rows: input rows of
# the rows at edge +- halo; edges: the twin's, of xyz


def planes_cloud(base, bound, leaf, radius, R):
    """base with a row ON every lattice plane of its x range and a row at the float below, and rows at the floats around
    edge +- halo of every inner edge of the AUGMENTED cloud (one more round if planting them moves an edge; then they stay
    put).  Planted rows come behind the base rows, each followed by its companions."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    assert inside_box(base, bound).all()
    cells = lattice_cell(base[:, 0], leaf)
    ks = list(range(int(cells.min()) + 1, int(cells.max()) + 1))
    planes = np.array([lattice_plane(k, leaf) for k in ks], np.float32)
    assert (lattice_cell(planes, leaf) == ks).all() and (lattice_cell(_below(planes), leaf) == np.array(ks) - 1).all()
    on, at = _plant(base, planes)
    under, _ = _plant(base, _below(planes))
    aug = np.vstack([base, on, under])
    plane_rows = {k: len(base) + int(a) for k, a in zip(ks, at)}
    below_rows = {k: len(base) + len(on) + int(a) for k, a in zip(ks, at)}
    halo = HALO * float(radius)
    e = edges_of(aug, bound, leaf, R)
    for _ in range(2):
        xs = [f for g in range(1, R) for s in (-1.0, 1.0) for f in floats_around(e[g] + s * halo)]
        rows, at = _plant(base, xs)
        full = np.vstack([aug, rows])
        assert inside_box(full, bound).all()
        e2 = edges_of(full, bound, leaf, R)
        if np.array_equal(e2, e):
            return Planted(full, len(base), plane_rows, below_rows, len(aug) + at, e)
        e = e2
    raise AssertionError("the edges do not settle")


def bound_cloud(base, bound):
    """base (rows inside and outside the box) with rows at exactly +-bound in each coordinate and at the floats just
    beyond, each with companions inside the box where the row itself is."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    inner = base[inside_box(base, 0.8 * bound)]
    rows = []
    for axis in range(3):
        for s in (-1.0, 1.0):
            for v in (F(s * bound), np.nextafter(F(s * bound), F(s * np.inf))):
                p = np.repeat(inner[7 * axis + 3:7 * axis + 4], 4, axis=0) + COMPANIONS
                p[:, axis] = v
                rows.append(p)
    return np.vstack([base] + rows).astype(np.float32)


def sheet(n, x0, x1, seed):
    """n points of a thin sheet z ~ 0.2 with x in [x0, x1] and |y| < 1."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(-1.0, 1.0, n), 0.2 + rng.uniform(-0.004, 0.004, n)], axis=1).astype(np.float32)


# A 1-NN tie across an edge (bound 5, leaf 0.5, radius 0.3, two ranks; every coordinate a multiple of 2^-6).  The voxel
# x, y, z in [0, 0.5) holds three valid points B0, B1, B2 whose mean is C = (1/16, 1/8, 1/4).  B0 = C + (3, 4, 0) / 32 and
# A = C - (5, 0, 0) / 32 (x < 0: the lower rank's) are both 5 / 32 from C; B1 and B2 are further.  Every one of the five has
# three companions outside that voxel and further from C; a filler cluster far below balances the cut at x = 0.
NN_TIE = dict(bound=5.0, leaf=0.5, radius=0.3, R=2)
_C = np.array([2.0, 4.0, 8.0]) / 32.0


def nn_tie_cloud(swapped):
    """(xyz, row of A, row of B0, C).  A comes first in the input; swapped: B0 does."""
    A, B0 = _C - np.array([5.0, 0, 0]) / 32, _C + np.array([3.0, 4.0, 0]) / 32
    B1, B2 = _C + np.array([-1.5, -2.0, 6.0]) / 32, _C + np.array([-1.5, -2.0, -6.0]) / 32
    comp = {
        "A": A + np.array([[-4.0, 0, 0], [-2.0, 4.0, 0], [-2.0, 0, 4.0]]) / 32,
        "B0": B0 + np.array([[1.0, 8.0, 0], [0, 8.0, 2.0], [2.0, 8.0, -2.0]]) / 32,       # y >= 0.5: the next voxel
        "B1": B1 + np.array([[0, 0, 2.0], [2.0, 2.0, 2.0], [2.0, 0, 4.0]]) / 32,          # z >= 0.5
        "B2": B2 + np.array([[0, 0, -4.0], [2.0, 2.0, -4.0], [2.0, 0, -6.0]]) / 32,       # z < 0
    }
    rng = np.random.default_rng(3)
    filler = np.array([-0.4375, -2.0, -2.0]) + rng.integers(0, 8, (12, 3)) / 64.0
    first, second = (B0, A) if swapped else (A, B0)
    xyz = np.vstack([first[None], second[None], B1[None], B2[None]] + list(comp.values()) + [filler])
    assert np.array_equal(xyz * 64, np.round(xyz * 64))
    return xyz.astype(np.float32), (1 if swapped else 0), (0 if swapped else 1), _C.astype(np.float32)
