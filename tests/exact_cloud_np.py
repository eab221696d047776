"""Clouds on which the fp32 per-point chain of the wall maps (gm_device.hpp: surf_rho, surf_residual, surf_station) is
exact, so that an fp64 evaluation gives the same bits and the device's per-point (e, cell) can be compared bit for bit
with values that never came from the device (tests/test_exact_cloud_np.py asserts the claims made here).

Construction: a primitive Pythagorean triple (a, b, c), a multiplier k and the scale 2^-8.  The eight points
(+-a, +-b) k / 256 and (+-b, +-a) k / 256 of the plane across the axis have rho = c k / 256; with c <= 1024 and
c k <= 2560 the squares, their sum (< 2^23 in units of 2^-16), the root and e = rho - R for R = 2 are exact in fp32, and
e 2^20 = (c k - 512) 2^12 is an integer of at most 2^23.  The axis lies on a coordinate axis and the frame vectors are
signed unit vectors, t is a multiple of ds / 4 (ds = 0.25) and translations are dyadic: o, a, u, v, t, w and the station
are exact too.  Only the sector goes through atan2f, which the device does not round correctly: base_points() keeps the
points whose phi / dtheta lies at least MARGIN = 0.05 of a sector from an integer (7.7e-5 rad at 4096 sectors, far
beyond any atan2f error), and asserts that at least MIN_SHARE of the base points stay.

A Spec is the cloud before it is placed: per point the exact t, the plane coordinates y = w.u and z = w.v, e, the sector,
the label and the kind of a bad row.  xyz() places it in a frame, expected() gives the per-point (e, cell, class) of the
stated rule (include/gm_hip.h) from the Spec alone; the expected cells are surface_np.cells_from / wall_np.cells_from of
those."""
from math import gcd

import numpy as np

SCALE = 256
C_MAX, CK_MAX = 1024, 2560
MARGIN, MIN_SHARE = 0.05, 0.80
R_DESIGN = 2.0
MAPPED, OUTSIDE, BEYOND, PLANE = 0, 1, 2, 3
GOOD, NAN_ROW, POS_INF_ROW, NEG_INF_ROW = 0, 1, 2, 3
FIELDS = ("t", "y", "z", "e", "sector", "labels", "bad")


def triples(c_max=C_MAX):
    """Primitive Pythagorean triples (a < b, c <= c_max), by Euclid's formula, sorted by c."""
    out = []
    m = 2
    while m * m + 1 <= c_max:
        for n in range(1, m):
            if (m - n) % 2 == 1 and gcd(m, n) == 1 and m * m + n * n <= c_max:
                a, b = m * m - n * n, 2 * m * n
                out.append((min(a, b), max(a, b), m * m + n * n))
        m += 1
    return sorted(out, key=lambda t: (t[2], t[0]))


def all_points(gate, R=R_DESIGN):
    """Every base point with |e| <= gate, before the sector margin: y, z, e (fp64, exact dyadic values)."""
    rows = []
    for a, b, c in triples():
        for k in range(1, CK_MAX // c + 1):
            e = c * k / SCALE - R
            if abs(e) <= gate:
                for p, q in ((a, b), (b, a)):
                    for sp in (1, -1):
                        for sq in (1, -1):
                            rows.append((sp * p * k / SCALE, sq * q * k / SCALE, e))
    r = np.array(rows, np.float64).reshape(-1, 3)
    return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()


def sector_coordinate(y, z, n_sectors):
    """phi / dtheta in fp64 with the device's fp32 dtheta; phi = atan2(z, y) folded to [0, 2 pi)."""
    dth = float(np.float32(2 * np.pi / n_sectors))
    return np.mod(np.arctan2(z, y), 2 * np.pi) / dth


def base_points(gate, n_sectors, R=R_DESIGN):
    """dict(y, z (fp64, exact in fp32), e (fp32), sector (int64), n_base, share): the base points with |e| <= gate whose
    sector on an n_sectors grid does not depend on the rounding of atan2f."""
    y, z, e = all_points(gate, R)
    ys = sector_coordinate(y, z, n_sectors)
    keep = np.abs(ys - np.rint(ys)) >= MARGIN
    share = float(keep.mean())
    assert share >= MIN_SHARE, (gate, n_sectors, share)
    sector = np.minimum(np.floor(ys[keep]), n_sectors - 1).astype(np.int64)
    return dict(y=y[keep], z=z[keep], e=e[keep].astype(np.float32), sector=sector, n_base=len(y), share=share)


def beyond_points(gate, n_sectors, R=R_DESIGN):
    """Exact base points with gate < |e| <= 8: beyond the gate by an exact residual."""
    b = base_points(8.0, n_sectors, R)
    m = np.abs(b["e"].astype(np.float64)) > float(np.float32(gate))
    return {k: (v[m] if isinstance(v, np.ndarray) else v) for k, v in b.items()}


# ---- a cloud before it is placed ----

def spec(base, idx, t, labels=None):
    """The base points idx at the axial coordinates t (relative to the frame's origin o)."""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    return dict(t=np.broadcast_to(np.asarray(t, np.float64), (n,)).copy(), y=base["y"][idx].copy(), z=base["z"][idx].copy(),
                e=base["e"][idx].copy(), sector=base["sector"][idx].copy(),
                labels=np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8).copy(),
                bad=np.zeros(n, np.uint8))


def concat(*specs):
    return {k: np.concatenate([s[k] for s in specs]) for k in FIELDS}


def take(s, idx):
    return {k: s[k][idx].copy() for k in FIELDS}


def set_rows(s, rows, other):
    """Rows `rows` of s become the rows of `other` (in place)."""
    for k in FIELDS:
        s[k][rows] = other[k]
    return s


def axis_point(t, R=R_DESIGN):
    """One point on the axis: rho = 0, e = -R, atan2(+0, +0) = 0: sector 0 (in a frame whose u and v make w.u = +0)."""
    return dict(t=np.array([t], np.float64), y=np.zeros(1), z=np.zeros(1), e=np.array([-R], np.float32),
                sector=np.zeros(1, np.int64), labels=np.zeros(1, np.uint8), bad=np.zeros(1, np.uint8))


def stations_t(j, frac, ds=0.25, t0=0.0):
    """t of station j (relative to t0) at the fraction frac of the station (multiples of 1/4 keep t dyadic for ds = 0.25)."""
    return t0 + (np.asarray(j, np.float64) + np.asarray(frac, np.float64)) * ds


def fill(base, n, n_stations, ds=0.25, t0=0.0, seed=0, fracs=(0, 1, 2, 3)):
    """n points: the base points in a seeded order, repeated as often as needed, over every station of the grid at the
    fractions fracs / 4 of a station (0 is the closed-left edge itself)."""
    rng = np.random.default_rng(seed)
    reps = -(-max(n, 1) // len(base["e"]))
    idx = np.concatenate([rng.permutation(len(base["e"])) for _ in range(reps)])[:n]
    j = rng.integers(0, n_stations, n)
    frac = np.asarray(fracs, np.float64)[rng.integers(0, len(fracs), n)] / 4.0
    return spec(base, idx, stations_t(j, frac, ds, t0))


def of_cell(base, sector):
    """Indices of the base points of one sector, ascending e."""
    i = np.flatnonzero(base["sector"] == sector)
    return i[np.argsort(base["e"][i], kind="stable")]


def run_indices(base, sector, length, where):
    """`length` base points of one sector (repeated when the sector has fewer), with the run's minimum and maximum each
    placed once, at `where` = (position of the minimum, position of the maximum): 'head', 'middle' or 'tail'."""
    own = of_cell(base, sector)
    assert len(own) >= 3, sector
    lo, hi, mid = own[0], own[-1], own[1:-1]
    assert base["e"][lo] <= base["e"][mid].min() and base["e"][hi] >= base["e"][mid].max()
    pos = dict(head=0, middle=length // 2, tail=length - 1)
    out = np.resize(mid, length)
    plo, phi = pos[where[0]], pos[where[1]]
    if plo == phi:
        phi = plo + 1 if plo + 1 < length else plo - 1
    out[plo], out[phi] = lo, hi
    return out


def cancelling_indices(base, sector, longest=64):
    """Base points of one sector whose rint(e 2^20) add up to 0 (n1 points of a negative e, n2 of a positive one), or
    None when the sector has no such pair within `longest` points."""
    own = of_cell(base, sector)
    q = np.rint(base["e"][own].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    best = None
    for i in np.flatnonzero(q < 0):
        for j in np.flatnonzero(q > 0):
            g = gcd(int(-q[i]), int(q[j]))
            n1, n2 = int(q[j]) // g, int(-q[i]) // g
            if n1 + n2 <= longest and (best is None or n1 + n2 < len(best)):
                best = np.array([own[i]] * n1 + [own[j]] * n2, np.int64)
    return best


# ---- placing and the expected outputs ----

def frame(o, a, u, v):
    return dict(o=np.asarray(o, np.float64), a=np.asarray(a, np.float64), u=np.asarray(u, np.float64),
                v=np.asarray(v, np.float64))


def xyz(s, f):
    """The Spec in the frame f = dict(o, a, u, v): fp32 rows, each coordinate exactly o + t a + y u + z v (asserted);
    bad rows are NaN or carry one infinite coordinate."""
    p = f["o"] + s["t"][:, None] * f["a"] + s["y"][:, None] * f["u"] + s["z"][:, None] * f["v"]
    with np.errstate(over="ignore"):
        out = p.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), p), "a coordinate is not an fp32 number"
    out[s["bad"] == NAN_ROW] = np.nan
    for kind, val in ((POS_INF_ROW, np.inf), (NEG_INF_ROW, -np.inf)):
        rows = np.flatnonzero(s["bad"] == kind)
        out[rows, rows % 3] = val
    return out


def stations(s, ds, t0=0.0, j0=0):
    """j0 + floor((t - t0) / ds) per point as fp64 (huge for a far point), asserted equal in fp32 and fp64 arithmetic."""
    ds32, t032 = np.float32(ds), np.float32(t0)
    t32 = s["t"].astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), s["t"])
    with np.errstate(over="ignore"):
        j32 = np.floor((t32 - t032) / ds32).astype(np.float64)
    j64 = np.floor((s["t"] - float(t032)) / float(ds32))
    near = np.abs(j64) < 2.0 ** 23
    assert np.array_equal(j32[near], j64[near]) and np.all(np.abs(j32[~near]) >= 2.0 ** 23)
    return j64 + j0


def expected(s, gate, ds, n_stations, n_sectors, t0=0.0, j0=0):
    """The stated rule on the Spec: dict(e (fp32; NaN for plane points and bad rows), cell (int64, -1 unless mapped),
    cls, counts (mapped, outside, beyond_gate, plane)).  The station is j0 + floor((t - t0) / ds)."""
    j = stations(s, ds, t0, j0)
    plane = s["labels"] == 1
    bad = s["bad"] != GOOD
    e = s["e"].astype(np.float64)
    beyond = ~plane & (bad | ~(np.abs(e) <= float(np.float32(gate))))
    outside = ~plane & ~beyond & ~((j >= 0) & (j < n_stations))
    cls = np.full(len(e), MAPPED, np.int8)
    cls[outside], cls[beyond], cls[plane] = OUTSIDE, BEYOND, PLANE
    m = cls == MAPPED
    assert np.all(s["sector"][m] < n_sectors)
    cell = np.full(len(e), -1, np.int64)
    cell[m] = j[m].astype(np.int64) * n_sectors + s["sector"][m]
    out = s["e"].copy()
    out[plane | bad] = np.nan
    return dict(e=out, cell=cell, cls=cls, counts=tuple(int((cls == c).sum()) for c in (MAPPED, OUTSIDE, BEYOND, PLANE)))


def same_points(res, cell, exp):
    """The device's per-point outputs against expected(): e bit for bit where it is finite, not finite where the row is
    bad (a NaN's payload is not stated), NaN for plane points; the cell index exactly."""
    res = np.asarray(res, np.float32)
    fin = np.isfinite(exp["e"])
    assert np.array_equal(np.isfinite(res), fin)
    assert np.array_equal(res[fin].view(np.uint32), exp["e"][fin].view(np.uint32))
    assert np.array_equal(np.asarray(cell, np.int64), exp["cell"])


def fillers(base, gate, n_stations, n_sectors, ds=0.25, t0=0.0):
    """One-row Specs of every class that has no cell: a plane-labelled point, a point beyond the gate (an exact residual
    above it; an infinite row when the gate is 8 and no base point lies beyond), a point in the first station past the
    grid, a NaN row."""
    one = spec(base, [0], stations_t(0, 0.5, ds, t0))
    plane = take(one, [0])
    plane["labels"][:] = 1
    far = beyond_points(gate, n_sectors)
    if len(far["e"]):
        beyond = spec(far, [len(far["e"]) // 2], stations_t(0, 0.5, ds, t0))
    else:
        beyond = take(one, [0])
        beyond["bad"][:] = POS_INF_ROW
    outside = spec(base, [1], stations_t(n_stations, 0.0, ds, t0))
    nan = take(one, [0])
    nan["bad"][:] = NAN_ROW
    return dict(plane=plane, beyond=beyond, outside=outside, nan=nan)


def sprinkle(s, fl):
    """Every class into a cloud of mapped points (in place): rows 3 mod 13 become plane-labelled, rows 5 mod 29 the
    outside filler, rows 7 mod 31 the beyond filler, rows 11 mod 37 the NaN row."""
    i = np.arange(len(s["t"]))
    s["labels"][i % 13 == 3] = 1
    for kind, m, r in (("outside", 29, 5), ("beyond", 31, 7), ("nan", 37, 11)):
        set_rows(s, i % m == r, {k: v[0] for k, v in fl[kind].items()})
    return s


# ---- per-wave cell patterns (a wave of the map kernels is 64 consecutive points, aligned to 64) ----

WAVE = 64
WHERE = [(a, b) for a in ("head", "middle", "tail") for b in ("head", "middle", "tail") if a != b]


def patterns(base, filler, n_stations, n_sectors, ds=0.25, t0=0.0):
    """dict name -> Spec.  base: base_points of the grid; filler: fillers() of the grid, the 'x' lanes.  Every run takes its points from one sector and one station; cells A, B, .. are
    (station, sector) pairs spread over the grid."""
    secs = [k for k in range(n_sectors) if (base["sector"] == k).sum() >= 3]
    assert secs
    cells = [((3 * i) % n_stations, secs[(7 * i) % len(secs)]) for i in range(64)]

    def run(ci, length, where=("head", "tail"), frac=0.25):
        j, k = cells[ci % len(cells)]
        return spec(base, run_indices(base, k, length, where), stations_t(j, frac, ds, t0))

    out = {}
    # 64 lanes of one cell, the extremes at every pair of places; three whole waves
    out["one_cell_per_wave"] = concat(*[run(i, WAVE, w) for i, w in enumerate(WHERE)])
    # a run that ends at lane 63 and goes on from lane 0 of the next wave (the merge must not cross the wave)
    out["across_waves"] = concat(run(0, 40), run(1, 24 + 10, ("tail", "head")), run(2, 54 + 64 + 5, ("middle", "tail")),
                                 run(3, 59, ("head", "middle")))
    # runs of length 1: A B A B
    a, b = run(4, 70, ("head", "tail")), run(5, 70, ("tail", "head"))
    ab = concat(a, b)
    order = np.arange(140).reshape(2, 70).T.reshape(-1)
    out["alternating"] = take(ab, order)
    # A A x x A A, x in turn every class that has no cell
    for kind, x in filler.items():
        parts = []
        for i, w in enumerate(WHERE):
            r = run(6, 2 + (i % 5), w)
            parts += [r, x, x] if i % 2 else [r, x]
        parts.append(run(6, 4))
        out["gap_" + kind] = concat(*parts)
    # a run from lane 0, short runs between, a run to lane 63, and the last wave cut inside a run
    out["head_and_tail_runs"] = concat(run(7, 9, ("tail", "head")), run(8, 1), run(9, 2), run(10, 3, ("middle", "head")),
                                       run(11, 49, ("middle", "tail")), run(12, 64 + 37, ("head", "tail")))
    # sums that cancel to 0 with count > 0
    parts = []
    for k in secs:
        c = cancelling_indices(base, k)
        if c is not None:
            j = (5 * len(parts)) % n_stations
            parts.append(spec(base, c, stations_t(j, 0.5, ds, t0)))
        if len(parts) == 4:
            break
    if parts:
        out["cancelling"] = concat(*parts)
    return out
