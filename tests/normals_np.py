"""Plain numpy twin of the neighbourhood kernel's PLAN (csrc/k_normals.hip, make_grid of csrc/gm_api.hip): no GPU, none
of the code under test.  It does not compute normals -- the C oracle does -- it says which tiles, windows, streams and
chunks a cloud reaches, so that a case table can assert the mechanism each case is there for, and it counts neighbours of
integer lattice clouds without any floating point.

grid          make_grid restated for the frame path (box [-bound, bound]^3, n = the frame's point count, bucketed as
              gm_process_frame buckets it): hr = float(radius) * 1.001f with its 1e-9 floor and the ext / 1023 clamp, D from
              rows_per_radius (the uniform-fill estimate times ten, D = 4 from 2 000; `rows` = GM_NORMALS_ROWS) and the
              loop that keeps <= 1024 rows per axis, ny / nz, fine (64, halved until the key fits 31 bits), nx, xreach,
              reach[a][b] (in double, as the host), r2 = float(radius * radius), r2_scale, snap, band = 2e-5f * hr * hr,
              dscale / dband.  Everything fp32 where the host code is fp32: numpy's fp32 arithmetic rounds every operation.
cell_keys     cell_coord / cell_key of csrc/gm_device.hpp: floorf((x - o) * inv) clamped to the grid, key = (cz ny + cy)
              nx + cx.
plan          the stable sort by key, the row table, the tile cutter (64-chunks counted from the row start; a chunk that
              spans more than span = 3 fine cell steps is cut again at aligned (span + 1)-cell groups; cost class from the
              tile's extent), per cutter block the number of 4096-position steps its backwards walk takes, and per tile
              what normals_tile_mxd derives before it streams: the windows of both 32-query groups in every row around the
              tile, the thin flag (group-0 windows sum < 64, usual grid only), the rows padded to octets, stream_total, the
              128-slot chunks and the slot at which each group's run of 32-candidate blocks starts inside each chunk
              (assemble_stream); for finer rows (D > 1) the passes of 32 rows and the chunks of <= 4 pieces
              (assemble_walk).
flann_d2      FLANN's L2_Simple in fp32: ((dx dx + dy dy) + dz dz), every operation rounded.
count_exact   neighbour counts of an integer cloud: sum d^2 < M in int64.  No floating point.
band_census   pairs of an integer cloud at d2 == M, inside the band (0 < |d2 - M| <= band) and just outside it (<= 4 band),
              in lattice units.
flann_is_exact  the fp32 chain reproduces the integer d2 of a lattice cloud and decides d2 < r2 as the integers do.
planted_lattice a lattice cloud with partners planted at integer offsets of squared length M - 2 .. M + 2: ties and
              near-ties by the thousand on a lattice too fine for them to come by chance.
The cloud makers and the case table of tests/test_gpu_normals_edges.py follow; tests/test_normals_reference.py asserts
on every CPU run that each case reaches what it is listed for.
"""
import collections
import functools
import math

import numpy as np

F = np.float32
TB_SPAN = 4096            # kTbSpan: sorted positions per cutter block, and per step of its backwards walk
TILE_Q = 64               # kTileQ
GROUP_Q = 32              # kMxGroupLanes
TILE_SPAN = 3             # kTileSpan
TILE_CLASSES = 8          # GM_TILE_CLASSES
MD_CHUNK = 128            # kMdChunk
MD_PIECES = 4             # kMdPieces
MIN_CANDIDATES = 64       # kMxMinCandidates


def size_bucket(n):
    """The capacity bucket a frame of n points runs in (gm_api.hip): multiples of max(1024, p2 / 16)."""
    if n == 0:
        return 0
    p2 = 1024
    while p2 < n:
        p2 <<= 1
    step = max(1024, p2 // 16)
    return (n + step - 1) // step * step


def _frexp_exp(x):
    return math.frexp(float(x))[1]


def grid(bound, radius, n, rows=None):
    lo = F(-bound)
    ext = F(bound) - lo
    assert ext.dtype == np.float32
    hr = F(radius) * F(1.001)
    if not hr > F(1e-9):
        hr = F(1e-9)
    if hr < ext / F(1023.0):
        hr = ext / F(1023.0)
    ns = size_bucket(n)
    if rows is not None:
        D = min(max(int(rows), 1), 4)
    else:
        vol = float(ext) * float(ext) * float(ext)
        k_est = 10.0 * float(ns) * (4.18879 * radius * radius * radius) / vol if vol > 0.0 and ns else 0.0
        D = 1 if k_est < 2000.0 else 4
    while D > 1 and hr / F(D) < ext / F(1023.0):
        D -= 1
    h = hr / F(D)
    inv_h = F(1.0) / h

    def dim(e, inv, cap):
        return min(max(int(np.floor(e * inv)) + 1, 1), cap)

    ny = nz = dim(ext, inv_h, 1024)
    inv_hr = F(1.0) / hr
    nxc = dim(ext, inv_hr, 1024)
    fine = 64
    while fine > 1 and ny * nz * (nxc * fine + fine) >= (1 << 31):
        fine >>= 1
    inv_hx = inv_hr * F(fine)
    nx = dim(ext, inv_hx, 1024 * fine)
    xreach = fine + 1
    reach = np.zeros((5, 5), np.int64)
    for a in range(5):
        for b in range(5):
            if a > D or b > D:
                continue
            gy = (a - 1) * float(h) if a > 1 else 0.0
            gz = (b - 1) * float(h) if b > 1 else 0.0
            w2 = radius * radius - gy * gy - gz * gz
            if w2 <= 0.0:
                continue
            reach[a, b] = min(int(math.floor(math.sqrt(w2) * float(inv_hx) * (1.0 + 1e-6))) + 2, xreach)
    r2 = F(radius * radius)
    k = min(max(100 - _frexp_exp(r2 if r2 > 0 else 1.0), -100), 126)
    cmax = max(abs(float(lo)), abs(float(lo + ext)))
    snap = math.ldexp(1.0, max(_frexp_exp(max(cmax, 1e-30)) - 24, -120))
    band = F(2.0e-5) * hr * hr
    assert band.dtype == np.float32 and inv_hx.dtype == np.float32
    dscale = math.ldexp(1.0, min(_frexp_exp(F(1.0) / band), 60))
    return dict(lo=lo, ext=ext, hr=hr, D=D, h=h, inv_h=inv_h, inv_hx=inv_hx, nx=nx, ny=ny, nz=nz, fine=fine, xreach=xreach,
                span=TILE_SPAN * fine, reach=reach, r2=r2, r2_scale=math.ldexp(1.0, k), snap=snap, band=band, dscale=dscale,
                dband=float(band) * dscale, ns=ns)


def cell_coords(xyz, g):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)

    def cc(v, inv, n):
        t = (v - g["lo"]) * inv
        assert t.dtype == np.float32
        return np.clip(np.floor(t).astype(np.int64), 0, n - 1)

    return cc(xyz[:, 0], g["inv_hx"], g["nx"]), cc(xyz[:, 1], g["inv_h"], g["ny"]), cc(xyz[:, 2], g["inv_h"], g["nz"])


def cell_keys(xyz, g):
    cx, cy, cz = cell_coords(xyz, g)
    key = (cz * g["ny"] + cy) * g["nx"] + cx
    assert key.max(initial=0) < (1 << 31)
    return key.astype(np.uint32)


def _pad8(x):
    return (x + 7) & ~7


def plan(xyz, bound, radius, rows=None):
    """A dict: g, n, order (sorted position -> input row), skeys, rows {x-row: (begin, end)}, back_steps [cutter block],
    tiles [dict per tile, in position order]."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = len(xyz)
    assert (np.abs(xyz) <= F(bound)).all(), "the cases keep every point inside the box"
    g = grid(bound, radius, n, rows)
    nx, D = g["nx"], g["D"]
    key = cell_keys(xyz, g).astype(np.int64)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    row, fx = sk // nx, sk % nx
    rs = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
    re = np.r_[rs[1:], n]
    rb = {int(row[a]): (int(a), int(b)) for a, b in zip(rs, re)}
    # ---- the cutter's backwards walk: steps of TB_SPAN positions until the start of the row running into the block
    back = []
    for base in range(0, n, TB_SPAN):
        start = int(rs[np.searchsorted(rs, base, "right") - 1])
        back.append(0 if start == base else -(-(base - start) // TB_SPAN))
    # ---- tiles
    cuts = []
    group = g["span"] + 1
    for a, b in zip(rs, re):
        for c0 in range(a, b, TILE_Q):
            c1 = min(c0 + TILE_Q, b)
            if fx[c1 - 1] - fx[c0] > g["span"]:
                gi = fx[c0:c1] // group
                st = np.flatnonzero(np.r_[True, gi[1:] != gi[:-1]])
                en = np.r_[st[1:], c1 - c0]
                cuts += [(c0 + s, c0 + e, True) for s, e in zip(st, en)]
            else:
                cuts.append((c0, c1, False))
    side = 2 * D + 1
    tiles = []
    for s, e, sparse in cuts:
        qn = e - s
        r0 = int(row[s])
        cy0, cz0 = r0 % g["ny"], r0 // g["ny"]
        c8 = int(fx[e - 1] - fx[s]) * TILE_CLASSES // group
        ngroups = 2 if qn > GROUP_Q else 1
        lanes = np.r_[fx[s:e], np.full(TILE_Q - qn, fx[e - 1])]       # lanes past qn repeat the last query
        wb = np.zeros((side * side, 2), np.int64)
        we = np.zeros((side * side, 2), np.int64)
        for r in range(side * side):
            a, b = r % side - D, r // side - D
            yy, zz = cy0 + a, cz0 + b
            reach = int(g["reach"][abs(a), abs(b)]) if D > 1 else g["xreach"]
            if reach <= 0 or not (0 <= yy < g["ny"] and 0 <= zz < g["nz"]) or (zz * g["ny"] + yy) not in rb:
                continue                                                # (both ends at 0: an empty window)
            p, q = rb[zz * g["ny"] + yy]
            for gg in range(2):
                lo = max(int(lanes[GROUP_Q * gg]) - reach, 0)
                hi = min(int(lanes[GROUP_Q * gg + GROUP_Q - 1]) + reach, nx - 1)
                wb[r, gg] = p + np.searchsorted(fx[p:q], lo, "left")
                we[r, gg] = p + np.searchsorted(fx[p:q], hi + 1, "left")
        t = dict(s=int(s), qn=int(qn), row=r0, sparse=bool(sparse), cls=TILE_CLASSES - 1 - min(c8, TILE_CLASSES - 1),
                 ngroups=ngroups, wb=wb, we=we, len0=(we[:, 0] - wb[:, 0]).tolist(), len1=(we[:, 1] - wb[:, 1]).tolist())
        rlen = we[:, ngroups - 1] - wb[:, 0]                            # a row's window, all groups of the tile
        assert (rlen >= 0).all()
        t["row_len"] = rlen.tolist()
        if D == 1:
            t["thin"] = int(sum(t["len0"])) < MIN_CANDIDATES
            padded = _pad8(rlen)
            S = np.r_[0, np.cumsum(padded)]
            t["padded"] = padded.tolist()
            t["stream_total"] = total = int(S[-1])
            t["chunks"] = 0 if t["thin"] else -(-total // MD_CHUNK)
            starts = []                                                  # [chunk][group]: n_lo, None when no window reaches in
            for c0 in range(0, total if not t["thin"] else 0, MD_CHUNK):
                per = []
                for gi in range(ngroups):
                    gb, ge = S[:-1] + (wb[:, gi] - wb[:, 0]), S[:-1] + (we[:, gi] - wb[:, 0])
                    cb, ce = np.maximum(gb, c0), np.minimum(ge, c0 + MD_CHUNK)
                    hit = np.flatnonzero(ce > cb)
                    per.append(int((cb[hit[0]] & ~7) - c0) if len(hit) else None)
                starts.append(per)
            t["run_start"] = starts
            t["passes"] = 1
        else:                                                            # assemble_walk: <= 4 pieces per chunk
            t["thin"] = False
            t["passes"] = -(-side * side // 32)
            chunks, slots, pieces, most = 0, 0, 0, 0
            for L in rlen:
                L = int(L)
                while L > 0:
                    take = min(L, MD_CHUNK - slots)
                    slots += _pad8(take)
                    L -= take
                    pieces += 1
                    if slots >= MD_CHUNK or pieces == MD_PIECES:
                        chunks, most, slots, pieces = chunks + 1, max(most, pieces), 0, 0
            if slots:
                chunks, most = chunks + 1, max(most, pieces)
            t["chunks"], t["max_pieces"] = chunks, most
        tiles.append(t)
    return dict(g=g, n=n, order=order, skeys=sk.astype(np.uint32), rows=rb, back_steps=back, tiles=tiles)


def summary(p):
    """What a plan reaches, as plain numbers and sets (the mechanism keys of the case table are tested on these)."""
    T, g = p["tiles"], p["g"]
    mx = [t for t in T if not t["thin"]]
    out = dict(D=g["D"], n=p["n"], tiles=len(T), thin_tiles=len(T) - len(mx), chunks=sum(t["chunks"] for t in T),
               back_steps=max(p["back_steps"]), qn=sorted({t["qn"] for t in T}), mfma_qn=sorted({t["qn"] for t in mx}),
               classes=sorted({t["cls"] for t in T}), sparse_tiles=sum(t["sparse"] for t in T),
               row_starts=sorted(a for a, _ in p["rows"].values()), row_ends=sorted(b for _, b in p["rows"].values()),
               ngroups=sorted({t["ngroups"] for t in mx}), passes=max(t["passes"] for t in T),
               min_window0=min(sum(t["len0"]) for t in T), chunk_counts=sorted({t["chunks"] for t in mx}))
    if g["D"] == 1:
        out["staged_slots"] = sum(t["stream_total"] for t in mx)
        out["total_mod128"] = sorted({t["stream_total"] % MD_CHUNK for t in mx})
        out["len_mod8"] = sorted({L % 8 for t in mx for L in t["row_len"] if L})
        # where a row's LAST candidate sits against the chunk grid: its slot + 1 (the row's unpadded end in the stream)
        out["row_end_mod128"] = sorted({(sum(t["padded"][:k]) + L) % MD_CHUNK for t in mx for k, L in enumerate(t["row_len"]) if L})
        occ = [[L > 0 for L in t["row_len"]] for t in mx]
        out["empty_first"] = any(not o[0] and any(o) for o in occ)
        out["empty_last"] = any(not o[-1] and any(o) for o in occ)
        out["empty_middle"] = any(not o[k] and any(o[:k]) and any(o[k + 1:]) for o in occ for k in range(1, len(o) - 1))
        runs = [s for t in mx for per in t["run_start"] for s in per if s is not None]
        out["max_run_start"] = max(runs, default=-1)
        # blocks with tiles of several cost classes, and a sparse chunk's group edge on a cutter-block edge
        per_block = collections.defaultdict(set)
        for t in T:
            per_block[t["s"] // TB_SPAN].add(t["cls"])
        out["classes_in_a_block"] = max(len(v) for v in per_block.values())
        out["group_edge_on_block_edge"] = any(t["sparse"] and t["s"] % TB_SPAN == 0 and t["s"] > 0 for t in T)
    else:
        out["max_pieces"] = max(t["max_pieces"] for t in T)
    return out


# ---------------------------------------------------------------- exact references of the neighbour predicate

def flann_d2(q, c):
    """[len(q), len(c)] fp32 squared distances in FLANN's L2_Simple order, every product and sum rounded."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    dx, dy, dz = (c[None, :, k] - q[:, None, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def _windows(P, M, step=256):
    """(rows a:b of the x-sorted cloud, the candidate range lo:hi that holds every pair with d2 < 4 M, their int64 d2)."""
    P = np.ascontiguousarray(P, dtype=np.int64)
    assert np.abs(P).max() < (1 << 30)
    reach = math.isqrt(4 * int(M)) + 1
    x = P[:, 0]
    for a in range(0, len(P), step):
        b = min(a + step, len(P))
        lo, hi = np.searchsorted(x, x[a] - reach, "left"), np.searchsorted(x, x[b - 1] + reach, "right")
        d = P[a:b, None, :] - P[None, lo:hi, :]
        yield a, b, lo, hi, (d * d).sum(-1)


def _by_x(P_int):
    P = np.ascontiguousarray(P_int, dtype=np.int64)
    order = np.argsort(P[:, 0], kind="stable")
    return P[order], order


def count_exact(P_int, M):
    """Neighbours of every point of an integer cloud, the point itself included: sum d^2 < M in int64 (pairs further apart
    than 2 sqrt(M) in x alone are not looked at)."""
    P, order = _by_x(P_int)
    out = np.empty(len(P), np.int32)
    for a, b, _, _, d2 in _windows(P, M):
        out[order[a:b]] = (d2 < int(M)).sum(axis=1)
    return out


def band_census(P_int, M, g, u):
    """(ties, in_band, near): ordered pairs with d2 == M, with 0 < |d2 - M| <= band, with band < |d2 - M| <= 4 band; the
    band of grid g in lattice units of u^2."""
    P, _ = _by_x(P_int)
    band = float(g["band"]) / (u * u)
    assert 4 * band < M
    ties = inb = near = 0
    for _, _, _, _, d2 in _windows(P, M):
        off = np.abs(d2 - int(M))
        ties += int((off == 0).sum())
        inb += int(((off > 0) & (off <= band)).sum())
        near += int(((off > band) & (off <= 4 * band)).sum())
    return ties, inb, near


def flann_is_exact(P_int, u, M, below=None):
    """The fp32 chain on the cloud P u reproduces the integer d2 on every pair with d2 < below (4 M unless given), and
    decides d2 < M u^2 as the integers do on every pair looked at."""
    below = 4 * M if below is None else below
    P, _ = _by_x(P_int)
    X = (P * u).astype(np.float32)
    r2 = F(M * u * u)
    if not np.array_equal(X.astype(np.float64) / u, P) or float(r2) != M * u * u:
        return False
    for a, b, lo, hi, d2 in _windows(P, M):
        f32 = flann_d2(X[a:b], X[lo:hi])
        f = f32.astype(np.float64) / (u * u)
        if not np.array_equal(f[d2 < below], d2[d2 < below]) or not np.array_equal(f32 < r2, d2 < M):
            return False
    return True


def radius_for_r2(r2):
    """A double radius with float32(radius * radius) == r2 (searched around sqrt(r2))."""
    r2 = F(r2)
    r = math.sqrt(float(r2))
    for _ in range(64):
        got = F(r * r)
        if got == r2:
            return r
        r = math.nextafter(r, math.inf if got < r2 else 0.0)
    raise AssertionError("no double squares to this float")


# ---------------------------------------------------------------- cloud makers (seeded)

Y0 = Z0 = -0.045          # a y / z cell centre of the r = 0.1 grid over the +-5 box (cell 49 of 100)
R01 = 0.1


def _shuffled(parts, rng):
    xyz = np.vstack(parts).astype(np.float32)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


def _row(x, rng, dy=0.0, dz=0.0):
    """Points of one x-row of the r = 0.1 grid: y within +-0.03 and z within +-0.003 of a cell centre (a thin ribbon: its
    normal is well defined), dy / dz cells of 0.1 away from the middle row."""
    m = len(x)
    return np.stack([x, Y0 + dy + rng.uniform(-0.03, 0.03, m), Z0 + dz + rng.uniform(-0.003, 0.003, m)], axis=1)


def ribbon(p, L, seed, after=False):
    """L points in one x-row, x uniform in +-4.8, behind (after: in front of) a filler row of p points one cell away in z:
    the ribbon's row starts at sorted position p (after: 0) and runs over several cutter blocks."""
    rng = np.random.default_rng(seed)
    parts = [_row(rng.uniform(-4.8, 4.8, L), rng)]
    if p:
        parts.append(_row(rng.uniform(-4.8, 4.8, p), rng, dz=0.1 if after else -0.1))
    return _shuffled(parts, rng)


def sized_row(q, seed):
    """A row of exactly q points within 0.06 in x, between two rows of 90 points each over the same stretch (y cells either
    side), so that every tile's group-0 windows hold >= 64 candidates: the matrix-core path at every q."""
    rng = np.random.default_rng(seed)
    return _shuffled([_row(rng.uniform(1.0, 1.06, q), rng), _row(rng.uniform(0.98, 1.08, 90), rng, dy=-0.1),
                      _row(rng.uniform(0.98, 1.08, 90), rng, dy=0.1)], rng)


def comb(p, clumps, seed):
    """A row of clumps of 40 points every 2.5 r in x (64-chunks there span more than 3 r and are cut again at cell groups),
    a dense row beside it, p filler points in front."""
    rng = np.random.default_rng(seed)
    cx = -4.5 + 2.5 * R01 * np.arange(clumps)
    x = (cx[:, None] + rng.uniform(-0.01, 0.01, (clumps, 40))).reshape(-1)
    parts = [_row(x, rng), _row(rng.uniform(-4.8, 4.8, 3000), rng, dy=0.1)]
    if p:
        parts.append(_row(rng.uniform(-4.8, 4.8, p), rng, dz=-0.1))
    return _shuffled(parts, rng)


def cluster(N, seed):
    rng = np.random.default_rng(seed)
    return (np.array([1.0, 2.0, -3.0]) + rng.uniform(-0.02, 0.02, (N, 3))).astype(np.float32)


def lattice_rows(step, counts, seed):
    """Three adjacent rows (y cells) of points ON an exact x-lattice of spacing `step` (a binary fraction), counts[k] points
    in row k starting at x = -2: window lengths are then arithmetic in the spacing."""
    rng = np.random.default_rng(seed)
    assert step == 2.0 ** round(math.log2(step))
    parts = [_row(-2.0 + step * np.arange(c), rng, dy=0.1 * (k - 1)) for k, c in enumerate(counts)]
    return _shuffled(parts, rng)


def tunnel_n(n, seed):
    """synth.tunnel_frame cropped to exactly n points inside the +-5 box."""
    from geometric_mapping_amd import synth
    xyz = synth.tunnel_frame(n + n // 2 + 64, seed=seed)
    xyz = xyz[(np.abs(xyz) <= F(5.0)).all(axis=1)][:n]
    assert len(xyz) == n
    return np.ascontiguousarray(xyz)


def tie_lattice(q, n, seed, scale=1):
    """(P, u): n integer points uniform in a 2 x 1 x 0.125 slab at (3, -4.5, 2), in units of u = 2^-q (times scale)."""
    rng = np.random.default_rng(seed)
    k = 1 << q
    P = np.stack([rng.integers(0, 2 * k, n), rng.integers(0, k, n), rng.integers(0, k // 8, n)], axis=1).astype(np.int64)
    return P + np.array([3 * k, -9 * k // 2, 2 * k]), (2.0 ** -q) * scale


# ---------------------------------------------------------------- the case table

TIE_N = 6000
# q -> M of the tie clouds: radius sqrt(M) 2^-q.  q = 7: the band is 0.02 lattice units, M = 1034 is rich in three-square
# representations (thousands of pairs at exactly d2 == r2); q = 10 / 12, M near (0.25 / u)^2: one lattice step is 0.76 /
# 0.05 of the band, so pairs sit inside the band without being ties.
# q = 14: a lattice too fine for the matrix-core product to be exact on (offsets from a tile's origin have 13 and more
# bits, their squares round), M just below 2^24 so that FLANN's own chain -- differences of NEIGHBOURS, 12 bits -- still is
# exact up to the threshold; near-ties do not come by chance at this resolution, they are planted (planted_lattice).
TIE_M = {7: 1034, 10: 66049, 12: 1048577, 14: (1 << 24) - 1213}      # (M = 3 mod 8: M - 2 .. M + 2 are all sums of three squares)
PLANTED = (14,)


def planted_lattice(q, M, n_base, seed, deltas=(-2, -1, 0, 1, 2)):
    """(P, u): n_base lattice points in the slab of tie_lattice, each with a partner at an integer offset (a, b, c) with
    a^2 + b^2 + c^2 = M + delta, delta drawn from `deltas` (partners that would leave the slab are dropped): thousands of
    pairs AT and within two lattice steps OF the threshold, whatever the lattice's resolution."""
    rng = np.random.default_rng(seed)
    base, u = tie_lattice(q, n_base, seed)
    k = 1 << q
    lo, hi = np.array([3 * k, -9 * k // 2, 2 * k]), np.array([5 * k, -7 * k // 2, 2 * k + k // 8])
    vecs = []
    a, c = np.meshgrid(np.arange(0, math.isqrt(M) + 1, dtype=np.int64), np.arange(0, k // 32, dtype=np.int64), indexing="ij")
    for d in deltas:
        s = (M + d) - a * a - c * c
        b = np.sqrt(np.maximum(s, 0).astype(np.float64)).astype(np.int64)       # (s < 2^53: the root of a square is exact)
        ok = (s >= 0) & (b * b == s)
        vecs.append(np.stack([a[ok], b[ok], c[ok]], axis=1))
        assert len(vecs[-1]) >= 100 and ((vecs[-1] ** 2).sum(axis=1) == M + d).all()
    pick = rng.integers(0, len(deltas), n_base)
    v = np.stack([vecs[j][rng.integers(0, len(vecs[j]))] for j in pick]) * rng.choice([-1, 1], (n_base, 3))
    swap = rng.random(n_base) < 0.5                                           # a <-> b: the offsets point every way in x / y
    v[swap] = v[swap][:, [1, 0, 2]]
    partner = base + v
    inside = ((partner >= lo) & (partner < hi)).all(axis=1)
    return np.vstack([base, partner[inside]]), u


@functools.lru_cache(maxsize=None)
def tie_points(q):
    P, u = planted_lattice(q, TIE_M[q], TIE_N // 2 + 600, seed=q) if q in PLANTED else tie_lattice(q, TIE_N, seed=q)
    P.setflags(write=False)
    return P, u


@functools.lru_cache(maxsize=None)
def near_tie_pairs(q, k=2):
    """Ordered pairs of the tie cloud q with |d2 - M| <= k lattice steps."""
    P, _ = _by_x(tie_points(q)[0])
    return sum(int((np.abs(d2 - TIE_M[q]) <= k).sum()) for _, _, _, _, d2 in _windows(P, TIE_M[q]))


@functools.lru_cache(maxsize=None)
def tie_counts(q, up):
    """count_exact of the tie cloud q; up: with r2 one ulp above M u^2, i.e. d2 <= M (an ulp of M u^2 is at most u^2 while
    M < 2^24: the raised threshold does not pass (M + 1) u^2)."""
    assert TIE_M[q] < (1 << 24)
    c = count_exact(tie_points(q)[0], TIE_M[q] + (1 if up else 0))
    c.setflags(write=False)
    return c


def _tie_case(q, up=False, scale=1):
    P, u = tie_points(q)
    u = u * scale
    M = TIE_M[q]
    r2 = F(M * u * u)
    assert float(r2) == M * u * u
    if up:
        r2 = np.nextafter(r2, F(np.inf))
    radius = radius_for_r2(r2)                  # (sqrt(M) u itself where that squares back to r2)
    assert F(radius * radius) == r2 and (up or q in PLANTED or radius == math.sqrt(M) * u)
    X = (P * u).astype(np.float32)
    assert np.array_equal(X.astype(np.float64) / u, P)
    return X, radius


Case = collections.namedtuple("Case", "make bound radius mech tie")
Case.__new__.__defaults__ = (None,)
CASES = {}
for _p, _L in ((0, 8193), (4095, 8194), (4096, 8192), (4097, 12289)):
    CASES[f"ribbon_p{_p}_L{_L}"] = Case(functools.partial(ribbon, _p, _L, _p + _L), 5.0, R01, {
        (0, 8193): {"back_2", "row_start_0", "long_row_ends_at_n", "misalign_0", "tile_of_1"},
        (4095, 8194): {"back_3", "row_start_base_minus_1", "walk_hit_past_trip_edge", "misalign_63", "long_row_ends_at_n",
                       "row_end_mod128_0", "row_end_mod128_1", "row_end_mod128_127", "empty_first", "empty_middle", "empty_last"},
        (4096, 8192): {"row_start_base", "walk_hit_on_trip_edge", "misalign_0", "long_row_ends_at_n", "stream_total_mod128_0"},
        (4097, 12289): {"back_3", "row_start_base_plus_1", "misalign_1", "long_row_ends_at_n", "chunks_4plus", "len_mod8_0",
                        "len_mod8_1", "len_mod8_7"}}[(_p, _L)])
CASES["ribbon_first_L8193"] = Case(functools.partial(ribbon, 4000, 8193, 5, True), 5.0, R01,
                                   {"back_2", "row_start_0", "long_row_ends_inside"})
for _q in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129):
    CASES[f"row_q{_q}"] = Case(functools.partial(sized_row, _q, 100 + _q), 5.0, R01,
                               {f"mfma_tile_of_{1 if _q in (65, 129) else (63 if _q == 127 else min(_q, 64))}",
                                "ngroups_1" if _q <= 32 else "ngroups_2"})
CASES["comb_p0"] = Case(functools.partial(comb, 0, 30, 7), 5.0, R01, {"sparse_chunk_cut", "classes_in_a_block_3"})
CASES["comb_p3976"] = Case(functools.partial(comb, 3976, 30, 7), 5.0, R01,
                           {"sparse_chunk_cut", "classes_in_a_block_3", "group_edge_on_block_edge", "run_start_120"})
for _n in (4095, 4096, 4097, 8191, 8192, 8193, 16385):
    CASES[f"tunnel_n{_n}"] = Case(functools.partial(tunnel_n, _n, _n), 5.0, 0.3, {f"n_{_n}"})
for _e, _counts in ((9, (700, 900, 800)), (10, (700, 900, 800)), (10, (1500, 1400, 1300))):
    CASES[f"lattice_2^-{_e}_{_counts[0]}"] = Case(functools.partial(lattice_rows, 2.0 ** -_e, _counts, _e), 5.0, R01,
                                                  {"chunks_2", "chunks_4plus"} | ({"chunks_1"} if (_e, _counts[0]) == (10, 700) else set()))
for _N in (63, 64, 65):
    CASES[f"cluster_{_N}"] = Case(functools.partial(cluster, _N, _N), 5.0, R01, {f"window_sum_{_N}"})
for _q in (7, 10, 12, 14):
    for _up in (False, True):
        CASES[f"tie_q{_q}" + ("_up" if _up else "")] = Case(
            functools.partial(_tie_case, _q, _up), 5.0, None,
            {7: {"ties_1000"}, 14: {"in_band_40", "near_ties_planted_1000"}}.get(_q, {"in_band_40"}) | {"no_thin_tile"}, (_q, _up))
CASES["tie_q10_x1024"] = Case(functools.partial(_tie_case, 10, False, 1024), 5120.0, None, {"in_band_40", "no_thin_tile"}, (10, False))
# (case, GM_NORMALS_ROWS) on contexts of their own; (case) as the second frame of a graph context
FINE_VARIANTS = [(c, d) for c in ("ribbon_p4097_L12289", "tie_q7", "tie_q12", "tie_q14", "row_q33") for d in (2, 4)]
GRAPH_VARIANTS = ["ribbon_p4095_L8194", "tie_q10"]
ALL_MECH = sorted(set().union(*(c.mech for c in CASES.values())) | {"fine_D2", "fine_D4", "fine_passes_3", "fine_pieces_4"})


@functools.lru_cache(maxsize=None)
def case(name):
    """(cloud, radius) of a case, made once and left unchanged."""
    c = CASES[name]
    made = c.make()
    xyz, radius = made if isinstance(made, tuple) else (made, c.radius)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    xyz.setflags(write=False)
    return xyz, float(radius)


@functools.lru_cache(maxsize=None)
def case_plan(name, rows=None):
    xyz, radius = case(name)
    p = plan(xyz, CASES[name].bound, radius, rows)
    return p, summary(p)


@functools.lru_cache(maxsize=None)
def case_census(name):
    """(ties, in_band, near) of a tie case, None for the others."""
    c = CASES[name]
    if c.tie is None:
        return None
    q, _ = c.tie
    P, u = tie_points(q)
    _, radius = case(name)
    u = u * (c.bound / 5.0)                    # (the scaled cloud: same integers, a larger unit)
    return band_census(P, TIE_M[q], case_plan(name)[0]["g"], u)


def reached(name, rows=None):
    """The mechanism keys (ALL_MECH) that the twin says a case reaches."""
    p, s = case_plan(name, rows)
    out = set()
    if s["D"] > 1:
        out.add(f"fine_D{s['D']}")
        if s["passes"] == 3:
            out.add("fine_passes_3")
        if s["max_pieces"] == MD_PIECES:
            out.add("fine_pieces_4")
        return out
    n, rows_ = p["n"], p["rows"]
    long_rows = [(a, b) for a, b in rows_.values() if b - a > TB_SPAN]
    out |= {f"back_{k}" for k in (2, 3) if s["back_steps"] >= k}
    for a, b in long_rows:
        out |= {"row_start_0"} if a == 0 else set()
        out |= {"row_start_base_minus_1"} if a > 0 and a % TB_SPAN == TB_SPAN - 1 else set()
        out |= {"row_start_base"} if a > 0 and a % TB_SPAN == 0 else set()
        out |= {"row_start_base_plus_1"} if a % TB_SPAN == 1 else set()
        out |= {"long_row_ends_at_n"} if b == n else {"long_row_ends_inside"}
        out |= {f"misalign_{a % TILE_Q}"} if a % TILE_Q in (0, 1, 63) else set()
        # the walk's hit against the 4096-position groups it reads: the row start is the lowest position of a trip, or the
        # highest of the next one
        for base in range(0, n, TB_SPAN):
            if a < base < b:
                out |= {"walk_hit_on_trip_edge"} if (base - a) % TB_SPAN == 0 else set()
                out |= {"walk_hit_past_trip_edge"} if (base - a) % TB_SPAN == 1 else set()
    mx = [t for t in p["tiles"] if not t["thin"]]
    out |= {f"mfma_tile_of_{t['qn']}" for t in mx if t["qn"] in (1, 2, 31, 32, 33, 63, 64)}
    out |= {"tile_of_1"} if 1 in s["qn"] else set()
    out |= {f"ngroups_{k}" for k in s["ngroups"]}
    out |= {"sparse_chunk_cut"} if s["sparse_tiles"] and any(t["sparse"] for t in mx) else set()
    out |= {"classes_in_a_block_3"} if s["classes_in_a_block"] >= 3 else set()
    out |= {"group_edge_on_block_edge"} if s["group_edge_on_block_edge"] else set()
    out |= {"run_start_120"} if s["max_run_start"] >= 120 else set()
    out |= {f"n_{n}"} if CASES[name].radius == 0.3 else set()
    out |= {"stream_total_mod128_0"} if 0 in s["total_mod128"] else set()
    out |= {f"row_end_mod128_{m}" for m in (0, 1, 127) if m in s["row_end_mod128"]}
    out |= {f"len_mod8_{m}" for m in (0, 1, 7) if m in s["len_mod8"]}
    out |= {k for k in ("empty_first", "empty_middle", "empty_last") if s[k]}
    out |= {f"chunks_{k}" for k in (1, 2) if k in s["chunk_counts"]}
    out |= {"chunks_4plus"} if any(k >= 4 for k in s["chunk_counts"]) else set()
    if name.startswith("cluster_"):
        w = {sum(t["len0"]) for t in p["tiles"]}
        thin = {t["thin"] for t in p["tiles"]}
        if w == {n} and thin == {n < MIN_CANDIDATES}:
            out.add(f"window_sum_{n}")
    if CASES[name].tie is not None:
        ties, inb, _ = case_census(name)
        out |= {"ties_1000"} if ties >= 1000 else set()
        out |= {"in_band_40"} if inb >= 40 else set()
        out |= {"no_thin_tile"} if s["thin_tiles"] == 0 else set()
        out |= {"near_ties_planted_1000"} if CASES[name].tie[0] in PLANTED and near_tie_pairs(CASES[name].tie[0]) >= 1000 else set()
    return out
