"""Plain numpy references of the binning chain (csrc/k_sort.hip, gm_compact.hpp, k_voxel.hip, k_nearest.hip): no GPU,
none of the code under test.

voxel_twin     pcl::VoxelGrid restated on its own: fp32 inverse leaf, the int64 overflow guard, min_b / div_b from the
               cloud's own extent, key = i0 + i1 dx + i2 dx dy with ik = int(floorf(p inv) - float(min_b)), a stable
               sort, one centroid per run of equal keys (fp64 sum in ascending (key, index) order, divided once, cast
               to fp32).
nearest_brute  exhaustive 1-NN, fp32 distances in FLANN's L2_Simple order with every operation rounded, first minimum.
lattice_cloud  points whose coordinates are exact binary fractions (cell + j / 256) * leaf, leaf a power of two: every
               coordinate is a multiple of leaf / 256 far below 2^24 of them, so an fp64 sum of all n coordinates is
               exact in ANY order (n * max|x| / (leaf / 256) < 2^53 is asserted) and a centroid is one fp64 division
               and one cast whatever the summation order was.  On such clouds every correct implementation of the
               voxel grid gives the same bits: the comparison needs no tolerance.
expected_plan  the sort plan a cloud reaches through gm_voxel_grid (voxel_key_bits and radix_plan restated), so a test's
               case table can assert that a case reaches the plan it is there for.
tests/test_binning_reference.py checks them against the C restatement on every CPU run.
"""
import numpy as np

INT32_MAX = 2147483647
RS_ITEMS = 8                 # keys a lane holds: tile = threads * RS_ITEMS (csrc/k_sort.hip)
RS_WINDOW_MIN = 112          # kRsWindow
RS_MAX_BITS = 9
# S -> (key bits, passes, digit bits, passthrough) of an S x S x S lattice_cloud at leaf 0.25: d = S + 1, bits_for(d^3).
# 1290: d^3 > INT32_MAX (a 32-bit plan) but the guard's 1290^3 is not; 1291: PCL's overflow guard, keys = row indices
LATTICE_PLANS = {1: (3, 1, 8, False), 5: (8, 1, 8, False), 6: (9, 1, 9, False), 39: (16, 2, 8, False), 40: (17, 2, 9, False),
                 79: (19, 3, 8, False), 511: (27, 3, 9, False), 1023: (30, 4, 8, False), 1289: (31, 4, 8, False),
                 1290: (32, 4, 8, False), 1291: (32, 4, 8, True)}


def voxel_keys(xyz, leaf):
    """(key per point as uint32, passthrough, (dx, dy, dz) of the overflow guard).  On passthrough the keys are the
    row indices."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    assert xyz.ndim == 2 and xyz.shape[1] == 3 and len(xyz) > 0
    one = np.float32(1.0)
    inv = one / np.float32(leaf)
    assert inv.dtype == np.float32
    mn, mx = xyz.min(axis=0), xyz.max(axis=0)
    ext = (mx - mn) * inv                                       # fp32, as PCL computes it
    assert ext.dtype == np.float32
    d = [int(np.int64(e)) + 1 for e in ext]                     # (C truncation of a non-negative float)
    if d[0] * d[1] * d[2] > INT32_MAX:                          # "Leaf size is too small": python ints cannot overflow
        return np.arange(len(xyz), dtype=np.uint32), True, tuple(d)
    min_b = np.floor(mn * inv).astype(np.int32)
    max_b = np.floor(mx * inv).astype(np.int32)
    div_b = (max_b - min_b + 1).astype(np.int64)
    cell = np.floor(xyz * inv) - min_b.astype(np.float32)       # fp32 floor, fp32 subtraction
    assert cell.dtype == np.float32
    ijk = cell.astype(np.int32).astype(np.int64)
    key = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * (div_b[0] * div_b[1])
    return (key & 0xFFFFFFFF).astype(np.uint32), False, tuple(d)


def voxel_twin(xyz, leaf):
    """(centroids [V,3] fp32, counts [V] int32, keys [V] uint32 ascending, passthrough).  Passthrough: the input rows in
    input order, counts 1."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if len(xyz) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32), False
    key, passthrough, _ = voxel_keys(xyz, leaf)
    if passthrough:
        return xyz.copy(), np.ones(len(xyz), np.int32), key, True
    order = np.argsort(key, kind="stable")
    skey = key[order]
    head = np.flatnonzero(np.concatenate(([True], skey[1:] != skey[:-1])))
    count = np.diff(np.concatenate((head, [len(xyz)])))
    seg = np.repeat(np.arange(len(head)), count)                # voxel of every sorted position
    pts = xyz[order].astype(np.float64)
    # np.bincount adds the weights one after the other in the order given: ascending (key, index), as PCL's loop over
    # the sorted index vector does
    sums = np.stack([np.bincount(seg, weights=pts[:, k], minlength=len(head)) for k in range(3)], axis=1)
    cen = (sums / count[:, None].astype(np.float64)).astype(np.float32)
    return cen, count.astype(np.int32), skey[head], False


def nearest_brute(xyz, queries, budget=1 << 22):
    """Index of the nearest point of every query, -1 without points.  d2 = ((dx dx + dy dy) + dz dz), each product and
    sum rounded to fp32 (numpy's fp32 arithmetic never contracts); np.argmin returns the first minimum."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    out = np.full(len(q), -1, np.int32)
    if len(xyz) == 0 or len(q) == 0:
        return out
    step = max(1, budget // len(xyz))
    for a in range(0, len(q), step):
        b = min(len(q), a + step)
        dx = q[a:b, None, 0] - xyz[None, :, 0]
        dy = q[a:b, None, 1] - xyz[None, :, 1]
        dz = q[a:b, None, 2] - xyz[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        out[a:b] = np.argmin(d2, axis=1)
    return out


def tied_share(xyz, queries, idx):
    """Share of the queries whose smallest fp32 distance is reached by more than one row."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    tied = 0
    for i in range(len(q)):
        d = q[i] - xyz
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        tied += int((d2 == d2[idx[i]]).sum() > 1)
    return tied / max(len(q), 1)


def tie_cloud(n, nq, rng):
    """(points [n,3], queries [nq,3]) for the 1-NN's tie rule.  Points have small-integer coordinates (about two rows
    per lattice site, in random row order), queries sit half-way between 2, 4 or 8 sites: every d2 is a multiple of 1/4
    far below 2^24 of them -- exact -- and most queries have several rows at exactly the smallest distance.  On top,
    where n allows, rows planted beside the lattice (sites that exist nowhere else), each with a query of its own:
      * a tied pair at rows 255 / 256 and at 4095 / 4096 (two LDS windows; two chunks);
      * four tied rows at 254, 257, 4094, 4097 (windows and chunks at once);
      * one site duplicated in rows of different chunks (100, 4100 and, beyond 8192 rows, n - 1), tied with a second
        site whose rows lie above them."""
    G = max(2, int(round((n / 2.0) ** (1.0 / 3.0))))
    xyz = rng.integers(0, G, size=(n, 3)).astype(np.float32)
    far = float(G + 2)
    forced = []

    def plant(rows_sites, query):
        for row, site in rows_sites:
            xyz[row] = site
        forced.append(query)

    if n > 4096:
        plant([(4095, (far + 1, 4, 0)), (4096, (far, 4, 0))], (far + 0.5, 4, 0))
    if n > 4097:
        plant([(254, (far, 6, 0)), (257, (far + 1, 6, 0)), (4094, (far, 7, 0)), (4097, (far + 1, 7, 0))], (far + 0.5, 6.5, 0))
    if n > 4200:
        rows = [(100, (far, 10, 0)), (4100, (far, 10, 0)), (4200, (far + 1, 10, 0))]
        if n > 8192:
            rows += [(n - 1, (far, 10, 0)), (8192, (far + 1, 10, 0))]
        plant(rows, (far + 0.5, 10, 0))
    if n > 256:
        plant([(255, (far + 1, 0, 0)), (256, (far, 0, 0))], (far + 0.5, 0, 0))
    q = rng.integers(0, max(G - 1, 1), size=(nq, 3)).astype(np.float32)
    axes = rng.integers(1, 4, size=nq)                                   # 1, 2 or 3 half-integer coordinates
    for i in range(nq):
        q[i, rng.permutation(3)[:axes[i]]] += 0.5
    m = min(nq, len(forced))
    if m:
        q[:m] = np.array(forced[:m], dtype=np.float32)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(q)


def eight_tie_cloud(nq, rng, n=8192, chunk=4096):
    """(points [n,3], queries [nq,3], rows of every query's eight tied points [nq,8]).  Query i sits in the centre of a
    unit cube of its own (cubes two apart); four of its corners lie in rows below `chunk`, four above, at random rows;
    the other rows are far away."""
    assert n == 2 * chunk and 4 * nq <= chunk and nq <= 1000
    xyz = np.empty((n, 3), np.float32)
    xyz[:] = (60.0, 60.0, 60.0)
    xyz += rng.integers(0, 8, size=(n, 3)).astype(np.float32)
    cube = 2.0 * np.stack(np.unravel_index(rng.permutation(1000)[:nq], (10, 10, 10)), axis=1).astype(np.float32)
    corner = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float32)
    rows = np.empty((nq, 8), np.int64)
    lo, hi = rng.permutation(chunk)[:4 * nq].reshape(nq, 4), chunk + rng.permutation(chunk)[:4 * nq].reshape(nq, 4)
    for i in range(nq):
        order = rng.permutation(8)
        rows[i, order[:4]], rows[i, order[4:]] = lo[i], hi[i]
        xyz[rows[i]] = cube[i] + corner
    return np.ascontiguousarray(xyz), np.ascontiguousarray(cube + 0.5), rows


def lattice_cloud(n, S, leaf, rng, cells=None, pin=True):
    """n points in an S[0] x S[1] x S[2] block of voxel cells (S: an int or three), cell (0, 0, 0) at the origin.
    Coordinates are (cell + j / 256) * leaf with integer j in [1, 63]: strictly inside the cell, exact in fp32.
    pin: rows 0 and 1 sit in the two opposite corner cells with j = 32, so the cloud's extent -- and with it the sort
    plan and the overflow guard -- is that of the block exactly (n = 1 has the first corner only).
    cells: [n, 3] integer cells instead of uniformly drawn ones (the pins still overwrite rows 0 and 1)."""
    S3 = np.broadcast_to(np.asarray(S, dtype=np.int64), (3,))
    lf = float(leaf)
    assert lf > 0 and np.log2(lf) == np.floor(np.log2(lf)), "leaf must be a power of two"
    if cells is None:
        cells = rng.integers(0, S3, size=(n, 3))
    cells = np.array(cells, dtype=np.int64).reshape(n, 3)
    assert (cells >= 0).all() and (cells < S3).all()
    j = rng.integers(1, 64, size=(n, 3))
    if pin and n > 0:
        cells[0], j[0] = 0, 32
        if n > 1:
            cells[1], j[1] = S3 - 1, 32
    x64 = (cells + j / 256.0) * lf
    xyz = x64.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), x64)                       # exact in fp32 ...
    assert n * (float(S3.max()) * 256.0) < 2.0 ** 53                         # ... and fp64 sums exact in any order
    return np.ascontiguousarray(xyz)


def bits_for(count):
    b = 1
    while (1 << b) < count and b < 32:
        b += 1
    return b


def expected_plan(xyz, leaf):
    """(key bits, passes, digit bits) of the sort gm_voxel_grid runs on this cloud: d = floor(max inv) - floor(min inv)
    + 2 over ALL coordinates, bits_for(d^3) (32 beyond INT32_MAX), passes = ceil(bits / 9), digit = max(8, ceil(bits /
    passes))."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    d = int(np.floor(float(xyz.max() * inv)) - np.floor(float(xyz.min() * inv))) + 2
    prod = d * d * d
    bits = 32 if prod > INT32_MAX else bits_for(prod)
    passes = (bits + RS_MAX_BITS - 1) // RS_MAX_BITS
    digit = max(8, (bits + passes - 1) // passes)
    return bits, passes, digit


def sort_shape(n, threads, digit):
    """(tiles, window, anchored tiles, anchors that are themselves anchored) of one pass over n items.  A tile sums the
    16-bit rows of the `window` tiles before it directly; tile t > window also reads the 32-bit inclusive row of tile
    t - window - 1 (k_rs_pass)."""
    tile = threads * RS_ITEMS
    tiles = (n + tile - 1) // tile
    groups = threads // ((1 << digit) // 8)
    window = groups * ((RS_WINDOW_MIN + groups - 1) // groups)
    anchored = max(0, tiles - 1 - window)                  # tiles window + 1 .. tiles - 1
    chained = max(0, tiles - 1 - (2 * window + 1))         # their anchor t - window - 1 > window
    return tiles, window, anchored, chained
