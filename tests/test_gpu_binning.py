"""The binning chain -- csrc/k_sort.hip (one-launch-per-pass radix sort with a decoupled look-back), gm_compact.hpp
(chained-scan compaction), k_voxel.hip (both voxel paths) and k_nearest.hip -- against the plain references of
tests/binning_np.py, at the pass, tile and window edges.

sort     through gm_voxel_grid (ctx.voxelGrid): the keys are the test's, the path always sorts.  Clouds are lattice
         clouds (binning_np.lattice_cloud): their fp64 sums are exact in any order, so flag, voxel count, counts and
         centroid BITS must equal the twin's.  A key out of order splits a run (voxel count), a value paired with the
         wrong key moves a centroid out of its cell.  Every case runs on a context with n_slots = 1 (1024-thread pass)
         and on one with n_slots = 2 (512-thread pass; the stage call uses slot 0).  What is NOT observable here is the
         sort's stability: the fp64 sums hide the order inside a voxel ("what is pinned where").
frames   points ON voxel faces and the dense <-> sort switch (dim 64 / 65), through whole frames, blocking and replayed
         from a graph.  The reference is the twin applied to the product's own valid cloud.
nearest  exact ties across the 256-point LDS windows and the 4096-point chunks of k_nn_scan, against nearest_brute.

The last test writes what the cases saw to build/binning_observed.json (git-ignored) and asserts that every mechanism the
cases are there for was reached.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binning_np as bn  # noqa: E402
from geometric_mapping_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.25
SHAPES = {"t1024": dict(n_slots=1, threads=1024), "t512": dict(n_slots=2, threads=512)}
OBSERVED = {"sort": {}, "reuse": {}, "frames": {}, "nearest": {}}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the sort's cases

def _lattice(n, S, seed, **kw):
    return lambda: bn.lattice_cloud(n, S, LEAF, np.random.default_rng(seed), **kw)


def _one_voxel_but_the_corners(n, S, seed):
    def make():
        cells = np.full((n, 3), S // 2)
        return bn.lattice_cloud(n, S, LEAF, np.random.default_rng(seed), cells=cells)
    return make


def _alternating(n):
    def make():
        cells = np.zeros((n, 3), np.int64)
        cells[1::2, 0] = 1
        return bn.lattice_cloud(n, (2, 1, 1), LEAF, np.random.default_rng(31), cells=cells)
    return make


def _by_key(descending):
    def make():
        xyz = bn.lattice_cloud(20000, 40, LEAF, np.random.default_rng(32))
        order = np.argsort(bn.voxel_keys(xyz, LEAF)[0], kind="stable")
        return np.ascontiguousarray(xyz[order[::-1] if descending else order])
    return make


def _own_voxel(n, S):
    def make():
        rng = np.random.default_rng(33)
        site = np.concatenate(([0, S ** 3 - 1], 1 + rng.permutation(S ** 3 - 2)[:n - 2]))
        cells = np.stack([site % S, (site // S) % S, site // (S * S)], axis=1)
        return bn.lattice_cloud(n, S, LEAF, rng, cells=cells)
    return make


TILE_EDGE_N = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 16385)
# name -> (maker, (key bits, passes, digit bits) the case is there for or None, passthrough, shapes it runs on)
CASES = {}
for _S, (_b, _p, _d, _pt) in bn.LATTICE_PLANS.items():
    CASES[f"plan_S{_S}"] = (_lattice(20000, _S, 100 + _S), (_b, _p, _d), _pt, tuple(SHAPES))
for _S, _plan in ((40, (17, 2, 9)), (79, (19, 3, 8))):
    for _n in TILE_EDGE_N:
        CASES[f"edge_S{_S}_n{_n}"] = (_lattice(_n, _S, 1000 * _S + _n), _plan if _n > 1 else (3, 1, 8), False, tuple(SHAPES))
CASES["skew_one_voxel"] = (_lattice(70000, 1, 30), (3, 1, 8), False, tuple(SHAPES))          # every tile: one digit, full count
CASES["skew_two_voxels"] = (_alternating(70001), (5, 1, 8), False, tuple(SHAPES))
CASES["skew_ascending"] = (_by_key(False), (17, 2, 9), False, tuple(SHAPES))
CASES["skew_descending"] = (_by_key(True), (17, 2, 9), False, tuple(SHAPES))
CASES["skew_own_voxel"] = (_own_voxel(3 * 4096 + 1, 24), (14, 2, 8), False, tuple(SHAPES))    # every position a segment head
CASES["skew_line_4096"] = (_lattice(20000, (4096, 1, 1), 34), (32, 4, 8), False, tuple(SHAPES))   # top passes: one digit
CASES["reuse_n5"] = (_lattice(5, 40, 35), (17, 2, 9), False, tuple(SHAPES))
# beyond the look-back window (binning_np.sort_shape): the 32-bit inclusive rows, and an anchor that is itself anchored
for _shape, _sizes in (("t1024", ((1100000, 80), (2200000, 80), (1100000, 6))),
                       ("t512", ((500000, 80), (1000000, 80), (500000, 6), (1000000, 6)))):
    for _n, _S in _sizes:
        CASES[f"window_{_shape}_n{_n}_S{_S}"] = (_lattice(_n, _S, _n // 1000 + _S), (20, 3, 8) if _S == 80 else (9, 1, 9), False, (_shape,))
# (not asked for by the case list, cheap: all rows but the corners in ONE voxel beyond the window -- the packed 16-bit
# partial sums of the look-back at their largest, 7 x 8192 and 14 x 4096)
CASES["window_t1024_skew"] = (_one_voxel_but_the_corners(1100000, 6, 36), (9, 1, 9), False, ("t1024",))
CASES["window_t512_skew"] = (_one_voxel_but_the_corners(500000, 6, 37), (9, 1, 9), False, ("t512",))
LONGEST = {"t1024": "window_t1024_n2200000_S80", "t512": "window_t512_n1000000_S80"}
SORT_PARAMS = [(shape, name) for name, c in CASES.items() for shape in c[3]]


@functools.lru_cache(maxsize=None)
def case(name):
    """(cloud, twin) of a case, made once; asserts that the cloud reaches the plan the case is there for."""
    make, plan, passthrough, _ = CASES[name]
    xyz = make()
    xyz.setflags(write=False)
    if plan is not None:
        assert bn.expected_plan(xyz, LEAF) == plan, name
    twin = bn.voxel_twin(xyz, LEAF)
    assert twin[3] == passthrough, name
    return xyz, twin


@pytest.fixture(scope="module")
def contexts(gm):
    assert "GM_SORT_THREADS" not in os.environ      # (the experiments' override of the block shape)
    ctx = {shape: gm.GeometricMapping(n_slots=kw["n_slots"]) for shape, kw in SHAPES.items()}
    yield ctx
    for c in ctx.values():
        c.close()


def check_voxel_grid(ctx, name):
    xyz, (cen, cnt, key, passthrough) = case(name)
    g_cen, g_cnt, g_pass = ctx.voxelGrid(LEAF, xyz)
    assert g_pass == passthrough, name
    assert len(g_cen) == len(cen), (name, len(g_cen), len(cen))
    assert np.array_equal(g_cnt, cnt), name
    diff = np.flatnonzero((bits(g_cen) != bits(cen)).any(axis=1))
    assert len(diff) == 0, (name, len(diff), diff[:5], g_cen[diff[:5]], cen[diff[:5]])
    if passthrough:
        assert np.array_equal(bits(g_cen), bits(xyz)) and (g_cnt == 1).all()      # the input rows, bit for bit, in order
    return g_cen, g_cnt


@pytest.mark.parametrize("shape,name", SORT_PARAMS)
def test_sort_through_voxel_grid(contexts, shape, name):
    xyz, twin = case(name)
    bits_, passes, digit = bn.expected_plan(xyz, LEAF)
    tiles, window, anchored, chained = bn.sort_shape(len(xyz), SHAPES[shape]["threads"], digit)
    check_voxel_grid(contexts[shape], name)
    OBSERVED["sort"][f"{shape}/{name}"] = dict(n=len(xyz), key_bits=bits_, passes=passes, digit_bits=digit, tiles=tiles,
                                               window=window, inclusive_row_tiles=anchored, anchored_anchors=chained,
                                               passthrough=bool(twin[3]), voxels=len(twin[0]))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sort_state_does_not_leak_between_calls(gm, shape):
    """A long sort, a short one, one of two tiles and the long one again on ONE context: the records and digit totals of
    a call (cleared per call, csrc/k_sort.hip) must not reach the next.  Every result equals the twin and, bit for bit,
    that of a context that has run nothing else."""
    names = [LONGEST[shape], "reuse_n5", "edge_S40_n8193", LONGEST[shape]]
    fresh = {}
    for name in set(names):
        with gm.GeometricMapping(n_slots=SHAPES[shape]["n_slots"]) as c:
            fresh[name] = check_voxel_grid(c, name)
    with gm.GeometricMapping(n_slots=SHAPES[shape]["n_slots"]) as c:
        for k, name in enumerate(names):
            g_cen, g_cnt = check_voxel_grid(c, name)
            assert np.array_equal(bits(g_cen), bits(fresh[name][0])) and np.array_equal(g_cnt, fresh[name][1]), (k, name)
    OBSERVED["reuse"][shape] = names


# ---------------------------------------------------------------- voxel faces and the dense <-> sort switch, in frames

BOUND, RADIUS = 5.0, 0.3
FRAME_LEAVES = {0.5: ("dense", 21), 0.1: ("sort", 101), 0.158: ("dense", 64), 0.15625: ("sort", 65)}
DENSE_MAX_CELLS = 1 << 18


def lattice_dim(leaf):
    """Cells per axis of the voxel lattice over the crop box, as the product's table is laid out."""
    inv = np.float32(1.0) / np.float32(leaf)
    return int(np.floor(np.float32(BOUND) * inv) - np.floor(np.float32(-BOUND) * inv)) + 1


@functools.lru_cache(maxsize=None)
def face_cloud(leaf):
    """A 20 k tunnel with the x of a random 30 % of the points and the y of another 30 % snapped to the nearest fp32
    multiple of float32(leaf) (the product k * float32(leaf) rounded to fp32), a few points exactly on x = +-5.0, z left
    continuous (no neighbourhood degenerates)."""
    xyz = synth.tunnel_frame(20000, seed=21).copy()
    rng = np.random.default_rng(77)
    lf = np.float32(leaf)
    pick = rng.permutation(len(xyz))
    m = (3 * len(xyz)) // 10
    for rows, axis in ((pick[:m], 0), (pick[m:2 * m], 1)):
        k = np.rint(xyz[rows, axis] / lf).astype(np.float32)
        snapped = k * lf
        assert snapped.dtype == np.float32
        xyz[rows, axis] = snapped
    xyz[np.flatnonzero((xyz[:, 0] > 4.8) & (xyz[:, 0] < 5.0))[:4], 0] = 5.0
    xyz[np.flatnonzero((xyz[:, 0] < -4.8) & (xyz[:, 0] > -5.0))[:4], 0] = -5.0
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def binary_cloud():
    """The tunnel with every coordinate rounded to a multiple of 2^-10: exact sums in fp64 (and in the dense table's
    fixed point, whose scale is a power of two >= 2^10) in any order."""
    xyz = (np.rint(synth.tunnel_frame(20000, seed=22).astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
    xyz.setflags(write=False)
    return xyz


def on_face_share(cloud, leaf):
    v = cloud * (np.float32(1.0) / np.float32(leaf))        # fp32, as both paths compute the lattice coordinate
    assert v.dtype == np.float32
    return float((v == np.floor(v)).any(axis=1).mean())


def run_frame(gm, xyz, leaf, graph):
    from geometric_mapping_amd import _lib
    flags = _lib.GM_CFG_DEFAULT | (_lib.GM_CFG_GRAPH if graph else 0)
    with gm.GeometricMapping(boxFilterBound=BOUND, voxelGridLeafSize=leaf, neighborRadius=RADIUS, flags=flags) as c:
        res = c.process_frame(xyz)
        if graph:       # the second frame of a context is the replayed one
            res = c.process_frame(xyz)
        cloud, _ = c.cropped_cloud()
        cen, vcnt = c.voxel_centroids()
    assert not (res["status_flags"] & _lib.GM_RES_VOXEL_PASSTHROUGH)
    return res, cloud, cen, vcnt


@pytest.mark.parametrize("graph", [False, True], ids=["blocking", "graph"])
@pytest.mark.parametrize("leaf", list(FRAME_LEAVES))
def test_points_on_voxel_faces(gm, leaf, graph):
    path, dim = FRAME_LEAVES[leaf]
    assert lattice_dim(leaf) == dim and (dim ** 3 <= DENSE_MAX_CELLS) == (path == "dense")
    res, cloud, cen, vcnt = run_frame(gm, face_cloud(leaf), leaf, graph)
    n_valid = res["n_valid"]
    assert n_valid == len(cloud) > 15000
    share = on_face_share(cloud, leaf)
    assert share >= 0.2                                                 # a condition on the input
    assert np.abs(cloud[:, 0]).max() == 5.0                             # points on the box's own faces are in
    t_cen, t_cnt, _, t_pass = bn.voxel_twin(cloud, leaf)                # the product's OWN valid cloud
    assert not t_pass
    assert res["n_voxels"] == len(cen) == len(t_cen)
    assert np.array_equal(vcnt, t_cnt)                                  # membership, order included
    assert vcnt.sum() == n_valid
    err = float(np.abs(cen.astype(np.float64) - t_cen).max())
    assert err < 2e-6 * max(1.0, BOUND)
    OBSERVED["frames"][f"faces/{leaf}/{'graph' if graph else 'blocking'}"] = dict(
        path=path, dim=dim, n_valid=int(n_valid), voxels=len(cen), on_face_share=share, max_centroid_error=err)


@pytest.mark.parametrize("leaf", list(FRAME_LEAVES))
def test_exact_sums_in_frames(gm, leaf):
    """Coordinates that are multiples of 2^-10: the sort path's fp64 sums are exact (centroid bits equal the twin's), and
    so are the dense table's fixed-point sums -- there three fp64 roundings (1 / count, the product, + lo) and one cast
    remain where the twin has one division and one cast: within 1 fp32 ulp."""
    path, dim = FRAME_LEAVES[leaf]
    res, cloud, cen, vcnt = run_frame(gm, binary_cloud(), leaf, False)
    assert res["n_valid"] == len(cloud) > 15000
    assert np.array_equal(cloud.astype(np.float64) * 1024.0, np.rint(cloud.astype(np.float64) * 1024.0))
    t_cen, t_cnt, _, _ = bn.voxel_twin(cloud, leaf)
    assert len(cen) == len(t_cen) and np.array_equal(vcnt, t_cnt) and vcnt.sum() == res["n_valid"]
    if path == "sort":
        assert np.array_equal(bits(cen), bits(t_cen))
    else:
        ulp = np.spacing(np.maximum(np.abs(cen), np.abs(t_cen)))
        assert (np.abs(cen - t_cen) <= ulp).all()
        assert np.abs(cen.astype(np.float64) - t_cen).max() < 2e-6 * max(1.0, BOUND)
    OBSERVED["frames"][f"exact/{leaf}"] = dict(path=path, dim=dim, n_valid=int(res["n_valid"]), voxels=len(cen),
                                               bit_equal_share=float((bits(cen) == bits(t_cen)).all(axis=1).mean()))


# ---------------------------------------------------------------- 1-NN ties

NN_PAIRS = [(1, 1), (1, 600), (255, 255), (255, 600), (256, 257), (257, 256), (4095, 255), (4096, 600), (4097, 1),
            (4097, 257), (9000, 1), (9000, 256), (9000, 600)]


@pytest.mark.parametrize("n,nq", NN_PAIRS)
def test_nearest_ties(contexts, n, nq):
    xyz, q = bn.tie_cloud(n, nq, np.random.default_rng(7 * n + nq))
    want = bn.nearest_brute(xyz, q)
    got = contexts["t1024"].nearest(xyz, q)
    share = bn.tied_share(xyz, q, want)
    assert n == 1 or share > 0.5                        # a condition on the input (one point cannot tie)
    assert np.array_equal(got, want), (n, nq, np.flatnonzero(got != want)[:8])
    OBSERVED["nearest"][f"n{n}_nq{nq}"] = dict(tied_share=share, windows=(n + 255) // 256, chunks=(n + 4095) // 4096)


def test_nearest_eight_way_ties_over_two_chunks(contexts):
    xyz, q, rows = bn.eight_tie_cloud(600, np.random.default_rng(8))
    want = bn.nearest_brute(xyz, q)
    assert np.array_equal(want, rows.min(axis=1)) and ((rows < 4096).sum(axis=1) == 4).all()
    got = contexts["t1024"].nearest(xyz, q)
    assert np.array_equal(got, want)
    OBSERVED["nearest"]["eight_way"] = dict(tied_share=bn.tied_share(xyz, q, want), windows=32, chunks=2, ways=8)


def test_nearest_without_a_choice(contexts, oc):
    """One point answers every query; no point answers none (-1, as the C restatement)."""
    xyz, q = bn.tie_cloud(300, 257, np.random.default_rng(9))
    assert contexts["t1024"].nearest(xyz[:1], q).tolist() == [0] * len(q)
    none = contexts["t1024"].nearest(xyz[:0], q)
    assert np.array_equal(none, oc.nearest(xyz[:0], q)) and np.array_equal(none, bn.nearest_brute(xyz[:0], q))
    assert (none == -1).all()


# ---------------------------------------------------------------- what the cases saw

def test_zz_write_what_the_cases_observed():
    """On record (runs last: the file's order), and every mechanism the cases are there for was reached."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", "binning_observed.json"), "w") as f:
        json.dump(OBSERVED, f, indent=1, sort_keys=True)
    for shape in SHAPES:
        seen = [o for k, o in OBSERVED["sort"].items() if k.startswith(shape + "/")]
        plans = {(o["passes"], o["digit_bits"]) for o in seen}
        assert plans >= {(1, 8), (1, 9), (2, 8), (2, 9), (3, 8), (3, 9), (4, 8)}, (shape, plans)
        for digit in (8, 9):    # the inclusive rows, with either digit width
            assert any(o["inclusive_row_tiles"] > 0 and o["digit_bits"] == digit for o in seen), (shape, digit)
        assert any(o["anchored_anchors"] > 0 for o in seen), shape                   # an anchor that is itself anchored
        assert any(o["key_bits"] == 31 for o in seen)
        assert any(o["key_bits"] == 32 and not o["passthrough"] for o in seen)
        assert any(o["passthrough"] and o["tiles"] > 1 for o in seen)
        assert any(o["voxels"] == 1 and o["tiles"] > 1 for o in seen)                # one digit, every tile
        assert any(o["voxels"] == o["n"] > 8192 and not o["passthrough"] for o in seen)   # every position a head
        assert OBSERVED["reuse"].get(shape)
    frames = OBSERVED["frames"]
    for mode in ("blocking", "graph"):
        for leaf, (path, dim) in FRAME_LEAVES.items():
            o = frames[f"faces/{leaf}/{mode}"]
            assert o["path"] == path and o["dim"] == dim and o["on_face_share"] >= 0.2
    assert {frames[f"faces/{leaf}/blocking"]["dim"] for leaf in FRAME_LEAVES} >= {64, 65}     # either side of the switch
    assert all(f"exact/{leaf}" in frames for leaf in FRAME_LEAVES)
    nn = OBSERVED["nearest"]
    assert any(o["windows"] > 1 and o["chunks"] == 1 and o["tied_share"] > 0.5 for o in nn.values())
    assert any(o["chunks"] > 2 and o["tied_share"] > 0.5 for o in nn.values())
    assert nn["eight_way"]["tied_share"] == 1.0
