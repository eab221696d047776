"""The numpy references of tests/binning_np.py against the C restatement (oracle/gm_oracle.c), on the CPU: what
tests/test_gpu_binning.py holds the sort, the voxel grid and the 1-NN against is itself checked in every CPU run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binning_np as bn  # noqa: E402
from geometric_mapping_amd import synth  # noqa: E402

LEAF = 0.25
PLAN_TABLE = bn.LATTICE_PLANS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_twin_is_oracle(oc, xyz, leaf):
    cen, cnt, key, pt = bn.voxel_twin(xyz, leaf)
    o_cen, o_key, o_cnt, o_pt = oc.voxel_grid(xyz, leaf, oc.F64)
    assert pt == o_pt
    assert len(cen) == len(o_cen)
    assert np.array_equal(cnt, o_cnt)
    assert np.array_equal(key, o_key.view(np.uint32))
    # both add a voxel's points in ascending (key, index) order in fp64 and divide once: the same bits on any cloud
    assert np.array_equal(bits(cen), bits(o_cen))
    return cen, cnt, key, pt


@pytest.mark.parametrize("S", sorted(PLAN_TABLE))
def test_expected_plan_and_twin_on_lattice_blocks(oc, S):
    rng = np.random.default_rng(100 + S)
    xyz = bn.lattice_cloud(20000, S, LEAF, rng)
    b, passes, digit, passthrough = PLAN_TABLE[S]
    assert bn.expected_plan(xyz, LEAF) == (b, passes, digit)
    _, _, guard = bn.voxel_keys(xyz, LEAF)
    assert guard == (S, S, S)                                   # the pinned corners make the extent exact
    cen, cnt, key, pt = assert_twin_is_oracle(oc, xyz, LEAF)
    assert pt == passthrough
    assert cnt.sum() == len(xyz)
    if passthrough:
        assert np.array_equal(bits(cen), bits(xyz)) and np.array_equal(key, np.arange(len(xyz)))
    else:
        assert (np.diff(key.astype(np.int64)) > 0).all()
        cell = np.floor(cen.astype(np.float64) / LEAF).astype(np.int64)     # a centroid lies in its own cell
        k2 = cell[:, 0] + cell[:, 1] * S + cell[:, 2] * S * S
        assert np.array_equal(k2, key.astype(np.int64))


def test_lattice_sums_do_not_depend_on_order(oc):
    """What makes bit-equality a derived bound: the fp64 sums of a lattice cloud are exact, so any summation order gives
    the twin's centroids."""
    rng = np.random.default_rng(5)
    xyz = bn.lattice_cloud(50000, 6, LEAF, rng)
    cen, cnt, key, _ = bn.voxel_twin(xyz, LEAF)
    perm = rng.permutation(len(xyz))
    cen2, cnt2, key2, _ = bn.voxel_twin(xyz[perm], LEAF)
    assert np.array_equal(key, key2) and np.array_equal(cnt, cnt2) and np.array_equal(bits(cen), bits(cen2))
    assert_twin_is_oracle(oc, xyz[perm], LEAF)


@pytest.mark.parametrize("S,n", [((4096, 1, 1), 20000), ((2, 1, 1), 7001), (1, 7000), (40, 1), (40, 2), (79, 4097)])
def test_twin_on_lattice_shapes(oc, S, n):
    rng = np.random.default_rng(7)
    xyz = bn.lattice_cloud(n, S, LEAF, rng)
    _, cnt, _, pt = assert_twin_is_oracle(oc, xyz, LEAF)
    assert not pt and cnt.sum() == n
    if S == (4096, 1, 1):
        assert bn.expected_plan(xyz, LEAF) == (32, 4, 8)        # a 32-bit plan without passthrough


@pytest.mark.parametrize("leaf", [0.5, 0.1, 0.27, 0.158, 0.15625, 0.02])
def test_twin_on_ordinary_clouds(oc, leaf):
    xyz = synth.tunnel_frame(30000, seed=3, floor_z=-1.2, outlier_frac=0.01)
    _, cnt, _, pt = assert_twin_is_oracle(oc, xyz, leaf)
    assert not pt and cnt.sum() == len(xyz)


def test_twin_passthrough_on_an_ordinary_cloud(oc):
    xyz = synth.tunnel_frame(5000, seed=4)
    cen, cnt, key, pt = assert_twin_is_oracle(oc, xyz, 0.001)   # 12000 x 4000 x 4000 cells
    assert pt and np.array_equal(bits(cen), bits(xyz)) and (cnt == 1).all()
    e = bn.voxel_twin(xyz[:0], 0.5)
    assert len(e[0]) == 0 and len(e[1]) == 0 and not e[3]


def test_nearest_brute_without_ties(oc):
    xyz = synth.cylinder_frame(9000, seed=11)
    q = oc.voxel_grid(xyz, 0.5)[0]
    a = bn.nearest_brute(xyz, q)
    assert np.array_equal(a, oc.nearest(xyz, q))
    assert bn.tied_share(xyz, q, a) < 0.01                      # (fp32 distances of a continuous cloud: a tie is an accident)
    assert np.array_equal(bn.nearest_brute(xyz[:0], q), np.full(len(q), -1))
    assert np.array_equal(oc.nearest(xyz[:0], q), np.full(len(q), -1))


@pytest.mark.parametrize("n,nq", [(255, 255), (4097, 257), (9000, 600)])
def test_nearest_brute_with_ties(oc, n, nq):
    rng = np.random.default_rng(n + nq)
    xyz, q = bn.tie_cloud(n, nq, rng)
    a = bn.nearest_brute(xyz, q)
    assert np.array_equal(a, oc.nearest(xyz, q))
    assert bn.tied_share(xyz, q, a) > 0.5
    # the reference is the lowest index among the rows at the smallest distance
    for i in range(0, nq, 7):
        d = (q[i] - xyz).astype(np.float64)
        d2 = (d * d).sum(axis=1)                                # small integers and halves: exact
        assert a[i] == np.flatnonzero(d2 == d2.min())[0]


def test_eight_way_ties_over_two_chunks(oc):
    xyz, q, corners = bn.eight_tie_cloud(600, np.random.default_rng(8))
    assert len(xyz) == 8192
    a = bn.nearest_brute(xyz, q)
    assert np.array_equal(a, oc.nearest(xyz, q))
    assert np.array_equal(a, corners.min(axis=1))
    assert ((corners < 4096).sum(axis=1) == 4).all()            # four tied rows in either 4096-point chunk


@pytest.mark.parametrize("n,threads,digit,expect", [
    (1100000, 1024, 8, (135, 128, 6, 0)), (2200000, 1024, 8, (269, 128, 140, 11)), (1100000, 1024, 9, (135, 112, 22, 0)),
    (500000, 512, 8, (123, 112, 10, 0)), (1000000, 512, 8, (245, 112, 132, 19)), (500000, 512, 9, (123, 112, 10, 0)),
    (833000, 1024, 9, (102, 112, 0, 0)), (20000, 1024, 8, (3, 128, 0, 0))])
def test_sort_shape(n, threads, digit, expect):
    assert bn.sort_shape(n, threads, digit) == expect
