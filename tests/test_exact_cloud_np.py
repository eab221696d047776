"""The claims of tests/exact_cloud_np.py, on the CPU: every fp32 operation of the per-point chain equals its fp64 value on
these clouds, e 2^20 is an integer, the sector margin holds, enough base points stay, the count tables are the quoted
ones, and the fp64 twins (surface_np.points, wall_np.points) reproduce the builder's cells without calling a point
ambiguous (but for |e| == gate exactly, which the twins flag by their own 1e-5 rule and still bin the same way)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cloud_np as ec  # noqa: E402
import surface_np as sn  # noqa: E402
import wall_np as wn  # noqa: E402

GATES = (0.25, 1.0, 8.0)
GRIDS = (1, 3, 4, 64, 90, 360, 4096)
# signed permutation frames: the models of the surface test and the frame-local frames of the wall test's poses
FRAMES = [ec.frame((0, 0, 0), (1, 0, 0), (0, 0, 1), (0, -1, 0)),
          ec.frame((0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0)),
          ec.frame((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)),
          ec.frame((-0.125, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)),
          ec.frame((0, 0.375, -1.5), (0, -1, 0), (0, 0, 1), (-1, 0, 0))]


def test_count_tables():
    assert len(ec.triples()) == 161 and ec.triples()[0] == (3, 4, 5)
    want = {0.25: (928, 72), 1.0: (3792, 298), 8.0: (18824, 1432)}
    for gate in GATES:
        y, z, e = ec.all_points(gate)
        assert (len(e), len(np.unique(e))) == want[gate]
        q = e * 2.0 ** 20
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 2.0 ** 23
    assert np.abs(ec.all_points(8.0)[2]).max() == 8.0                  # e == gate == 8 is reached exactly: e 2^20 = 2^23
    assert not np.any(np.abs(ec.all_points(1.0)[2]) == 1.0) and not np.any(np.abs(ec.all_points(0.25)[2]) == 0.25)


@pytest.mark.parametrize("gate", GATES)
def test_share_kept_and_sector_margin(gate):
    for ns in GRIDS:
        b = ec.base_points(gate, ns)
        assert b["share"] >= (0.80 if ns == 64 else 0.90), (ns, b["share"])
        ys = ec.sector_coordinate(b["y"], b["z"], ns)
        assert np.all(np.abs(ys - np.rint(ys)) >= ec.MARGIN)
        assert np.array_equal(b["sector"], np.minimum(np.floor(ys), ns - 1)) and b["sector"].max() < ns
        if ns in (64, 90):
            assert len(np.unique(b["sector"])) == (64 if ns == 64 else 88)
    assert ec.base_points(gate, 64)["share"] < 0.84


def _chain32(x, f, R):
    """The per-point chain in numpy fp32, one rounding per operation (the device fuses some of them; where every
    intermediate is exact the fused and the unfused value are the same)."""
    f32 = np.float32
    o, a = f["o"].astype(f32), f["a"].astype(f32)
    q = x - o
    t = (q[:, 0] * a[0] + q[:, 1] * a[1]) + q[:, 2] * a[2]
    w = q - t[:, None] * a
    sq = w * w
    rho = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    return q, t, w, sq, rho, rho - f32(R)


def _chain64(x, f, R):
    x = x.astype(np.float64)
    q = x - f["o"]
    t = q @ f["a"]
    w = q - t[:, None] * f["a"]
    sq = w * w
    rho = np.sqrt(sq.sum(1))
    return q, t, w, sq, rho, rho - R


@pytest.mark.parametrize("gate,R", [(0.25, 2.0), (1.0, 2.0), (8.0, 2.0), (8.0, 9.25)])   # R = 9.25: e == -8 at rho = 1.25
def test_every_fp32_operation_is_exact(gate, R):
    b = ec.base_points(gate, 90, R)
    assert R == 2.0 or np.any(b["e"] == np.float32(-8.0))
    s = ec.fill(b, 2 * len(b["e"]), 40, t0=-5.0, seed=1)
    for f in FRAMES:
        x = ec.xyz(s, f)
        for v32, v64 in zip(_chain32(x, f, R), _chain64(x, f, R)):
            assert v32.dtype == np.float32 and np.array_equal(v32.astype(np.float64), v64)
        e32 = _chain32(x, f, R)[5]
        assert np.array_equal(e32, s["e"])
        q = e32 * np.float32(2.0 ** 20)
        assert np.array_equal(q, np.rint(q)) and np.array_equal(q.astype(np.float64), s["e"].astype(np.float64) * 2.0 ** 20)
        # the plane coordinates the sector is decided from
        w = _chain64(x, f, R)[2]
        assert np.array_equal(w @ f["u"], s["y"]) and np.array_equal(w @ f["v"], s["z"])
    j = ec.stations(s, 0.25, t0=-5.0)
    assert j.min() == 0 and j.max() == 39


@pytest.mark.parametrize("gate,ns,nst", [(0.25, 90, 40), (1.0, 64, 64), (8.0, 4096, 1), (0.25, 1, 4096), (0.25, 1, 1)])
def test_surface_twin_reproduces_the_builder(gate, ns, nst):
    b = ec.base_points(gate, ns)
    p = sn.params(n_stations=nst, n_sectors=ns, gate=gate)
    s = ec.fill(b, 3000, nst, t0=-5.0, seed=2, fracs=(1, 2, 3))
    exp = ec.expected(s, gate, 0.25, nst, ns, t0=-5.0)
    for model in ([0, 0, 0, 1, 0, 0, 2], [0, 0, 0, 0, -1, 0, 2], [0, 0, 0, 0, 0, 1, 2]):
        f = sn.map_frame(model)
        r = sn.points(ec.xyz(s, f), None, f["o"], f["a"], f["u"], f["v"], f["R"], p)
        assert np.array_equal(r["ambiguous"], np.abs(s["e"]) == np.float32(gate)) and r["ambiguous"].mean() < 0.01
        assert np.array_equal(r["e"], s["e"].astype(np.float64)) and np.array_equal(r["cell"], exp["cell"])
        assert np.array_equal(r["cls"], exp["cls"]) and exp["counts"][0] == 3000
    c = sn.cells_from(exp["e"], exp["cell"], nst * ns)
    assert int(c[0].sum()) == 3000


@pytest.mark.parametrize("pose", [wn.pose_matrix((0, 0, 0)), wn.pose_matrix((12.625, 0, 0)),
                                  np.array([[1, 0, 0, 12.5], [0, 0, -1, 0], [0, 1, 0, 0]], float),
                                  np.array([[0, -1, 0, 3.0], [1, 0, 0, 0], [0, 0, 1, 0]], float)])
def test_wall_twin_reproduces_the_builder(pose):
    p = wn.params(n_stations=128)
    f = wn.add_frame(wn.design_frame(p), p, pose)
    b = ec.base_points(0.25, 90)
    s = ec.fill(b, 3000, 40, t0=-5.0, seed=3, fracs=(1, 2, 3))
    exp = ec.expected(s, 0.25, 0.25, 128, 90, j0=f["anchor"])
    r = wn.points(ec.xyz(s, f), None, f, p)
    assert not r["ambiguous"].any()
    assert np.array_equal(r["e"], s["e"].astype(np.float64)) and np.array_equal(r["cell"], exp["cell"])
    assert np.array_equal(r["cls"], exp["cls"])
    assert exp["counts"][1] == int((ec.stations(s, 0.25, j0=f["anchor"]) < 0).sum())


def test_expected_classes_and_patterns():
    b = ec.base_points(0.25, 90)
    fl = ec.fillers(b, 0.25, 40, 90, t0=-5.0)
    for kind, cls in (("plane", ec.PLANE), ("beyond", ec.BEYOND), ("outside", ec.OUTSIDE), ("nan", ec.BEYOND)):
        exp = ec.expected(fl[kind], 0.25, 0.25, 40, 90, t0=-5.0)
        assert exp["cls"][0] == cls and exp["cell"][0] == -1
        assert np.isnan(exp["e"][0]) == (kind in ("plane", "nan"))
    pats = ec.patterns(b, fl, 40, 90, t0=-5.0)
    f = FRAMES[0]
    cells = lambda s: ec.expected(s, 0.25, 0.25, 40, 90, t0=-5.0)["cell"]  # noqa: E731
    c = cells(pats["one_cell_per_wave"]).reshape(-1, 64)
    assert np.all(c == c[:, :1]) and np.all(c >= 0)
    c = cells(pats["across_waves"])
    assert c[63] == c[64] and c[127] == c[128] and c[191] == c[192] and c[62] == c[63] and c[39] != c[40]
    c = cells(pats["alternating"])
    assert np.all(c[:-1] != c[1:]) and np.all(c[:-2] == c[2:])
    for kind in fl:
        c = cells(pats["gap_" + kind])
        gaps = np.flatnonzero(c < 0)
        assert len(gaps) >= 6 and np.all(c[c >= 0] == c[0]) and c[0] >= 0 and c[-1] >= 0
    s = pats["cancelling"]
    exp = ec.expected(s, 0.25, 0.25, 40, 90, t0=-5.0)
    count, mean, _, _ = sn.cells_from(exp["e"], exp["cell"], 3600)
    assert np.any((count > 0) & (mean == 0.0))
    for s in pats.values():
        ec.xyz(s, f)
    # the extremes of a run at every pair of places
    for where in ec.WHERE:
        i = ec.run_indices(b, int(b["sector"][0]), 9, where)
        e = b["e"][i]
        pos = dict(head=0, middle=4, tail=8)
        assert e[pos[where[0]]] == e.min() and e[pos[where[1]]] == e.max()
