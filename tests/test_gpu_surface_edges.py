"""GPU tests of k_surface_map (csrc/k_surface.hip) on small clouds whose fp32 per-point chain is exact
(tests/exact_cloud_np.py): the per-point residual and cell, every cell record and the class counts are compared bit for
bit with values computed from the builder alone -- never from what the device reported -- at the wave, trip, unroll and
block edges of the kernel, on per-wave cell patterns the run merge has to get right, and at the stated edges of the rule
(include/gm_hip.h): the closed-left station edge, |e| == gate, the clamp to the last sector, rows that are not finite,
a point on the axis."""
import functools
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cloud_np as ec  # noqa: E402
import surface_np as sn  # noqa: E402

pytestmark = pytest.mark.gpu
X_MODEL = [0, 0, 0, 1, 0, 0, 2]
T_MIN, DS = -5.0, 0.25
# n_stations, n_sectors, gate (a finer grid takes a wider gate: enough base points per sector for the runs)
GRIDS = {"40x90": (40, 90, 0.25), "1x1": (1, 1, 0.25), "64x64": (64, 64, 1.0), "1x4096": (1, 4096, 8.0),
         "4096x1": (4096, 1, 0.25)}
# one wave, one block trip (1024), the 2-point unroll (2048), the 1 -> 2 -> 3 block steps of surface_blocks (16384 each)
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 32769)


@functools.lru_cache(maxsize=None)
def _base(gate, n_sectors, R=2.0):
    return ec.base_points(gate, n_sectors, R)


@pytest.fixture(scope="module")
def ctx(gm):
    with gm.GeometricMapping() as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _check(out, s, nst, nsec, gate, model=X_MODEL, status=_lib.GM_SURF_OK, t0=T_MIN, ds=DS):
    """One stage call's outputs against the builder: per point, per cell, the info block."""
    info, count, mean, mn, mx, res, cell = out
    exp = ec.expected(s, gate, ds, nst, nsec, t0=t0)
    assert info["status"] == status and (info["n_stations"], info["n_sectors"]) == (nst, nsec)
    f = sn.map_frame(model)
    for k in ("o", "a", "u", "v"):
        assert np.array_equal(info[k].astype(np.float64), f[k]), k
    assert float(info["R"]) == f["R"]
    ec.same_points(res, cell, exp)
    c2, m2, lo2, hi2 = sn.cells_from(exp["e"], exp["cell"], nst * nsec)
    assert np.array_equal(count.reshape(-1), c2)
    for a, b in ((mean, m2), (mn, lo2), (mx, hi2)):
        assert np.array_equal(_bits(a), _bits(b))
    got = tuple(info[k] for k in ("mapped", "outside", "beyond_gate", "plane"))
    assert got == exp["counts"] and info["cells_hit"] == int((c2 > 0).sum())
    return exp, (c2, m2, lo2, hi2)


def _call(c, s, nst, nsec, gate, model=X_MODEL, **kw):
    f = sn.map_frame(model)
    return c.surfaceMap(ec.xyz(s, f), model, s["labels"], n_stations=nst, n_sectors=nsec, gate=gate, **kw)


@pytest.mark.parametrize("model,status", [([0, 0, 0, 1, 0, 0, 2], 0), ([0, 0, 0, -1, 0, 0, 2], 0), ([0, 0, 0, 0, 1, 0, 2], 0),
                                          ([0, 0, 0, 0, -1, 0, 2], 0), ([0, 0, 0, 0, 0, 1, 2], _lib.GM_SURF_UP_FALLBACK),
                                          ([0, 0, 0, 0, 0, -1, 2], _lib.GM_SURF_UP_FALLBACK)])
def test_frame_vectors_are_the_signed_unit_vectors(ctx, model, status):
    f = sn.map_frame(model)
    assert f["status"] == status
    for k in ("a", "u", "v"):                                           # signed unit vectors, o the origin
        assert sorted(np.abs(f[k])) == [0, 0, 1]
    assert not f["o"].any() and (f["a"] @ [1, 0, 0] >= 0)
    b = _base(0.25, 90)
    s = ec.sprinkle(ec.fill(b, 1500, 40, t0=T_MIN, seed=4), ec.fillers(b, 0.25, 40, 90, t0=T_MIN))
    _check(_call(ctx, s, 40, 90, 0.25, model), s, 40, 90, 0.25, model, status)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_sizes(ctx, grid):
    nst, nsec, gate = GRIDS[grid]
    b = _base(gate, nsec)
    full = ec.sprinkle(ec.fill(b, max(SIZES), nst, t0=T_MIN, seed=5), ec.fillers(b, gate, nst, nsec, t0=T_MIN))
    for n in SIZES:
        s = ec.take(full, np.arange(n))
        exp, _ = _check(_call(ctx, s, nst, nsec, gate), s, nst, nsec, gate)
        if n >= 1023:
            assert all(exp["counts"])                                    # every class is in the cloud


@pytest.mark.parametrize("grid", ["40x90", "64x64", "1x4096", "1x1"])
def test_run_patterns(ctx, grid):
    nst, nsec, gate = GRIDS[grid]
    b = _base(gate, nsec)
    pats = ec.patterns(b, ec.fillers(b, gate, nst, nsec, t0=T_MIN), nst, nsec, t0=T_MIN)
    assert {"one_cell_per_wave", "across_waves", "alternating", "gap_plane", "gap_beyond", "gap_outside", "gap_nan",
            "head_and_tail_runs", "cancelling"} <= set(pats)
    for name, s in pats.items():
        exp, cells = _check(_call(ctx, s, nst, nsec, gate), s, nst, nsec, gate)
        if name == "cancelling" and nst * nsec > 1:
            assert np.any((cells[0] > 0) & (cells[1] == 0.0)), name     # a sum that cancels to 0 with count > 0
    # all of them in one cloud: the patterns at other lanes, and more than one wave per block
    s = ec.concat(*pats.values())
    _check(_call(ctx, s, nst, nsec, gate), s, nst, nsec, gate)


def test_station_edges(ctx):
    b = _base(0.25, 90)
    n = len(b["e"])
    on_edge = ec.spec(b, np.arange(n), ec.stations_t(np.arange(n) % 40, 0.0, t0=T_MIN))       # t == t_min + j ds
    past = ec.spec(b, np.arange(40), ec.stations_t(40, 0.0, t0=T_MIN))                        # t == t_min + n_stations ds
    below = ec.spec(b, np.arange(40), float(np.nextafter(np.float32(T_MIN), np.float32(-np.inf))))
    far = ec.concat(ec.spec(b, np.arange(8), float(np.float32(1e30))), ec.spec(b, np.arange(8), float(np.float32(-1e30))))
    s = ec.concat(on_edge, past, below, far)
    exp, _ = _check(_call(ctx, s, 40, 90, 0.25), s, 40, 90, 0.25)
    assert np.array_equal(exp["cell"][:n] // 90, np.arange(n) % 40)
    assert np.all(exp["cls"][n:] == ec.OUTSIDE) and exp["counts"] == (n, 96, 0, 0)


def test_gate_is_closed(ctx):
    _, _, e_all = ec.all_points(8.0)
    mags = np.intersect1d(e_all[e_all > 0], -e_all[e_all < 0])
    assert len(mags)                                                     # residual magnitudes the cloud has in both signs
    for g in (float(mags[0]), float(mags[-1])):
        b, far = _base(g, 90), ec.beyond_points(g, 90)
        assert np.any(b["e"] == np.float32(g)) and np.any(b["e"] == np.float32(-g))
        s = ec.concat(ec.spec(b, np.arange(len(b["e"])), ec.stations_t(np.arange(len(b["e"])) % 40, 0.5, t0=T_MIN)),
                      ec.spec(far, np.arange(len(far["e"])), ec.stations_t(np.arange(len(far["e"])) % 40, 0.5, t0=T_MIN)))
        exp, _ = _check(_call(ctx, s, 40, 90, g), s, 40, 90, g)
        at = np.abs(s["e"]) == np.float32(g)
        assert np.all(exp["cls"][at] == ec.MAPPED) and {-1.0, 1.0} <= set(np.sign(s["e"][at]))
        assert np.all(exp["cls"][np.abs(s["e"]) > np.float32(g)] == ec.BEYOND) and exp["counts"][2] == len(far["e"])


@pytest.mark.parametrize("R,sign", [(2.0, 1.0), (9.25, -1.0)])
def test_gate_of_eight_keeps_two_to_the_23(ctx, R, sign):
    """e == +8 (R = 2, rho = 10) and e == -8 (R = 9.25, rho = 1.25): e 2^20 = +-2^23 is in the sum, the mean is +-8."""
    b = _base(8.0, 4, R)
    at = np.flatnonzero(b["e"] == np.float32(sign * 8.0))
    assert len(at) >= 4
    model = [0, 0, 0, 1, 0, 0, R]
    s = ec.concat(ec.spec(b, np.resize(at, 300), ec.stations_t(0, 0.5, t0=T_MIN)), ec.fill(b, 3000, 39, t0=T_MIN + DS, seed=6))
    f = sn.map_frame(model)
    out = ctx.surfaceMap(ec.xyz(s, f), model, None, n_stations=40, n_sectors=4, gate=8.0)
    exp, (count, mean, lo, hi) = _check(out, s, 40, 4, 8.0, model)
    assert exp["counts"][0] == 3300 and count[:4].sum() == 300
    hit = count[:4] > 0
    assert np.all(mean[:4][hit] == np.float32(sign * 8.0)) and np.all(lo[:4][hit] == hi[:4][hit])


def test_axis_point_and_rows_that_are_not_finite(ctx):
    b = _base(8.0, 90)
    s = ec.fill(b, 500, 40, t0=T_MIN, seed=7)
    ec.set_rows(s, [5, 64, 300], {k: v[0] for k, v in ec.axis_point(ec.stations_t(3, 0.25, t0=T_MIN)).items()})
    s["bad"][[7, 63, 128, 129]] = ec.NAN_ROW
    s["bad"][[9, 65, 200]] = ec.POS_INF_ROW
    s["bad"][[10, 66, 201]] = ec.NEG_INF_ROW
    for gate in (2.0, 8.0):                                              # gate >= R: the axis point maps
        out = _call(ctx, s, 40, 90, gate)
        exp, _ = _check(out, s, 40, 90, gate)
        assert np.all(exp["cell"][[5, 64, 300]] == 3 * 90) and np.all(out[5][[5, 64, 300]] == np.float32(-2.0))
        bad = s["bad"] != 0
        assert np.all(exp["cls"][bad] == ec.BEYOND) and not np.isfinite(out[5][bad]).any() and np.all(out[6][bad] == -1)
    out = _call(ctx, s, 40, 90, 1.0)                                     # gate < R: beyond the gate
    exp, _ = _check(out, s, 40, 90, 1.0)
    assert np.all(exp["cls"][[5, 64, 300]] == ec.BEYOND)


@pytest.mark.parametrize("nsec", [1, 3, 64, 90, 360, 4096])
def test_fold_and_clamp_to_the_last_sector(ctx, nsec):
    """w.u > 0 and w.v a tiny negative number: theta is a tiny negative angle, phi = theta + 2 pi rounds to 2 pi and
    phi / dtheta to n_sectors or just below: the clamp keeps the point in the last sector.  Not an exact cloud: e against
    the twin at its own 5e-6."""
    f = sn.map_frame(X_MODEL)
    wv = np.array([-1e-30, -1e-20, -1e-10, -1e-6, -2e-5], np.float64)
    nst = min(40, 4096 // nsec)
    j = np.arange(5) % nst
    t = ec.stations_t(j, 0.5, t0=T_MIN)
    xyz = (t[:, None] * f["a"] + 2.125 * f["u"] + wv[:, None] * f["v"]).astype(np.float32)
    info, count, mean, mn, mx, res, cell = ctx.surfaceMap(xyz, X_MODEL, None, n_stations=nst, n_sectors=nsec, gate=0.25)
    assert np.array_equal(cell, j * nsec + nsec - 1) and info["mapped"] == 5
    r = sn.points(xyz, None, info["o"], info["a"], info["u"], info["v"], float(info["R"]),
                  sn.params(n_stations=nst, n_sectors=nsec))
    assert np.abs(res.astype(np.float64) - r["e"]).max() <= 5e-6
    c2, m2, lo2, hi2 = sn.cells_from(res, cell, nst * nsec)             # (the device's own e: this cloud is not exact)
    assert np.array_equal(count.reshape(-1), c2) and count.sum() == 5
    for a, b in ((mean, m2), (mn, lo2), (mx, hi2)):
        assert np.array_equal(_bits(a), _bits(b))


def _bytes(v):
    return np.atleast_1d(np.asarray(v)).view(np.uint8)


def _same(a, b):
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert np.array_equal(_bytes(a[0][k]), _bytes(b[0][k])), k
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(_bytes(x), _bytes(y))


def test_a_call_leaves_nothing_behind(gm):
    """64 x 64, 1 x 1, a call without a model and 40 x 90 on one context: each equals the same call on a fresh context,
    byte for byte (the last block re-zeroes the table, the class counters and the ticket)."""
    calls = []
    for grid, model in (("64x64", X_MODEL), ("1x1", X_MODEL), ("40x90", [np.nan] * 7), ("40x90", X_MODEL)):
        nst, nsec, gate = GRIDS[grid]
        b = _base(gate, nsec)
        s = ec.sprinkle(ec.fill(b, 20_000, nst, t0=T_MIN, seed=8), ec.fillers(b, gate, nst, nsec, t0=T_MIN))
        calls.append((ec.xyz(s, sn.map_frame(X_MODEL)), model, s["labels"], dict(n_stations=nst, n_sectors=nsec, gate=gate), s))
    with gm.GeometricMapping() as c:
        chained = [c.surfaceMap(x, m, lab, **kw) for x, m, lab, kw, _ in calls]
    for (x, m, lab, kw, s), got in zip(calls, chained):
        with gm.GeometricMapping() as c:
            _same(got, c.surfaceMap(x, m, lab, **kw))
        if np.isnan(m[0]):
            assert got[0]["status"] == _lib.GM_SURF_NO_MODEL and not got[1].any() and (got[6] == -1).all()
            assert got[0]["mapped"] == got[0]["outside"] == got[0]["beyond_gate"] == got[0]["plane"] == 0
        else:
            _check(got, s, kw["n_stations"], kw["n_sectors"], kw["gate"])
