"""GPU tests of k_wall_add (csrc/k_wall.hip) on small clouds whose fp32 per-point chain is exact
(tests/exact_cloud_np.py): the per-point residual and cell, the raw map, the records and the totals are compared bit for
bit with values computed from the builder and the host twin (wall_np.add_frame) alone -- never from what the device
reported -- at the wave, trip and block edges of the kernel under every grid rule (GM_WALL_POINTS_PER_BLOCK), on
per-wave cell patterns, at both edges of the LDS station window (the direct-to-map path beside it), at the stated edges
of the rule (include/gm_hip.h) and over several adds and clears of one map."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cloud_np as ec  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
DS = 0.25
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], float)
SHIFT = np.array([[1, 0, 0, 12.5], [0, 1, 0, 0], [0, 0, 1, 0]], float)       # anchor 50, o' = 0
SHIFT8 = np.array([[1, 0, 0, 12.625], [0, 1, 0, 0], [0, 0, 1, 0]], float)    # anchor 50, o' = (-0.125, 0, 0)
ROLL = np.array([[1, 0, 0, 12.5], [0, 0, -1, 0], [0, 1, 0, 0]], float)        # 90 degrees about x
YAW = np.array([[0, -1, 0, 3.0], [1, 0, 0, 0], [0, 0, 1, 0]], float)          # 90 degrees about z: a' = (0, -1, 0), anchor 12
POSES = dict(identity=IDENTITY, shift=SHIFT, shift8=SHIFT8, roll=ROLL, yaw=YAW)
PPB = [None, "1024", "64"]                                                     # GM_WALL_POINTS_PER_BLOCK
# n_sectors, gate (a finer grid takes a wider gate: enough base points per sector for the runs)
GRIDS = {"90": (90, 0.25), "1": (1, 0.25), "64": (64, 1.0), "4096": (4096, 8.0)}
# as the surface map's, and the steps of wall_blocks: 2048 points per block up to 48 blocks, 8192 from there
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385, 32769,
         48 * 2048 - 1, 48 * 2048, 48 * 2048 + 1)


@functools.lru_cache(maxsize=None)
def _base(gate, n_sectors):
    return ec.base_points(gate, n_sectors)


@pytest.fixture(scope="module")
def ctx(gm):
    with gm.GeometricMapping() as c:
        yield c


@pytest.fixture(params=PPB, ids=lambda v: "ppb_" + str(v))
def ppb(request, monkeypatch):
    """The wall add's grid knob, read when a map is created."""
    if request.param is None:
        monkeypatch.delenv("GM_WALL_POINTS_PER_BLOCK", raising=False)
    else:
        monkeypatch.setenv("GM_WALL_POINTS_PER_BLOCK", request.param)
    return request.param


class Ledger:
    """What a map must hold: the (e, cell) pairs of every add so far, from the builder."""

    def __init__(self, wm, prm):
        self.wm, self.prm = wm, prm
        self.design = wn.design_frame(prm)
        self.e, self.cell, self.counts, self.frames = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)], np.zeros(4, np.int64), 0

    def add(self, s, pose):
        p = self.prm
        f = wn.add_frame(self.design, p, pose)
        info, res, cell = self.wm.add_points(ec.xyz(s, f), pose, s["labels"])
        assert info["anchor_station"] == f["anchor"] and info["status"] == self.design["status"]
        for k in ("o", "a", "u", "v"):
            assert np.array_equal(info[k].astype(np.float64), f[k]), k
        for k, v in (("R", f["R"]), ("station_length", f["ds"]), ("gate", f["gate"]), ("sector_angle", f["dtheta"])):
            assert float(info[k]) == v, k
        exp = ec.expected(s, p["gate"], p["station_length"], p["n_stations"], p["n_sectors"], j0=f["anchor"])
        ec.same_points(res, cell, exp)
        self.e.append(exp["e"])
        self.cell.append(exp["cell"])
        self.counts += exp["counts"]
        self.frames += 1
        return exp

    def clear(self, s0, n):
        self.wm.clear(s0, n)
        ns = self.prm["n_sectors"]
        for c in self.cell:
            c[(c >= s0 * ns) & (c < (s0 + n) * ns)] = -1

    def raw(self):
        return wn.cells_from(np.concatenate(self.e), np.concatenate(self.cell), self.prm["n_stations"] * self.prm["n_sectors"])

    def check(self):
        want = self.raw()
        got = self.wm.read_raw()
        assert got.dtype == want.dtype and np.array_equal(got.reshape(-1).view(np.uint8), want.view(np.uint8))
        for a, b in zip(self.wm.read(), wn.records_from(want)):
            assert np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint32), b.view(np.uint32))
        i = self.wm.info()
        assert tuple(i[k] for k in ("mapped", "outside", "beyond_gate", "plane")) == tuple(int(c) for c in self.counts)
        assert i["frames"] == self.frames and i["cells_hit"] == int((want["count"] > 0).sum())
        return want


def _map(ctx, **kw):
    prm = wn.params(**kw)
    return ctx.wall_map(**kw), prm


@pytest.mark.parametrize("name", list(POSES))
def test_add_frame_is_the_twins(ctx, name):
    """Dyadic translations and signed permutations: the host's fp64 frame arithmetic is exact, the info equals the twin."""
    wm, prm = _map(ctx, n_stations=72)
    with wm:
        f = wn.add_frame(wn.design_frame(prm), prm, POSES[name])
        assert f["anchor"] == dict(identity=0, shift=50, shift8=50, roll=50, yaw=12)[name]
        assert np.array_equal(f["o"], [-0.125, 0, 0] if name == "shift8" else [0, 0, 0])
        for k in ("a", "u", "v"):
            assert sorted(np.abs(f[k])) == [0, 0, 1]
        led = Ledger(wm, prm)
        b = _base(0.25, 90)
        s = ec.sprinkle(ec.fill(b, 3000, 40, t0=-5.0, seed=11), ec.fillers(b, 0.25, 22, 90))
        exp = led.add(s, POSES[name])
        led.check()
        assert all(exp["counts"]) and (name != "identity" or exp["counts"][1] > 1000)     # below station 0: outside


@pytest.mark.parametrize("grid", list(GRIDS))
def test_sizes(ctx, ppb, grid):
    nsec, gate = GRIDS[grid]
    b = _base(gate, nsec)
    full = ec.sprinkle(ec.fill(b, max(SIZES), 40, t0=-5.0, seed=12), ec.fillers(b, gate, 22, nsec))
    for n in SIZES:
        wm, prm = _map(ctx, n_stations=72, n_sectors=nsec, gate=gate)
        with wm:
            led = Ledger(wm, prm)
            led.add(ec.take(full, np.arange(n)), SHIFT8 if n % 2 else SHIFT)
            led.check()


@pytest.mark.parametrize("grid", ["90", "64", "4096"])
def test_run_patterns(ctx, ppb, grid):
    nsec, gate = GRIDS[grid]
    b = _base(gate, nsec)
    pats = ec.patterns(b, ec.fillers(b, gate, 42, nsec, t0=-5.0), 40, nsec, t0=-5.0)   # the outside filler: station 72
    wm, prm = _map(ctx, n_stations=72, n_sectors=nsec, gate=gate)
    with wm:
        led = Ledger(wm, prm)
        for i, (name, s) in enumerate(pats.items()):
            led.add(s, (SHIFT, SHIFT8, ROLL)[i % 3])
            led.check()
        led.add(ec.concat(*pats.values()), YAW)                          # other lanes, other stations
        want = led.check()
        assert np.any((want["count"] > 0) & (want["sum"] == 0))           # a sum that cancels to 0 with count > 0


def _at_stations(b, js, per, ds=DS, frac=(0.25, 0.5, 0.0, 0.75)):
    """`per` points in each of the stations js (relative to the anchor), in runs of 5 of one sector."""
    parts = []
    secs = [k for k in np.unique(b["sector"]) if (b["sector"] == k).sum() >= 3]
    for i, j in enumerate(js):
        idx = np.concatenate([ec.run_indices(b, secs[(i + 3 * r) % len(secs)], 5, ec.WHERE[(i + r) % len(ec.WHERE)])
                              for r in range(per // 5)])
        fr = np.asarray(frac)[np.arange(len(idx)) // 5 % len(frac)]
        t = ec.stations_t(j, fr, ds)
        parts.append(ec.spec(b, idx, t.astype(np.float32).astype(np.float64)))
    return ec.concat(*parts)


def test_both_sides_of_the_lds_window(ctx, ppb):
    """90 sectors and the context's 5 m box: the LDS window is stations -21 .. 22 around the anchor; -23, -22, 23 and 24
    go to the map directly, in the same add."""
    b = _base(0.25, 90)
    js = [-23, -22, -21, -20, -1, 0, 21, 22, 23, 24]
    for pose, nst in ((SHIFT8, 128), (ROLL, 74), (IDENTITY, 24)):
        wm, prm = _map(ctx, n_stations=nst)
        with wm:
            led = Ledger(wm, prm)
            s = _at_stations(b, js, 60)
            far = ec.spec(b, np.arange(16), np.repeat(np.float32([1e17, -1e17, 1e18, -1e18, 1e30, -1e30, 3e38, -3e38]), 2)
                          .astype(np.float64))                           # the 4e18 guard of the station conversion
            exp = led.add(ec.concat(s, far), pose)
            led.check()
            anchor = 0 if pose is IDENTITY else 50
            n_in = sum(60 for j in js if 0 <= anchor + j < nst)
            assert exp["counts"] == (n_in, 600 - n_in + 16, 0, 0) and n_in >= 240
            assert np.all(exp["cls"][600:] == ec.OUTSIDE)


def test_one_station_window_of_4096_sectors(ctx, ppb):
    b = _base(8.0, 4096)
    wm, prm = _map(ctx, n_stations=64, n_sectors=4096, gate=8.0)
    with wm:
        led = Ledger(wm, prm)
        exp = led.add(_at_stations(b, [-2, -1, 0, 1, 2, 13, 14], 100), SHIFT8)     # 50 + 14 = n_stations: outside
        led.check()
        assert exp["counts"] == (600, 100, 0, 0)


def test_window_on_two_centimetre_stations(ctx, ppb):
    """n_stations = 2500, station_length = 0.02: the 5 m box covers 500 stations, the LDS window the 45 around the
    anchor (-22 .. 22).  0.02 is not an fp32 number: the points sit in the middle of their stations."""
    kw = dict(n_stations=2500, station_length=0.02)
    prm = wn.params(**kw)
    pose = IDENTITY.copy()
    pose[0, 3] = 1000 * 0.02
    f = wn.add_frame(wn.design_frame(prm), prm, pose)
    assert f["anchor"] == 1000 and not f["o"].any()
    b = _base(0.25, 90)
    wm, prm = _map(ctx, **kw)
    with wm:
        led = Ledger(wm, prm)
        js = [-250, -24, -23, -22, -21, 0, 21, 22, 23, 24, 249]
        exp = led.add(_at_stations(b, js, 60, ds=0.02, frac=(0.5,)), pose)
        led.check()
        assert exp["counts"] == (660, 0, 0, 0)
        assert np.array_equal(np.unique(exp["cell"] // 90), 1000 + np.array(js))
    wm, prm = _map(ctx, **kw)
    with wm:                                                             # below station 0
        led = Ledger(wm, prm)
        exp = led.add(_at_stations(b, [-2, -1, 0, 1], 60, ds=0.02, frac=(0.5,)), IDENTITY)
        led.check()
        assert exp["counts"] == (120, 120, 0, 0)


def test_rules(ctx, ppb):
    """The closed-left station edge, both map ends, |e| == gate in both signs, e == 8 at gate 8, the axis point, rows
    that are not finite."""
    b = _base(0.25, 90)
    n = len(b["e"])
    wm, prm = _map(ctx, n_stations=72)
    with wm:
        led = Ledger(wm, prm)
        on_edge = ec.spec(b, np.arange(n), ec.stations_t(np.arange(n) % 40 - 20, 0.0))          # t == j ds
        below = ec.spec(b, np.arange(40), float(np.nextafter(np.float32(-12.5), np.float32(-np.inf))))   # station -1
        first = ec.spec(b, np.arange(40), -12.5)                                                # station 0
        past = ec.spec(b, np.arange(40), ec.stations_t(22, 0.0))                                # station 72 = n_stations
        last = ec.spec(b, np.arange(40), float(np.nextafter(np.float32(5.5), np.float32(0))))    # station 71
        exp = led.add(ec.concat(on_edge, below, first, past, last), SHIFT)
        led.check()
        assert np.array_equal(exp["cell"][:n] // 90, 50 + np.arange(n) % 40 - 20)
        assert np.array_equal(exp["cls"][n:], np.repeat([ec.OUTSIDE, ec.MAPPED, ec.OUTSIDE, ec.MAPPED], 40))
        assert np.all(exp["cell"][n + 40:n + 80] // 90 == 0) and np.all(exp["cell"][n + 120:] // 90 == 71)
    _, _, e_all = ec.all_points(8.0)
    mags = np.intersect1d(e_all[e_all > 0], -e_all[e_all < 0])
    for g in (float(mags[0]), float(mags[-1])):
        bg, far = _base(g, 90), ec.beyond_points(g, 90)
        wm, prm = _map(ctx, n_stations=96, gate=g)
        with wm:
            led = Ledger(wm, prm)
            s = ec.concat(ec.spec(bg, np.arange(len(bg["e"])), ec.stations_t(np.arange(len(bg["e"])) % 40 - 20, 0.5)),
                          ec.spec(far, np.arange(len(far["e"])), ec.stations_t(np.arange(len(far["e"])) % 40 - 20, 0.5)))
            exp = led.add(s, SHIFT8)
            led.check()
            at = np.abs(s["e"]) == np.float32(g)
            assert np.all(exp["cls"][at] == ec.MAPPED) and {-1.0, 1.0} <= set(np.sign(s["e"][at]))
            assert exp["counts"][2] == len(far["e"]) > 0
    b8 = _base(8.0, 90)
    wm, prm = _map(ctx, n_stations=96, gate=8.0)
    with wm:
        led = Ledger(wm, prm)
        at = np.flatnonzero(b8["e"] == np.float32(8.0))
        s = ec.concat(ec.spec(b8, np.resize(at, 200), ec.stations_t(-20, 0.5)), ec.fill(b8, 1000, 39, t0=-4.75, seed=13))
        ec.set_rows(s, [205, 264, 900], {k: v[0] for k, v in ec.axis_point(ec.stations_t(3, 0.25)).items()})
        s["bad"][[207, 263, 328, 329]] = ec.NAN_ROW
        s["bad"][[209, 265, 400]] = ec.POS_INF_ROW
        s["bad"][[210, 266, 401]] = ec.NEG_INF_ROW
        exp = led.add(s, SHIFT)
        want = led.check()
        first = want[30 * 90:31 * 90]
        hit = first["count"] > 0
        assert first["count"].sum() == 200 and np.all(first["sum"][hit] == first["count"][hit].astype(np.int64) << 23)
        assert np.all(exp["cell"][[205, 264, 900]] == 53 * 90)            # on the axis: sector 0, e == -R
        assert np.all(exp["cls"][s["bad"] != 0] == ec.BEYOND) and exp["counts"][2] == 10


@pytest.mark.parametrize("nsec", [1, 3, 64, 90, 360, 4096])
def test_fold_and_clamp_to_the_last_sector(ctx, nsec):
    """w.u > 0 and w.v a tiny negative number: phi = theta + 2 pi rounds to 2 pi, phi / dtheta to n_sectors or just
    below, and the clamp keeps the point in the last sector.  Not an exact cloud: e against the twin at its own 5e-6."""
    wm, prm = _map(ctx, n_stations=72, n_sectors=nsec)
    with wm:
        f = wn.add_frame(wn.design_frame(prm), prm, SHIFT8)
        wv = np.array([-1e-30, -1e-20, -1e-10, -1e-6, -2e-5], np.float64)
        j = np.arange(5) - 2
        t = ec.stations_t(j, 0.5)
        xyz = (f["o"] + t[:, None] * f["a"] + 2.125 * f["u"] + wv[:, None] * f["v"]).astype(np.float32)
        info, res, cell = wm.add_points(xyz, SHIFT8)
        assert np.array_equal(cell, (50 + j) * nsec + nsec - 1)
        r = wn.points(xyz, None, info, prm)
        assert np.abs(res.astype(np.float64) - r["e"]).max() <= 5e-6
        want = wn.cells_from(res, cell, 72 * nsec)                       # (the device's own e: this cloud is not exact)
        assert np.array_equal(wm.read_raw().reshape(-1).view(np.uint8), want.view(np.uint8))
        assert wm.info()["mapped"] == 5


def test_five_adds_and_clears_of_one_map(ctx, ppb):
    b = _base(0.25, 90)
    k = int(np.bincount(b["sector"]).argmax())
    own = ec.of_cell(b, k)
    lo, hi, mid = own[0], own[-1], own[1:-1]
    assert len(mid) >= 1 and b["e"][lo] < b["e"][mid].min() and b["e"][hi] > b["e"][mid].max()
    wm, prm = _map(ctx, n_stations=128)
    with wm:
        led = Ledger(wm, prm)
        rest = {key: (v[b["sector"] != k] if isinstance(v, np.ndarray) else v) for key, v in b.items()}
        fl = ec.fillers(rest, 0.25, 22, 90)
        # station 60 = anchor 50 + 10 = anchor 12 + 48: the minimum of cell (60, k) comes with the first add, the maximum
        # with the last, the adds between bring the middle of the sector
        marks = [(SHIFT8, 10, [lo] + list(mid)), (ROLL, 10, list(mid)), (SHIFT, 10, list(mid) * 2), (IDENTITY, 60, list(mid)),
                 (YAW, 48, list(mid) + [hi])]
        for i, (pose, j, idx) in enumerate(marks):
            s = ec.concat(ec.sprinkle(ec.fill(rest, 3000 + 700 * i, 40, t0=-5.0, seed=20 + i), fl),
                          ec.spec(b, idx, ec.stations_t(j, 0.25 * (i % 4))))
            s = ec.take(s, np.random.default_rng(30 + i).permutation(len(s["t"])))
            led.add(s, pose)
            led.check()
            if i == 1:
                led.clear(35, 20)                                        # stations 35 .. 54: part of what two adds brought
                led.check()
            if i == 3:
                led.clear(0, 8)
                led.clear(61, 67)
                led.check()
        want = led.raw()[60 * 90 + k]
        e_cell = [e[c == 60 * 90 + k] for e, c in zip(led.e, led.cell)]
        assert want["min_key"] == ~wn.ordered(b["e"][lo]) and want["max_key"] == wn.ordered(b["e"][hi])
        assert [bool((e == b["e"][lo]).any()) for e in e_cell[1:]] == [True, False, False, False, False]
        assert [bool((e == b["e"][hi]).any()) for e in e_cell[1:]] == [False, False, False, False, True]
        assert led.frames == 5 and want["count"] == sum(len(e) for e in e_cell)
