"""GPU tests of gm_wall_map_regions (csrc/k_wall_regions.hip + gm_wall.hip) against the integer twin tests/regions_np.py.
Maps are filled with add_raw, so no frames are needed; every comparison with the twin is exact (region bytes, info
counts, the labels array): the rule has no floating point in it."""
import contextlib
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth
from geometric_mapping_amd.api import RAW_CELL, REGION

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_np as rn  # noqa: E402
import wall_np as wn  # noqa: E402
from test_wall_regions_abi import E2E, check_e2e  # noqa: E402

pytestmark = pytest.mark.gpu
TS, TK = _lib.GM_WALL_REGION_TILE
T = rn.threshold_q(0.05)
INFO_KEYS = ("station0", "n_stations", "n_sectors", "threshold_q", "flagged_pos", "flagged_neg", "unusable", "empty",
             "components", "regions")


@contextlib.contextmanager
def tile(shape):
    """Maps created inside use the labelling tile `shape` ("<stations>x<sectors>"; None: the default)."""
    old = os.environ.pop("GM_WALL_REGION_TILE", None)
    if shape:
        os.environ["GM_WALL_REGION_TILE"] = shape
    try:
        yield
    finally:
        os.environ.pop("GM_WALL_REGION_TILE", None)
        if old is not None:
            os.environ["GM_WALL_REGION_TILE"] = old


def make(c, raw, shape=None, **kw):
    with tile(shape):
        m = c.wall_map(n_stations=raw.shape[0], n_sectors=raw.shape[1], **kw)
    m.add_raw(raw)
    return m


def check(m, raw, base=None, base_raw=None, station0=0, n=None, want=None, **params):
    """One call against the twin, byte for byte; returns the twin's (info, regions, labels)."""
    info, reg, metrics, labels = m.regions(station0, n, baseline=base, labels=True, **params)
    want = want or rn.regions(raw, base_raw, station0, n, **params)
    winfo, wreg, wlabels = want
    assert reg.dtype == REGION and reg.tobytes() == wreg.tobytes()
    assert {k: info[k] for k in INFO_KEYS} == {k: winfo[k] for k in INFO_KEYS}
    assert labels.dtype == np.int32 and np.array_equal(labels, wlabels)
    p = {k: getattr(m.prm, k) for k in ("n_sectors", "station_length", "t_min", "radius")}
    assert info["cell_area"] == rn.cell_area(p)
    assert metrics == [rn.metrics(p, r) for r in wreg]
    assert np.all(np.diff(reg["label"].astype(np.int64)) > 0)
    return want


def field(shape, cells, q=2 * T, count=8):
    """Raw cells of `shape` with the listed (j, k) at value q (count points each), everything else empty."""
    raw = np.zeros(shape, RAW_CELL)
    for j, k in cells:
        raw[j, k] = (q * count, count, 0, 0, 0)
    return raw


# ---- 1. tile and seam edges ----

@pytest.mark.parametrize("ns", (1, 2, 3, TK - 1, TK, TK + 1, 257))
@pytest.mark.parametrize("n", (1, 2, TS - 1, TS, TS + 1, 2 * TS + 1))
def test_tile_and_seam_edges(gm, n, ns):
    rng = np.random.default_rng(1000 * n + ns)
    with gm.GeometricMapping() as c:
        for density in (0.35, 0.45, 0.6):   # around the 8- and 4-connected percolation thresholds
            raw = rn.random_field(rng, n, ns, density, T, RAW_CELL)
            m = make(c, raw)
            small = make(c, raw, "3x5")      # many tiles: every border kind inside a small grid
            for conn in (4, 8):
                for min_cells in (1, 5):
                    want = check(m, raw, connectivity=conn, min_cells=min_cells)
                    check(small, raw, want=want, connectivity=conn, min_cells=min_cells)
            m.close()
            small.close()


# ---- 2. snake ----

def snake(n=130, ns=67):
    raw = np.zeros((n, ns), RAW_CELL)
    for j in range(n):
        if j % 2 == 0:
            for k in range(1, ns - 1):
                raw[j, k] = (2 * T * 8, 8, 0, 0, 0)
        else:
            kc = ns - 2 if (j // 2) % 2 == 0 else 1          # the connector to the next even station
            raw[j, kc] = (2 * T * 8, 8, 0, 0, 0)
            for k in range(1, ns - 1):
                if abs(k - kc) > 1:                           # the free cells that do not touch it: the other sign
                    raw[j, k] = (-3 * T * 9, 9, 0, 0, 0)
    return raw


def test_snake_is_one_region_under_every_tile(gm):
    raw = snake()
    n, ns = raw.shape
    want = rn.regions(raw, connectivity=4, min_cells=1)
    _, wreg, _ = want
    pos = wreg[wreg["sign"] > 0]
    assert len(pos) == 1 and pos[0]["label"] == 1 and pos[0]["cells"] == (n // 2) * (ns - 2) + n // 2 > 4000
    assert (pos[0]["station_min"], pos[0]["station_max"], pos[0]["sector_min"], pos[0]["sector_max"]) == (0, n - 1, 1, ns - 2)
    neg = wreg[wreg["sign"] < 0]
    assert len(neg) == n // 2 and np.all(neg["cells"] == ns - 4) and np.all(neg["station_min"] == neg["station_max"])
    got = []
    with gm.GeometricMapping() as c:
        for shape in (None, "5x13", "1x4096", "64x1"):
            m = make(c, raw, shape)
            check(m, raw, want=want, connectivity=4, min_cells=1)
            got.append(m.regions(connectivity=4, min_cells=1)[1].tobytes())
    assert all(g == got[0] for g in got)


# ---- 3. rings and the seam ----

def test_rings_and_seam(gm):
    ns = 90
    ring = field((5, ns), [(2, k) for k in range(ns)])
    patch = field((6, ns), [(j, k) for j in (2, 3) for k in (88, 89, 0, 1)], q=-2 * T)
    # two pairs that touch only diagonally across the seam; (2, 0) and (4, 0) share no neighbour, so the pairs stay apart
    diag = field((6, ns), [(1, ns - 1), (2, 0), (4, 0), (5, ns - 1)])
    with gm.GeometricMapping() as c:
        _, reg, _ = check(make(c, ring), ring, min_cells=1)
        assert len(reg) == 1 and reg[0]["cells"] == ns and reg[0]["label"] == 2 * ns
        assert (reg[0]["sector_min"], reg[0]["sector_max"], reg[0]["sector_min_turned"], reg[0]["sector_max_turned"]) == (0, ns - 1, 0, ns - 1)
        m = make(c, patch)
        _, reg, _ = check(m, patch, min_cells=1)
        assert len(reg) == 1 and reg[0]["sign"] == -1 and reg[0]["cells"] == 8 and reg[0]["label"] == 2 * ns
        assert (reg[0]["sector_min"], reg[0]["sector_max"]) == (0, 89)                       # the plain extent is the whole ring,
        assert (reg[0]["sector_min_turned"], reg[0]["sector_max_turned"]) == (43, 46)        # the turned one is tight
        met = m.regions(min_cells=1)[2][0]
        assert (met["angle_from_deg"], met["angle_to_deg"]) == (352.0, 8.0)
        m = make(c, diag)
        _, reg8, _ = check(m, diag, min_cells=1, connectivity=8)
        _, reg4, _ = check(m, diag, min_cells=1, connectivity=4)
        assert reg8["cells"].tolist() == [2, 2] and reg4["cells"].tolist() == [1, 1, 1, 1]
        for ns_small in (1, 2):   # the modulus alone: no special case
            col = field((4, ns_small), [(0, 0), (1, ns_small - 1), (3, 0)])
            for conn in (4, 8):
                check(make(c, col), col, min_cells=1, connectivity=conn)


# ---- 4. usability and the threshold ----

def test_usability_and_threshold(gm):
    raw = field((7, 8), [(j, k) for j in range(5) for k in (2, 3, 4)])
    raw["count"][2, 2:5] = 7                      # min_count - 1: the row splits the region
    edge = np.zeros((4, 8), RAW_CELL)
    edge[0, 1] = (T * 9, 9, 0, 0, 0)              # q = T: flagged
    edge[0, 2] = (T * 9 - 1, 9, 0, 0, 0)          # q = T - 1: not
    edge[2, 5] = (-T * 9, 9, 0, 0, 0)             # q = -T: flagged
    edge[2, 6] = (-T * 9 + 1, 9, 0, 0, 0)         # toward zero: q = -(T - 1), not flagged (a floor would give -T)
    with gm.GeometricMapping() as c:
        info, reg, _ = check(make(c, raw), raw, min_cells=1)
        assert reg["cells"].tolist() == [6, 6] and info["unusable"] == 3 and info["empty"] == 7 * 8 - 15
        info, reg, lab = check(make(c, edge), edge, min_cells=1)
        assert reg["label"].tolist() == [1, 2 * 8 + 5] and reg["sign"].tolist() == [1, -1] and reg["cells"].tolist() == [1, 1]
        assert reg["peak"].tolist() == [T, -T] and info["flagged_pos"] == info["flagged_neg"] == 1
        check(make(c, raw), raw, min_cells=1, min_count=7)   # the thin row is usable now: one region
        assert c.wall_map(n_stations=7, n_sectors=8).regions()[0]["empty"] == 56


# ---- 5. window ----

def test_window(gm):
    raw = field((12, 10), [(j, k) for j in range(3, 9) for k in (4, 5)] + [(11, 9), (11, 0)])
    with gm.GeometricMapping() as c:
        m = make(c, raw)
        check(m, raw, min_cells=1)
        _, reg, lab = check(m, raw, station0=5, n=4, min_cells=1)
        assert len(reg) == 1 and reg[0]["label"] == 5 * 10 + 4 and reg[0]["cells"] == 8
        assert (reg[0]["station_min"], reg[0]["station_max"]) == (5, 8) and lab.shape == (4, 10) and lab[0, 4] == 54
        info, reg, lab = check(m, raw, station0=4, n=0, min_cells=1)
        assert len(reg) == 0 and lab.shape == (0, 10) and info["components"] == 0
        _, reg, _ = check(m, raw, station0=11, n=1, min_cells=1)
        assert len(reg) == 1 and reg[0]["label"] == 110 and reg[0]["cells"] == 2 and reg[0]["peak_cell"] == 110
        with pytest.raises(gm.GmError) as e:
            m.regions(station0=11, n=2)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG


# ---- 6. baseline ----

def test_baseline(gm):
    rng = np.random.default_rng(6)
    a = rn.random_field(rng, 70, 33, 0.3, T, RAW_CELL)
    b = rn.random_field(rng, 70, 33, 0.3, T, RAW_CELL)
    with gm.GeometricMapping() as c, gm.GeometricMapping() as other:
        ma, mb = make(c, a), make(c, b)
        for conn in (4, 8):
            info, _, _ = check(ma, a, base=mb, base_raw=b, connectivity=conn, min_cells=2)
        thin = (a["count"] < 8) | (b["count"] < 8)
        assert info["unusable"] + info["empty"] == int(thin.sum()) and info["empty"] == int(((a["count"] == 0) & (b["count"] == 0)).sum())
        check(ma, a, base=mb, base_raw=b, station0=60, n=10, min_cells=1)
        copy = make(c, ma.read_raw())
        info, reg, _ = check(ma, a, base=copy, base_raw=a, min_cells=1)
        assert len(reg) == 0 and info["flagged_pos"] == info["flagged_neg"] == 0
        refused = [ma, make(other, b), make(c, b, t_min=0.125), make(c, b[:69]), make(c, b, radius=2.5)]
        for bad in refused:
            with pytest.raises(gm.GmError) as e:
                ma.regions(baseline=bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        ma.regions(baseline=make(c, b, gate=0.5))   # the gate may differ


# ---- 7. the largest map, once ----

def test_largest_map(gm):
    n = ns = 4096
    raw = np.zeros((n, ns), RAW_CELL)
    k = np.arange(ns, dtype=np.int64)
    raw["count"][::3] = 8
    raw["sum"][::3] = (2 * T + k) * 8 + 3            # d = 2 T + k: the peak is the last sector
    with gm.GeometricMapping() as c:
        m = make(c, raw)
        info, reg, _, lab = m.regions(labels=True)
    rings = np.arange(0, n, 3, dtype=np.int64)
    assert len(reg) == info["regions"] == info["components"] == -(-n // 3) == len(rings)
    assert info["flagged_pos"] == len(rings) * ns and info["flagged_neg"] == info["unusable"] == 0
    assert info["empty"] == (n - len(rings)) * ns
    assert np.array_equal(reg["label"], rings * ns) and np.all(reg["sign"] == 1) and np.all(reg["cells"] == ns)
    assert np.array_equal(reg["station_min"], rings) and np.array_equal(reg["station_max"], rings)
    for f in ("sector_min", "sector_min_turned"):
        assert np.all(reg[f] == 0)
    for f in ("sector_max", "sector_max_turned"):
        assert np.all(reg[f] == ns - 1)
    assert np.array_equal(reg["peak_cell"], rings * ns + ns - 1) and np.all(reg["peak"] == 2 * T + ns - 1)
    assert np.all(reg["sum_d"] == 2 * T * ns + ns * (ns - 1) // 2) and np.all(reg["points"] == 8 * ns)
    want = np.full((n, ns), -1, np.int32)
    want[::3] = (rings * ns).astype(np.int32)[:, None]
    assert np.array_equal(lab, want)


# ---- 8. capacity and errors ----

def test_capacity_and_errors(gm):
    import ctypes as C
    raw = field((9, 12), [(0, 0), (0, 1), (4, 5), (4, 6), (8, 11), (8, 0)])
    with gm.GeometricMapping() as c:
        m = make(c, raw)
        L, h = c._L, m._h()
        p = m.region_params(min_cells=2)
        info, got = _lib.WallRegionsInfo(), C.c_uint32(99)
        assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(p), C.byref(info), None, 0, C.byref(got), None) == _lib.GM_OK
        assert got.value == 3 == info.regions and info.struct_size == C.sizeof(_lib.WallRegionsInfo)
        buf = np.frombuffer(bytearray(b"\x55" * 192), dtype=REGION)
        keep = buf.tobytes()
        bp = buf.ctypes.data_as(C.POINTER(_lib.WallRegion))
        got = C.c_uint32(99)
        assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(p), C.byref(info), bp, 2, C.byref(got), None) == _lib.GM_ERR_CAPACITY
        assert got.value == 3 and info.regions == 3 and buf.tobytes() == keep
        assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(p), C.byref(info), bp, 3, None, None) == _lib.GM_OK
        assert buf["label"].tolist() == [0, 4 * 12 + 5, 8 * 12]
        assert L.gm_wall_map_regions(h, None, 0, 9, None, C.byref(info), None, 0, None, None) == _lib.GM_OK   # NULL: defaults
        assert info.regions == 0 and info.components == 3 and info.threshold_q == T
        assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(p), None, None, 0, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(p), C.byref(info), None, 2, None, None) == _lib.GM_ERR_INVALID_ARG
        for bad in (dict(min_count=0), dict(min_cells=0), dict(connectivity=6), dict(threshold=0.0), dict(threshold=8.5),
                    dict(threshold=float("nan")), dict(threshold=1e-9), dict(struct_size=8)):
            q = m.region_params()
            for k, v in bad.items():
                setattr(q, k, v)
            assert L.gm_wall_map_regions(h, None, 0, 9, C.byref(q), C.byref(info), None, 0, None, None) == _lib.GM_ERR_INVALID_ARG, bad
        assert m.regions(threshold=8.0)[0]["threshold_q"] == 8 << 20


# ---- 9. isolation ----

def test_regions_leave_the_maps_alone(gm):
    rng = np.random.default_rng(9)
    a = rn.random_field(rng, 160, 90, 0.2, T, RAW_CELL)
    b = rn.random_field(rng, 160, 90, 0.2, T, RAW_CELL)
    xyz, pose = synth.tunnel_drive(1, 100_000, seed=3)["frames"][0]
    with gm.GeometricMapping() as c:
        ma, mb, fresh = make(c, a), make(c, b), make(c, a)
        before = ma.read_raw().tobytes(), mb.read_raw().tobytes()
        ma.regions(baseline=mb, labels=True, min_cells=1)
        ma.regions(station0=20, n=50)
        assert (ma.read_raw().tobytes(), mb.read_raw().tobytes()) == before
        c.process_frame(xyz)
        ma.add_frame(0, pose)
        fresh.add_frame(0, pose)
        assert ma.read_raw().tobytes() == fresh.read_raw().tobytes() != before[0]
        assert ma.info()["mapped"] == fresh.info()["mapped"] > 0


# ---- 10. end to end ----

def test_end_to_end_drive(gm):
    drive = synth.tunnel_drive(12, 150_000, seed=21, sigma=0.01)
    p = wn.params(n_stations=208, **drive["design"])
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in drive["frames"]:
            m.add_points(cloud, pose, outputs=False)
        info, reg, metrics, labels = m.regions(labels=True, **E2E)
        raw = m.read_raw()
    check_e2e(p, info, reg, metrics)
    # (the device's per-point cells differ from the fp64 twin's at ambiguous edge points only, so the structure is
    # asserted above; on the device's own cells the rule is exact)
    winfo, wreg, wlabels = rn.regions(raw, **E2E)
    assert reg.tobytes() == wreg.tobytes() and np.array_equal(labels, wlabels)
    assert {k: info[k] for k in INFO_KEYS} == {k: winfo[k] for k in INFO_KEYS}
