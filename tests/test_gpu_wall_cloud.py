"""GPU tests of gm_wall_map_cloud (csrc/k_wall_cloud.hip + gm_wall.hip) against the twin tests/wall_cloud_np.py.
Maps are filled with add_raw; every comparison with the twin is byte equality of the record array and dict equality of
the info, on gm_wall_cloud_directions' table and the design frame the map reports."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth
from geometric_mapping_amd.api import RAW_CELL, WALL_CLOUD_POINT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_np as rn  # noqa: E402
import wall_cloud_np as cn  # noqa: E402
import wall_np as wn  # noqa: E402
from test_wall_regions_abi import E2E, check_e2e  # noqa: E402

pytestmark = pytest.mark.gpu
STRIDES = ((1, 1), (2, 3), (7, 5), (64, 64), (200, 1), (1, 5000))


@contextlib.contextmanager
def chunk(blocks):
    """Maps created inside process a cloud in chunks of `blocks` blocks (whole block rows; None: the default)."""
    old = os.environ.pop("GM_WALL_CLOUD_CHUNK", None)
    if blocks:
        os.environ["GM_WALL_CLOUD_CHUNK"] = str(blocks)
    try:
        yield
    finally:
        os.environ.pop("GM_WALL_CLOUD_CHUNK", None)
        if old is not None:
            os.environ["GM_WALL_CLOUD_CHUNK"] = old


def make(c, raw, blocks=None, **kw):
    """(map, its gm_wall_params dict) holding the raw cells."""
    p = wn.params(n_stations=raw.shape[0], n_sectors=raw.shape[1], **kw)
    with chunk(blocks):
        m = c.wall_map(**p)
    m.add_raw(raw)
    return m, p


def frame_of(m):
    i = m.info()
    return dict(o=i["o"], a=i["a"], u=i["u"], v=i["v"], R=i["R"])


def same_frame(f, d):
    """The reported design frame and wall_np.design_frame's, bit for bit."""
    return all(np.asarray(f[k], np.float64).tobytes() == np.asarray(d[k], np.float64).tobytes() for k in ("o", "a", "u", "v", "R"))


def check(m, p, raw, station0=0, n=None, frame=None, **params):
    """One call against the twin, byte for byte; returns (info, records)."""
    tab = api.wall_cloud_directions(m.prm, **params)
    info, rec = m.cloud(station0, n, **params)
    winfo, wrec = cn.cloud(raw, p, station0, n, tab, frame=frame or frame_of(m), **params)
    assert rec.dtype == WALL_CLOUD_POINT and rec.tobytes() == wrec.tobytes()
    assert info == winfo
    assert np.all(np.diff(rec["block"].astype(np.int64)) > 0)
    assert info["points"] + info["below_min_count"] + info["empty"] == info["blocks"] and len(rec) == info["points"]
    return info, rec


def random_raw(rng, n, ns, fill):
    """Counts 1 .. 20, sums of both signs, keys consistent through wn.ordered."""
    raw = np.zeros((n, ns), RAW_CELL)
    hit = rng.random((n, ns)) < fill
    cnt = rng.integers(1, 21, (n, ns))
    lo = rng.uniform(-0.25, 0.0, (n, ns)).astype(np.float32)
    hi = rng.uniform(0.0, 0.25, (n, ns)).astype(np.float32)
    mean = rng.uniform(lo, hi)
    raw["count"] = np.where(hit, cnt, 0)
    raw["sum"] = np.where(hit, np.rint(mean * cnt * 2.0 ** 20).astype(np.int64), 0)
    raw["min_key"] = np.where(hit, ~wn.ordered(lo), 0)
    raw["max_key"] = np.where(hit, wn.ordered(hi), 0)
    return raw


# ---- 1. grids ----

@pytest.mark.parametrize("ns", (1, 2, 3, 63, 64, 65, 257))
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 129))
def test_grids(gm, n, ns):
    rng = np.random.default_rng(1000 * n + ns)
    with gm.GeometricMapping() as c:
        for fill in (0.0, 0.03, 0.5, 1.0):
            raw = random_raw(rng, n, ns, fill)
            m, p = make(c, raw, t_min=-3.0, radius=2.5)
            f = frame_of(m)
            assert same_frame(f, wn.design_frame(p))   # axis-aligned: the derivation from the parameters, not only its report
            for bs, bk in STRIDES:
                for mc in (1, 8):
                    info, rec = check(m, p, raw, frame=f, block_stations=bs, block_sectors=bk, min_count=mc)
                    if fill == 0.0:
                        assert info["points"] == 0 and info["empty"] == info["blocks"]
                    if mc == 1:
                        assert int(rec["count"].sum()) == int(raw["count"].sum())
                        assert int(rec["cells"].sum()) == int((raw["count"] > 0).sum())
            m.close()


# ---- 2. chunking ----

@pytest.mark.parametrize("shape", ((65, 257), (129, 65)))
def test_chunks_do_not_change_the_bytes(gm, shape):
    n, ns = shape
    raw = random_raw(np.random.default_rng(n), n, ns, 0.5)
    with gm.GeometricMapping() as c:
        whole, p = make(c, raw)
        f = frame_of(whole)
        for bs, bk in ((1, 1), (2, 3), (7, 5)):
            kw = dict(block_stations=bs, block_sectors=bk, min_count=4)
            _, want = check(whole, p, raw, frame=f, **kw)
            NK = -(-ns // bk)
            for blocks in (1, NK, 16 * NK, 16 * NK + NK // 2, 10 ** 9):   # less than a row: one row; ... ; beyond the window
                m, _ = make(c, raw, blocks)
                _, got = check(m, p, raw, frame=f, **kw)
                assert got.tobytes() == want.tobytes()
                _, cut = check(m, p, raw, 3, n - 5, frame=f, **kw)        # a window that ends mid-block, chunked
                assert len(cut) > 0
                m.close()


def test_two_default_chunks(gm):
    """512 x 4096 cells: 2^21 blocks at stride 1, two default chunks; 0.5 % of the cells filled."""
    n, ns = 512, 4096
    raw = random_raw(np.random.default_rng(7), n, ns, 0.005)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        f = frame_of(m)
        info, rec = check(m, p, raw, frame=f)
        assert info["blocks"] == 1 << 21 and info["points"] == int((raw["count"] > 0).sum()) > 9000
        assert rec["block"][0] < (1 << 20) <= rec["block"][-1]          # points on both sides of the chunk boundary
        info, _ = check(m, p, raw, frame=f, block_stations=16, block_sectors=16, min_count=3)
        assert info["blocks"] == 32 * 256 and info["below_min_count"] > 0


# ---- 3. windows ----

def test_windows(gm):
    raw = random_raw(np.random.default_rng(3), 40, 33, 0.6)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        for kw in (dict(), dict(block_stations=7, block_sectors=5), dict(block_stations=64, block_sectors=64)):
            check(m, p, raw, 5, 20, **kw)                # station0 > 0; 20 stations end mid-block at 7
            check(m, p, raw, 39, 1, **kw)
            info, rec = check(m, p, raw, 17, 0, **kw)    # n = 0: no points
            assert info["blocks"] == 0 and info["blocks_stations"] == 0 and len(rec) == 0
            info, rec = check(m, p, raw, 40, 0, **kw)
        _, rec = check(m, p, raw, 5, 20, block_stations=7, block_sectors=33)
        assert rec["block"].tolist() == [0, 1, 2]        # rows of 7, 7 and 6 stations
        assert rec["x"].tolist() == [(5 + 3.5) * 0.25, (12 + 3.5) * 0.25, (19 + 3.0) * 0.25]
        for s0, n in ((39, 2), (41, 0), (0, 41)):
            with pytest.raises(gm.GmError) as e:
                m.cloud(s0, n)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        empty, pe = make(c, np.zeros((9, 12), RAW_CELL))
        info, rec = check(empty, pe, np.zeros((9, 12), RAW_CELL))
        assert info["points"] == 0 and info["empty"] == 108 and len(rec) == 0


# ---- 4. extremes ----

def test_extremes(gm):
    raw = np.zeros((6, 8), RAW_CELL)
    q8 = 8 << 20
    raw[0, 0] = (-q8, 1, ~wn.ordered(np.float32(-8.0)), wn.ordered(np.float32(-8.0)), 0)   # the gate's extreme residuals
    raw[0, 1] = (3 * q8, 3, ~wn.ordered(np.float32(8.0)), wn.ordered(np.float32(8.0)), 0)
    raw[1, 0] = (q8 - q8, 2, ~wn.ordered(np.float32(-8.0)), wn.ordered(np.float32(8.0)), 0)
    raw[3, 5] = (-1, 1, ~wn.ordered(np.float32(-2.0 ** -20)), wn.ordered(np.float32(-2.0 ** -20)), 0)   # sum negative, count 1
    raw[4, 2] = (-123457, 7, ~wn.ordered(np.float32(-0.2)), wn.ordered(np.float32(0.1)), 0)
    raw["count"][5, 6:8] = 0xFFFFFFFF                    # two cells whose counts do not fit 32 bits together
    raw["sum"][5, 6:8] = (-3 << 40, 1 << 41)
    raw["min_key"][5, 6:8] = ~wn.ordered(np.float32(-0.01))
    raw["max_key"][5, 6:8] = wn.ordered(np.float32(0.02))
    designs = (dict(),
               dict(point=(3.0, -1.0, 0.5), direction=(0.3, 0.2, 0.93), up=(0.3, 0.2, 0.93), forward=(0.0, 0.0, 1.0), radius=3.1,
                    station_length=0.3, t_min=-7.7),                       # not axis-aligned, up along the axis: the fallback
               dict(t_min=5000.0))                                          # chainage 5 km
    with gm.GeometricMapping() as c:
        for k, kw in enumerate(designs):
            m, p = make(c, raw, **kw)
            f = frame_of(m)
            assert bool(m.info()["status"] & _lib.GM_SURF_UP_FALLBACK) == (k == 1)
            d = wn.design_frame(p)
            if k == 1:   # oblique: the twin's dot products may differ in the last bit, no more
                assert all(np.allclose(f[key], d[key], rtol=0, atol=1e-14) for key in ("o", "a", "u", "v")) and f["R"] == d["R"]
            else:
                assert same_frame(f, d)
            anchors = [(0.0, 0.0, 0.0), tuple(f["o"] + (p["t_min"] + 0.5) * f["a"])]
            for g in (0.0, 1.0, 50.0):
                for anchor in anchors:
                    for bs, bk in ((1, 1), (2, 2), (6, 8), (1, 2)):
                        info, rec = check(m, p, raw, frame=f, exaggeration=g, anchor=anchor, block_stations=bs, block_sectors=bk)
                        if (bs, bk) == (1, 1):
                            assert rec["mean"][:3].tolist() == [-8.0, 8.0, 0.0] and rec["min"][2] == -8.0 and rec["max"][2] == 8.0
                            assert rec["mean"][3] == np.float32(-2.0 ** -20) and rec["count"][3] == 1
                        if (bs, bk) == (1, 2):
                            assert int(rec["count"][-1]) == 2 * 0xFFFFFFFF and rec["cells"][-1] == 2
                        if g == 0.0:   # every point on the design cylinder itself
                            xyz = np.stack([rec[k] for k in "xyz"], axis=1)
                            q = xyz.astype(np.float64) + np.array(anchor) - f["o"]
                            r = np.linalg.norm(q - np.outer(q @ f["a"], f["a"]), axis=1)
                            assert np.all(np.abs(r - f["R"]) < 3 * np.spacing(np.abs(xyz).max()))
        # the anchor at chainage 5 km gives the bytes of the same map at chainage 0 (axis along x, ds = 0.25)
        near, pn = make(c, raw)
        far, pf = make(c, raw, t_min=5000.0)
        for kw in (dict(), dict(block_stations=2, block_sectors=3, exaggeration=50.0)):
            _, a = check(near, pn, raw, **kw)
            _, b = check(far, pf, raw, anchor=(5000.0, 0.0, 0.0), **kw)
            assert a.tobytes() == b.tobytes()


# ---- 5. capacity and errors ----

def test_capacity_and_errors(gm):
    raw = random_raw(np.random.default_rng(5), 20, 30, 0.4)
    want = int((raw["count"] > 0).sum())
    with gm.GeometricMapping() as c:
        m, p = make(c, raw, 4 * 30)          # five chunks
        L, h = c._L, m._h()
        prm = m.cloud_params()
        info, got = _lib.WallCloudInfo(), C.c_uint64(99)
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), C.byref(info), None, 0, C.byref(got)) == _lib.GM_OK   # the count query
        assert got.value == want == info.points and info.struct_size == C.sizeof(_lib.WallCloudInfo)
        assert info.blocks == 600 and info.empty == 600 - want and info.below_min_count == 0
        buf = np.zeros(want, WALL_CLOUD_POINT)
        bp = buf.ctypes.data_as(C.POINTER(_lib.WallCloudPoint))
        info, got = _lib.WallCloudInfo(), C.c_uint64(99)
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), C.byref(info), bp, want - 1, C.byref(got)) == _lib.GM_ERR_CAPACITY
        assert got.value == want == info.points and info.blocks == 600 and info.empty == 600 - want   # counting went on
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), C.byref(info), bp, 0, C.byref(got)) == _lib.GM_ERR_CAPACITY
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), C.byref(info), bp, want, None) == _lib.GM_OK
        tab = api.wall_cloud_directions(m.prm)
        assert buf.tobytes() == cn.cloud(raw, p, 0, None, tab)[1].tobytes()
        assert L.gm_wall_map_cloud(h, 0, 20, None, C.byref(info), bp, want, C.byref(got)) == _lib.GM_OK   # NULL: the defaults
        assert got.value == want
        bad = _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), None, None, 0, C.byref(got)) == bad
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(prm), C.byref(info), None, 5, C.byref(got)) == bad   # NULL points with a capacity
        for k, v in (("block_stations", 0), ("block_sectors", 0), ("min_count", 0), ("exaggeration", -1.0),
                     ("exaggeration", float("nan")), ("exaggeration", float("inf")), ("struct_size", 8)):
            q = m.cloud_params()
            setattr(q, k, v)
            assert L.gm_wall_map_cloud(h, 0, 20, C.byref(q), C.byref(info), None, 0, None) == bad, (k, v)
        q = m.cloud_params()
        q.anchor[1] = float("nan")
        assert L.gm_wall_map_cloud(h, 0, 20, C.byref(q), C.byref(info), None, 0, None) == bad


# ---- 6. the map is untouched; the regions' scratch is separate ----

def test_cloud_leaves_the_map_and_the_regions_alone(gm):
    T = rn.threshold_q(0.05)
    raw = rn.random_field(np.random.default_rng(9), 160, 90, 0.3, T, RAW_CELL)
    with gm.GeometricMapping() as c:
        a, p = make(c, raw)
        b, _ = make(c, raw)
        f = frame_of(a)
        before = a.read_raw().tobytes()
        wreg = rn.regions(raw, min_cells=2)
        _, wcloud = check(a, p, raw, frame=f, block_stations=3, block_sectors=4)      # cloud, then regions
        info, reg, _, labels = a.regions(labels=True, min_cells=2)
        assert reg.tobytes() == wreg[1].tobytes() and np.array_equal(labels, wreg[2]) and info["regions"] == wreg[0]["regions"]
        info, reg, _, labels = b.regions(labels=True, min_cells=2)                       # regions, then cloud
        assert reg.tobytes() == wreg[1].tobytes() and np.array_equal(labels, wreg[2])
        _, got = check(b, p, raw, frame=f, block_stations=3, block_sectors=4)
        assert got.tobytes() == wcloud.tobytes()
        check(a, p, raw, frame=f)
        assert a.read_raw().tobytes() == before == b.read_raw().tobytes() == raw.tobytes()


# ---- 7. end to end ----

def test_end_to_end_drive(gm):
    drive = synth.tunnel_drive(12, 150_000, seed=21, sigma=0.01)
    p = wn.params(n_stations=208, **drive["design"])
    anchor = (20.0, 0.0, 0.0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in drive["frames"]:
            m.add_points(cloud, pose, outputs=False)
        info, reg, metrics, _ = m.regions(**E2E)
        raw = m.read_raw()
        _, rec = check(m, p, raw, anchor=anchor)
    check_e2e(p, info, reg, metrics)          # the drive is the one the wall-map tests know
    assert len(rec) == int((raw["count"] > 0).sum()) > 10000
    # the rows are where the wall is: in fp64 on the fp32 rows, the distance of xyz + anchor from the design axis (x)
    # minus R is the mean, within 3 fp32 ulps of the largest coordinate magnitude (each component carries at most half)
    q = np.stack([rec[k].astype(np.float64) for k in "xyz"], axis=1) + np.array(anchor)
    r = np.hypot(q[:, 1], q[:, 2])
    big = np.abs(np.stack([rec[k] for k in "xyz"], axis=1)).max(axis=1)
    assert np.all(np.abs((r - 2.0) - rec["mean"].astype(np.float64)) <= 3 * np.spacing(big).astype(np.float64))
    # the three patches stand out of the cloud by their 0.15 m
    j, k = rec["block"] // 90, rec["block"] % 90
    inside = (j >= 40) & (j <= 47) & (k >= 5) & (k <= 10)
    assert inside.sum() == 48 and np.all(np.abs(rec["mean"][inside] - 0.15) < 0.02)


# ---- 8. two maps on one context, a frame in flight ----

def test_two_maps_beside_a_frame_in_flight(gm):
    rng = np.random.default_rng(8)
    ra, rb = random_raw(rng, 65, 257, 0.5), random_raw(rng, 129, 65, 0.3)
    xyz = np.ascontiguousarray(synth.tunnel_frame(300_000, seed=4), dtype=np.float32)
    keys = ("n_in", "n_cropped", "n_valid", "n_voxels", "status_flags")
    with gm.GeometricMapping(n_slots=2) as c:
        ref = c.process_frame(xyz)
        a, pa = make(c, ra)
        b, pb = make(c, rb)
        fa, fb = frame_of(a), frame_of(b)
        ta, tb = api.wall_cloud_directions(a.prm, block_sectors=3), api.wall_cloud_directions(b.prm)
        wa = cn.cloud(ra, pa, 0, None, ta, frame=fa, block_stations=2, block_sectors=3)
        wb = cn.cloud(rb, pb, 0, None, tb, frame=fb)
        c.submit_frame(0, xyz)
        got = []
        for _ in range(3):
            got.append(a.cloud(block_stations=2, block_sectors=3))
            got.append(b.cloud())
        res = c.wait_frame(0)
        for i, (info, rec) in enumerate(got):
            winfo, wrec = (wa, wb)[i % 2]
            assert info == winfo and rec.tobytes() == wrec.tobytes()
        assert {k: res[k] for k in keys} == {k: ref[k] for k in keys}
        for k in ("eigenvalues", "eigenvectors", "center_axis", "scatter6"):
            assert res[k].tobytes() == ref[k].tobytes(), k


# ---- 9. the Python surface ----

def test_python_surface(gm):
    raw = random_raw(np.random.default_rng(2), 10, 12, 0.5)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec = m.cloud()
        assert set(info) == set(cn.INFO_KEYS) and rec.dtype == WALL_CLOUD_POINT
        with pytest.raises(TypeError):
            m.cloud(blocks=3)
        assert m.cloud(station0=4)[0]["n_stations"] == 6
