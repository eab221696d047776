"""GPU tests of gm_wall_map_mesh (csrc/k_wall_mesh.hip + gm_wall.hip) against the twin tests/wall_mesh_np.py.
Maps are filled with add_raw; the triangles and the info equal the twin byte for byte, the vertices equal WallMap.cloud()
of the same parameters byte for byte (and through it the cloud's twin)."""
import contextlib
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth
from geometric_mapping_amd.api import RAW_CELL, WALL_CLOUD_POINT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_cloud_np as cn  # noqa: E402
import wall_mesh_np as mn  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTWARD, NO_WRAP = _lib.GM_WALL_MESH_OUTWARD, _lib.GM_WALL_MESH_NO_WRAP
BLOCKS = ((1, 1), (2, 3), (7, 5))


def cp_tile():
    """kCpTile of csrc/gm_compact.hpp: the slots one block of the triangle pass takes."""
    src = open(os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_compact.hpp")).read()
    threads = int(re.search(r"#define GM_CPTHREADS (\d+)", src).group(1))
    items = int(re.search(r"#define GM_CPITEMS (\d+)", src).group(1))
    assert "kCpTile = kCpThreads * kCpItems" in src
    return threads * items


@contextlib.contextmanager
def chunk(blocks):
    """Maps created inside walk a window in chunks of `blocks` blocks (whole block rows; None: the default)."""
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
    p = wn.params(n_stations=raw.shape[0], n_sectors=raw.shape[1], **kw)
    with chunk(blocks):
        m = c.wall_map(**p)
    m.add_raw(raw)
    return m, p


def frame_of(m):
    i = m.info()
    return dict(o=i["o"], a=i["a"], u=i["u"], v=i["v"], R=i["R"])


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


def check(m, p, raw, station0=0, n=None, frame=None, flags=0, max_step=0.0, cloud=True, **params):
    """One call against the twin and against cloud(), byte for byte; returns (info, vertices, triangles)."""
    tab = api.wall_cloud_directions(m.prm, **params)
    info, v, tri = m.mesh(station0, n, flags, max_step, **params)
    winfo, wv, wtri = mn.mesh(raw, p, station0, n, tab, frame=frame or frame_of(m), flags=flags, max_step=max_step, **params)
    assert v.dtype == WALL_CLOUD_POINT and v.tobytes() == wv.tobytes()
    assert tri.dtype == np.uint32 and tri.shape == wtri.shape and tri.tobytes() == wtri.tobytes()
    assert info == winfo
    if cloud:
        cinfo, cv = m.cloud(station0, n, **params)
        assert cinfo == info["cloud"] and cv.tobytes() == v.tobytes()
    assert info["quads"] == info["quads_two"] + info["quads_one"] + info["quads_none"]
    assert info["triangles"] == 2 * info["quads_two"] + info["quads_one"] - info["cut_by_step"] == len(tri)
    assert np.all(tri < max(len(v), 1))
    return info, v, tri


# ---- 1. grids ----

@pytest.mark.parametrize("shape", ((1, 1), (2, 3), (3, 3), (65, 257), (129, 257)))
def test_grids(gm, shape):
    n, ns = shape
    rng = np.random.default_rng(1000 * n + ns)
    with gm.GeometricMapping() as c:
        for fill in (1.0, 0.5):
            raw = random_raw(rng, n, ns, fill)
            m, p = make(c, raw, t_min=-3.0, radius=2.5)
            f = frame_of(m)
            for bs, bk in BLOCKS:
                for mc, flags, step in ((1, 0, 0.0), (8, OUTWARD, 0.1), (1, NO_WRAP, 0.05), (30, OUTWARD | NO_WRAP, 0.0)):
                    info, v, tri = check(m, p, raw, frame=f, flags=flags, max_step=step, cloud=(flags == 0),
                                         block_stations=bs, block_sectors=bk, min_count=mc)
                    if fill == 1.0 and mc == 1 and step == 0.0:
                        assert info["triangles"] == 2 * info["quads"]
                    if mc == 8 and (bs, bk) == (1, 1):
                        assert info["cloud"]["below_min_count"] > 0 or n * ns < 100   # min_count above some blocks' counts
            m.close()
    if shape == (129, 257):
        assert 2 * 128 * 257 > 16 * cp_tile()   # several compaction tiles


def test_slots_on_and_just_past_a_tile_edge(gm):
    """The triangle pass takes kCpTile slots per block: windows of exactly one tile, one tile and two slots, two tiles."""
    tile = cp_tile()
    assert tile == 4096
    rng = np.random.default_rng(17)
    with gm.GeometricMapping() as c:
        for n, ns, flags in ((9, 256, 0), (4, 683, 0), (9, 513, NO_WRAP), (9, 257, 0)):
            wrapped, NKq, quads = mn.grid(n, ns, flags)
            assert 2 * quads in (tile, tile + 2, 2 * tile, tile + 16)
            for fill in (1.0, 0.5):
                raw = random_raw(rng, n, ns, fill)
                m, p = make(c, raw)
                info, v, tri = check(m, p, raw, flags=flags, max_step=0.2)
                assert info["quads"] == quads and (fill < 1.0 or info["quads_two"] == quads)
                m.close()


# ---- 2. chunks ----

@pytest.mark.parametrize("shape", ((65, 257), (129, 65)))
def test_chunks_do_not_change_the_bytes(gm, shape):
    n, ns = shape
    raw = random_raw(np.random.default_rng(n), n, ns, 0.5)
    with gm.GeometricMapping() as c:
        whole, p = make(c, raw)
        f = frame_of(whole)
        for bs, bk in BLOCKS:
            kw = dict(block_stations=bs, block_sectors=bk, min_count=4, max_step=0.15)
            _, wv, wtri = check(whole, p, raw, frame=f, **kw)
            NK = -(-ns // bk)
            for blocks in (NK, 3 * NK, None):          # one block row, three rows, the default
                m, _ = make(c, raw, blocks)
                _, v, tri = check(m, p, raw, frame=f, cloud=False, **kw)
                assert v.tobytes() == wv.tobytes() and tri.tobytes() == wtri.tobytes()
                _, _, cut = check(m, p, raw, 3, n - 5, frame=f, cloud=False, **kw)   # a window that ends mid-block, chunked
                assert len(cut) > 0
                m.close()


def test_holes_straddling_the_chunk_boundary(gm):
    """Chunks of three block rows: the quad row between rows 2 and 3 has its corners in two vertex chunks.  Holes on both
    sides of that boundary and in the wrapped column give every class there."""
    n, ns = 8, 12
    raw = random_raw(np.random.default_rng(4), n, ns, 1.0)
    raw[2, [1, 5, 11]] = np.zeros((), RAW_CELL)      # above the boundary
    raw[3, [2, 5, 6, 0]] = np.zeros((), RAW_CELL)    # below it
    with gm.GeometricMapping() as c:
        whole, p = make(c, raw)
        m, _ = make(c, raw, 3 * ns)
        for flags in (0, OUTWARD, NO_WRAP):
            winfo, wv, wtri = check(whole, p, raw, flags=flags)
            info, v, tri = check(m, p, raw, flags=flags)
            assert info == winfo and v.tobytes() == wv.tobytes() and tri.tobytes() == wtri.tobytes()
        # the boundary row alone: quads of every class
        row = mn.triangles(2, ns, np.flatnonzero(raw["count"][2:4].reshape(-1) > 0), np.zeros(int((raw["count"][2:4] > 0).sum())))[1]
        assert row["quads_two"] > 0 and row["quads_one"] > 0 and row["quads_none"] > 0


# ---- 3. windows ----

def test_windows(gm):
    raw = random_raw(np.random.default_rng(3), 40, 33, 0.6)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        for kw in (dict(), dict(block_stations=7, block_sectors=5), dict(block_stations=2, block_sectors=3, max_step=0.1)):
            check(m, p, raw, 5, 20, **kw)                        # inside the map; 20 stations end mid-block at 7
            check(m, p, raw, 12, 28, **kw)                       # ends at n_stations
            info, v, tri = check(m, p, raw, 39, 1, **kw)         # n = 1: vertices, no triangles
            assert info["quads"] == 0 and len(tri) == 0
            info, v, tri = check(m, p, raw, 17, 0, **kw)         # n = 0: nothing
            assert info["quads"] == 0 and info["cloud"]["blocks"] == 0 and len(v) == 0 and len(tri) == 0
            check(m, p, raw, 40, 0, **kw)
        for s0, n in ((39, 2), (41, 0), (0, 41)):
            with pytest.raises(gm.GmError) as e:
                m.mesh(s0, n)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG


# ---- 4. capacity and errors ----

def test_capacity_and_errors(gm):
    raw = random_raw(np.random.default_rng(5), 20, 30, 0.7)
    p0 = wn.params(n_stations=20, n_sectors=30)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw, 4 * 30)          # five chunks
        winfo, wv, wtri = mn.mesh(raw, p0, 0, None, api.wall_cloud_directions(m.prm), frame=frame_of(m))
        nv_want, nt_want = len(wv), len(wtri)
        assert nv_want > 100 and nt_want > 100
        L, h = c._L, m._h()
        prm = _lib.WallMeshParams()
        L.gm_wall_mesh_default_params(C.byref(prm))
        info, nv, nt = _lib.WallMeshInfo(), C.c_uint64(99), C.c_uint64(99)

        def call(q, vbuf, vcap, tbuf, tcap, i=info, a=nv, b=nt):
            return L.gm_wall_map_mesh(h, 0, 20, q, C.byref(i) if i is not None else None, vbuf, vcap, tbuf, tcap,
                                      C.byref(a) if a is not None else None, C.byref(b) if b is not None else None)

        def counted():
            return (nv.value, nt.value, info.cloud.points, info.triangles, info.quads) == (nv_want, nt_want, nv_want, nt_want, 19 * 30)

        assert call(C.byref(prm), None, 0, None, 0) == _lib.GM_OK and counted()       # the count query
        assert info.struct_size == C.sizeof(_lib.WallMeshInfo) and info.wrapped == 1
        v = np.zeros(nv_want, WALL_CLOUD_POINT)
        t = np.zeros((nt_want, 3), np.uint32)
        vp, tp = v.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)), t.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle))
        nv.value = nt.value = 99
        assert call(C.byref(prm), vp, nv_want - 1, tp, nt_want) == _lib.GM_ERR_CAPACITY and counted()   # either side one short
        nv.value = nt.value = 99
        assert call(C.byref(prm), vp, nv_want, tp, nt_want - 1) == _lib.GM_ERR_CAPACITY and counted()
        assert call(C.byref(prm), vp, 0, tp, nt_want) == _lib.GM_ERR_CAPACITY
        assert call(C.byref(prm), vp, nv_want, tp, nt_want, a=None, b=None) == _lib.GM_OK
        assert v.tobytes() == wv.tobytes() and t.tobytes() == wtri.tobytes()
        v[:] = 0
        assert call(C.byref(prm), vp, nv_want, None, 0) == _lib.GM_OK and counted()   # the vertices alone
        assert v.tobytes() == wv.tobytes()
        t[:] = 0
        assert call(None, None, 0, tp, nt_want) == _lib.GM_OK and counted()           # NULL: the defaults; the triangles alone
        assert t.tobytes() == wtri.tobytes()
        bad = _lib.GM_ERR_INVALID_ARG
        assert call(C.byref(prm), None, 0, None, 0, i=None) == bad
        assert call(C.byref(prm), None, 5, None, 0) == bad                            # NULL with a capacity, either side
        assert call(C.byref(prm), None, 0, None, 5) == bad
        for k, val in (("flags", 4), ("flags", 1 << 31), ("max_step", -1.0), ("max_step", float("nan")), ("max_step", float("inf")),
                       ("struct_size", 8), ("reserved", 1)):
            q = _lib.WallMeshParams()
            L.gm_wall_mesh_default_params(C.byref(q))
            setattr(q, k, val)
            assert call(C.byref(q), None, 0, None, 0) == bad, (k, val)
        for k, val in (("block_stations", 0), ("block_sectors", 0), ("min_count", 0), ("exaggeration", -1.0), ("struct_size", 8)):
            q = _lib.WallMeshParams()
            L.gm_wall_mesh_default_params(C.byref(q))
            setattr(q.cloud, k, val)
            assert call(C.byref(q), None, 0, None, 0) == bad, (k, val)
        with pytest.raises(TypeError):
            m.mesh(blocks=3)


# ---- 5. non-interference ----

def test_mesh_leaves_the_map_the_cloud_and_the_regions_alone(gm):
    raw = random_raw(np.random.default_rng(9), 60, 45, 0.6)
    L = _lib.load()
    with gm.GeometricMapping() as c:
        live0 = L.gm_debug_live_buffers()
        m, p = make(c, raw)
        created = L.gm_debug_live_buffers()
        kw = dict(block_stations=3, block_sectors=4)
        cloud0 = m.cloud(**kw)
        reg0 = m.regions(labels=True, min_cells=2, threshold=0.05)
        assert L.gm_debug_live_buffers() > created
        before = L.gm_debug_live_buffers()
        check(m, p, raw, max_step=0.1, **kw)
        check(m, p, raw, flags=OUTWARD)
        assert L.gm_debug_live_buffers() > before          # the mesh's scratch is the map's, allocated on first use
        cloud1 = m.cloud(**kw)
        reg1 = m.regions(labels=True, min_cells=2, threshold=0.05)
        assert cloud1[0] == cloud0[0] and cloud1[1].tobytes() == cloud0[1].tobytes()
        assert reg1[0] == reg0[0] and reg1[1].tobytes() == reg0[1].tobytes() and np.array_equal(reg1[3], reg0[3])
        assert m.read_raw().tobytes() == raw.tobytes()
        m.close()
        assert L.gm_debug_live_buffers() == live0
        other, _ = make(c, raw)                             # a map that never meshes allocates none of it
        other.cloud(**kw)
        n_cloud = L.gm_debug_live_buffers()
        other.mesh(**kw)
        assert L.gm_debug_live_buffers() > n_cloud
        other.close()
        assert L.gm_debug_live_buffers() == live0


def test_mesh_beside_a_frame_in_flight(gm):
    rng = np.random.default_rng(8)
    raw = random_raw(rng, 65, 257, 0.5)
    xyz = np.ascontiguousarray(synth.tunnel_frame(300_000, seed=4), dtype=np.float32)
    keys = ("n_in", "n_cropped", "n_valid", "n_voxels", "status_flags")
    with gm.GeometricMapping(n_slots=2) as c:
        ref = c.process_frame(xyz)
        m, p = make(c, raw)
        kw = dict(block_stations=2, block_sectors=3, max_step=0.1)
        alone = m.mesh(**kw)
        c.submit_frame(0, xyz)
        got = [m.mesh(**kw) for _ in range(3)]
        res = c.wait_frame(0)
        check(m, p, raw, **kw)
        for info, v, tri in got:
            assert info == alone[0] and v.tobytes() == alone[1].tobytes() and tri.tobytes() == alone[2].tobytes()
        assert {k: res[k] for k in keys} == {k: ref[k] for k in keys}
        for k in ("eigenvalues", "eigenvectors", "center_axis", "scatter6"):
            assert res[k].tobytes() == ref[k].tobytes(), k


# ---- 6. end to end ----

def test_end_to_end_drive(gm):
    drive = synth.tunnel_drive(6, 80_000, seed=21, sigma=0.01)
    p = wn.params(n_stations=120, **drive["design"])
    anchor = (12.0, 0.0, 0.0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for cloud, pose in drive["frames"]:
            m.add_points(cloud, pose, outputs=False)
        kw = dict(block_stations=2, block_sectors=2, min_count=4, anchor=anchor)
        info, v, tri = m.mesh(max_step=0.05, **kw)
        cinfo, cv = m.cloud(**kw)
        raw = m.read_raw()
        check(m, p, raw, max_step=0.05, **kw)
    assert cinfo == info["cloud"] and cv.tobytes() == v.tobytes() and len(v) > 1000
    hinfo, htri = api.wall_mesh_triangulate(cinfo["blocks_stations"], cinfo["blocks_sectors"], v, 0, 0.05)
    assert htri.tobytes() == tri.tobytes() and len(tri) > 1000
    assert {k: hinfo[k] for k in mn.INFO_KEYS} == {k: info[k] for k in mn.INFO_KEYS}
    # the patches' 0.15 m steps are cut: no triangle joins a patch block to the wall around it
    assert info["cut_by_step"] > 0
    mean = v["mean"][tri.astype(np.int64)]
    assert np.all(np.abs(mean.max(axis=1) - mean.min(axis=1)) <= np.float32(0.05))
