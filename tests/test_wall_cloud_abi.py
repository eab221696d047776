"""gm_wall_map_cloud without a GPU: the symbols, the struct layouts from plain C99, the defaults, the refusals that
need no device, the host-only direction table against math.cos / math.sin, and the twin's own arithmetic
(tests/wall_cloud_np.py): merged blocks equal a map binned on the coarse grid, the classes add up, and the anchor makes
the positions independent of the chainage."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_cloud_np as cn  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_cloud_default_params", "gm_wall_cloud_directions", "gm_wall_map_cloud")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_cloud_params": _lib.WallCloudParams,
        "gm_wall_cloud_point": _lib.WallCloudPoint,
        "gm_wall_cloud_info": _lib.WallCloudInfo,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gm_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = []
    for _, ct in sorted(fields.items()):
        want.append(C.sizeof(ct))
        want += [getattr(ct, f).offset for f, _t in ct._fields_]
    assert out == want
    assert C.sizeof(_lib.WallCloudPoint) == 40 == api.WALL_CLOUD_POINT.itemsize and cn.POINT == api.WALL_CLOUD_POINT
    assert [api.WALL_CLOUD_POINT.fields[f][1] for f, _t in _lib.WallCloudPoint._fields_] == [
        getattr(_lib.WallCloudPoint, f).offset for f, _t in _lib.WallCloudPoint._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]


def test_defaults():
    L = _lib.load()
    p = _lib.WallCloudParams()
    L.gm_wall_cloud_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallCloudParams) and p.reserved == 0
    assert (p.block_stations, p.block_sectors, p.min_count, p.exaggeration, list(p.anchor)) == (1, 1, 1, 1.0, [0.0, 0.0, 0.0])
    for k, v in cn.DEFAULTS.items():
        assert (tuple(getattr(p, k)) if k == "anchor" else getattr(p, k)) == v
    L.gm_wall_cloud_default_params(None)   # a NULL is ignored
    q = api.WallMap.cloud_params(block_sectors=4, anchor=(5000, 0, 1))
    assert q.block_sectors == 4 and list(q.anchor) == [5000.0, 0.0, 1.0] and q.min_count == 1
    with pytest.raises(TypeError):
        api.WallMap.cloud_params(struct_size=8)


def test_null_and_bad_struct_size_are_refused_without_a_device():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    info, got = _lib.WallCloudInfo(), C.c_uint64(7)
    assert L.gm_wall_map_cloud(None, 0, 0, None, C.byref(info), None, 0, C.byref(got)) == bad
    p, c = api.WallMap.params(), api.WallMap.cloud_params()
    buf = (C.c_double * 180)()
    n = C.c_uint32(7)
    assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf, 90, C.byref(n)) == _lib.GM_OK and n.value == 90
    assert L.gm_wall_cloud_directions(C.byref(p), None, buf, 90, None) == _lib.GM_OK   # NULL: the defaults
    assert L.gm_wall_cloud_directions(None, C.byref(c), buf, 90, C.byref(n)) == bad
    assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), None, 90, C.byref(n)) == bad
    c.struct_size = 8
    assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf, 90, C.byref(n)) == bad
    c = api.WallMap.cloud_params()
    c.block_sectors = 0
    assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf, 90, C.byref(n)) == bad
    c = api.WallMap.cloud_params()
    p.struct_size -= 8
    assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf, 90, C.byref(n)) == bad
    p = api.WallMap.params()
    for ns in (0, 4097):
        p.n_sectors = ns
        assert L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf, 90, C.byref(n)) == bad


def _ulp_apart(a, b):
    return abs(a - b) <= math.ulp(b)


@pytest.mark.parametrize("ns,bk", ((90, 1), (90, 7), (1, 1), (4096, 4096), (65, 64)))
def test_directions(ns, bk):
    L = _lib.load()
    p = api.WallMap.params(n_sectors=ns)
    tab = api.wall_cloud_directions(p, block_sectors=bk)
    NK = -(-ns // bk)
    assert tab.shape == (NK, 2) and tab.dtype == np.float64
    for K in range(NK):
        nk = min(bk, ns - K * bk)
        phi = (2.0 * math.pi) * (float(2 * K * bk + nk) / float(2 * ns))
        # libm's stated accuracy is the bound: 1 ulp
        assert _ulp_apart(tab[K, 0], math.cos(phi)) and _ulp_apart(tab[K, 1], math.sin(phi)), (K, tab[K], phi)
    twin = cn.directions(ns, bk)
    assert twin.shape == tab.shape and np.all(np.abs(twin - tab) <= np.spacing(np.abs(tab)))
    # a short capacity: GM_ERR_CAPACITY with the count, nothing written
    c = api.WallMap.cloud_params(block_sectors=bk)
    buf = np.full(2 * NK, 7.0)
    n = C.c_uint32(0)
    st = L.gm_wall_cloud_directions(C.byref(p), C.byref(c), buf.ctypes.data_as(C.POINTER(C.c_double)), NK - 1, C.byref(n))
    assert st == _lib.GM_ERR_CAPACITY and n.value == NK and np.all(buf == 7.0)
    # a block wider than the ring is one block
    wide = api.wall_cloud_directions(p, block_sectors=5000)
    assert wide.shape == (1, 2) and _ulp_apart(wide[0, 0], -1.0) and abs(wide[0, 1]) < 1e-15


# ---- the twin's own arithmetic ----

def _pairs(rng, n_cells, n_points):
    e = (rng.normal(0.0, 0.05, n_points)).astype(np.float32)
    return e, rng.integers(0, n_cells, n_points)


@pytest.mark.parametrize("shape,bs,bk", (((12, 30), 3, 5), ((64, 64), 64, 64), ((8, 9), 1, 3), ((10, 4), 5, 1)))
def test_twin_merge_equals_binning_on_the_coarse_grid(shape, bs, bk):
    """With bs, bk dividing the grid, merging the fine map's cells gives the raw cells of a map binned directly on the
    coarse grid from the same (cell, e) pairs."""
    n, ns = shape
    rng = np.random.default_rng(n * 100 + ns)
    e, cell = _pairs(rng, n * ns, 3000)
    cell[rng.random(len(cell)) < 0.1] = -1          # some points are not mapped
    fine = wn.cells_from(e, cell, n * ns).reshape(n, ns)
    j, k = cell // ns, cell % ns
    coarse_cell = np.where(cell >= 0, (j // bs) * (ns // bk) + k // bk, -1)
    coarse = wn.cells_from(e, coarse_cell, (n // bs) * (ns // bk)).reshape(n // bs, ns // bk)
    m = cn.merge_blocks(fine, bs, bk)
    for f in ("sum", "count", "min_key", "max_key"):
        assert np.array_equal(m[f], coarse[f]), f
    assert m["count"].dtype == np.uint64 and m["sum"].dtype == np.int64
    occupied = (fine["count"] > 0).reshape(n // bs, bs, ns // bk, bk).sum(axis=(1, 3))
    assert np.array_equal(m["cells"], occupied)


def test_twin_count_is_64_bits_wide():
    raw = np.zeros((2, 2), wn.RAW_CELL)
    raw["count"] = 0xFFFFFFFF
    raw["sum"] = -5
    m = cn.merge_blocks(raw, 2, 2)
    assert m.shape == (1, 1) and int(m["count"][0, 0]) == 4 * 0xFFFFFFFF and m["sum"][0, 0] == -20 and m["cells"][0, 0] == 4


def _random_raw(rng, n, ns, fill):
    raw = np.zeros((n, ns), wn.RAW_CELL)
    hit = rng.random((n, ns)) < fill
    cnt = rng.integers(1, 21, (n, ns))
    lo = rng.uniform(-0.2, 0.0, (n, ns)).astype(np.float32)
    hi = rng.uniform(0.0, 0.2, (n, ns)).astype(np.float32)
    raw["count"] = np.where(hit, cnt, 0)
    raw["sum"] = np.where(hit, np.rint(rng.uniform(-0.2, 0.2, (n, ns)) * cnt * 2.0 ** 20).astype(np.int64), 0)
    raw["min_key"] = np.where(hit, ~wn.ordered(lo), 0)
    raw["max_key"] = np.where(hit, wn.ordered(hi), 0)
    return raw


@pytest.mark.parametrize("stride", ((1, 1), (2, 3), (7, 5), (64, 64), (200, 1), (1, 5000)))
def test_twin_classes_add_up_and_blocks_ascend(stride):
    rng = np.random.default_rng(sum(stride))
    p = wn.params(n_stations=65, n_sectors=33)
    raw = _random_raw(rng, 65, 33, 0.3)
    for s0, n in ((0, None), (3, 40), (10, 0)):
        for mc in (1, 8):
            info, rec = cn.cloud(raw, p, s0, n, cn.directions(33, stride[1]), block_stations=stride[0], block_sectors=stride[1],
                                 min_count=mc)
            assert info["points"] + info["below_min_count"] + info["empty"] == info["blocks"] == info["blocks_stations"] * info["blocks_sectors"]
            assert len(rec) == info["points"] and np.all(np.diff(rec["block"].astype(np.int64)) > 0)
            assert np.all(rec["count"] >= mc) and np.all(rec["cells"] >= 1)
            win = raw[s0:] if n is None else raw[s0:s0 + n]
            if mc == 1:
                assert int(rec["count"].sum()) == int(win["count"].sum()) and int(rec["cells"].sum()) == int((win["count"] > 0).sum())
    # stride 1 is gm_wall_map_read's records of the non-empty cells, in cell order
    info, rec = cn.cloud(raw, p, 0, None, cn.directions(33, 1))
    count, mean, mn, mx = wn.records_from(raw.reshape(-1))
    keep = count > 0
    assert np.array_equal(rec["block"], np.flatnonzero(keep)) and np.array_equal(rec["count"], count[keep])
    for f, want in (("mean", mean), ("min", mn), ("max", mx)):
        assert rec[f].tobytes() == want[keep].tobytes()
    # the point sits on the design cylinder displaced by the mean: radius R + mean around the x axis, at the block's centre
    r = np.hypot(rec["y"].astype(np.float64), rec["z"].astype(np.float64))
    assert np.allclose(r, 2.0 + rec["mean"], atol=1e-6)
    assert np.array_equal(rec["x"], ((rec["block"] // 33) + 0.5).astype(np.float32) * np.float32(0.25))


def test_twin_anchor_makes_positions_independent_of_the_chainage():
    """The map's t_min and the anchor moved along the axis by the same 20 000 stations: bit-equal x, y, z (design at the
    origin along x; ds = 0.25, so every t_c is exact)."""
    rng = np.random.default_rng(5)
    raw = _random_raw(rng, 40, 90, 0.5)
    near = wn.params(n_stations=40, t_min=0.0, station_length=0.25)
    far = wn.params(n_stations=40, t_min=5000.0, station_length=0.25)
    for stride in ((1, 1), (7, 5)):
        tab = cn.directions(90, stride[1])
        kw = dict(block_stations=stride[0], block_sectors=stride[1], exaggeration=50.0)
        _, a = cn.cloud(raw, near, 0, None, tab, anchor=(0.0, 0.0, 0.0), **kw)
        _, b = cn.cloud(raw, far, 0, None, tab, anchor=(5000.0, 0.0, 0.0), **kw)
        assert len(a) > 0 and a.tobytes() == b.tobytes()
