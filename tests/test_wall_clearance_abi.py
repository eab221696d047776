"""gm_wall_map_clearance without a GPU: the symbols, the struct layouts from plain C99, the defaults, every refusal
(gm_wall_clearance_check_params states what the map call refuses, without a map), the host-only polygon helper and the
runs against the twin (tests/wall_clearance_np.py), and the twin's own arithmetic: the classes add up and the inputs of
the GPU tests reach every class."""
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
import wall_clearance_np as gn  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_clearance_default_params", "gm_wall_clearance_check_params", "gm_wall_map_clearance",
         "gm_wall_gauge_from_polygon", "gm_wall_clearance_runs")
BAD, OK, CAP = _lib.GM_ERR_INVALID_ARG, _lib.GM_OK, _lib.GM_ERR_CAPACITY
i32p, u8p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)

BOX = np.array([(-1.4, -1.1), (1.4, -1.1), (1.4, 1.3), (-1.4, 1.3)])                     # shifted off the axis below
SEVEN = np.array([(1.6 * math.cos(a) * (1 + 0.2 * (i % 3)), 1.6 * math.sin(a) * (1 + 0.2 * (i % 3)))
                  for i, a in enumerate(np.arange(7) * 2 * math.pi / 7 + 0.3)])
HORSESHOE = np.array([(-1.5, -1.2), (1.5, -1.2), (1.5, 0.4), (1.06, 1.46), (0.0, 1.9), (-1.06, 1.46), (-1.5, 0.4)])
POLYGONS = (("box", BOX, (0.3, -0.2)), ("seven", SEVEN, (0.0, 0.0)), ("horseshoe", HORSESHOE, (-0.1, 0.25)))


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_clearance_params": _lib.WallClearanceParams,
        "gm_wall_clearance_station": _lib.WallClearanceStation,
        "gm_wall_clearance_cell": _lib.WallClearanceCell,
        "gm_wall_clearance_info": _lib.WallClearanceInfo,
        "gm_wall_clearance_run": _lib.WallClearanceRun,
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
    assert C.sizeof(_lib.WallClearanceStation) == 32 == api.WALL_CLEARANCE_STATION.itemsize and gn.STATION == api.WALL_CLEARANCE_STATION
    assert C.sizeof(_lib.WallClearanceCell) == 16 == api.WALL_CLEARANCE_CELL.itemsize and gn.CELL == api.WALL_CLEARANCE_CELL
    assert C.sizeof(_lib.WallClearanceRun) == 72 == api.WALL_CLEARANCE_RUN.itemsize and gn.RUN == api.WALL_CLEARANCE_RUN
    for ct, dt in ((_lib.WallClearanceStation, api.WALL_CLEARANCE_STATION), (_lib.WallClearanceCell, api.WALL_CLEARANCE_CELL),
                   (_lib.WallClearanceRun, api.WALL_CLEARANCE_RUN)):
        assert [dt.fields[f][1] for f, _t in ct._fields_] == [getattr(ct, f).offset for f, _t in ct._fields_]


def test_defaults():
    L = _lib.load()
    p = _lib.WallClearanceParams()
    L.gm_wall_clearance_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallClearanceParams) == 24 and p.reserved == 0
    assert (p.reference, p.min_count, p.margin) == (_lib.GM_WALL_CLEAR_MIN, 8, 0.10)
    for k, v in gn.DEFAULTS.items():
        assert getattr(p, k) == v
    L.gm_wall_clearance_default_params(None)   # a NULL is ignored
    q = api.WallMap.clearance_params(reference=_lib.GM_WALL_CLEAR_MEAN, margin=0.05)
    assert (q.reference, q.min_count, q.margin) == (1, 8, 0.05)
    with pytest.raises(TypeError):
        api.WallMap.clearance_params(struct_size=8)
    with pytest.raises(TypeError):
        api.WallMap.clearance_params(threshold=0.1)


def _check(p, c, g, n_gauges, sg, n):
    L = _lib.load()
    return L.gm_wall_clearance_check_params(C.byref(p) if p is not None else None, C.byref(c) if c is not None else None,
                                            g.ctypes.data_as(i32p) if g is not None else None, n_gauges,
                                            sg.ctypes.data_as(u8p) if sg is not None else None, n)


def test_every_refusal_of_the_call_without_a_device():
    L = _lib.load()
    info, got = _lib.WallClearanceInfo(), C.c_uint64(7)
    g = np.full((3, 90), 1 << 20, np.int32)
    assert L.gm_wall_map_clearance(None, 0, 0, g.ctypes.data_as(i32p), 1, None, None, C.byref(info), None, 0, None, 0, C.byref(got)) == BAD
    p, c = api.WallMap.params(), api.WallMap.clearance_params()
    sg = np.array([0, 2, 1, 2], np.uint8)
    assert _check(p, c, g, 3, sg, 4) == OK
    assert _check(p, None, g, 3, None, 4) == OK                       # NULL: the defaults; NULL: table 0 everywhere
    assert gn.params_ok(wn.params(), g, sg, 4)
    assert _check(None, c, g, 3, sg, 4) == BAD and _check(p, c, None, 3, sg, 4) == BAD
    for ng in (0, 257):
        assert _check(p, c, np.zeros((max(ng, 1), 90), np.int32), ng, None, 0) == BAD
    assert _check(p, c, np.zeros((256, 90), np.int32), 256, None, 0) == OK    # all sectors not gauged is a table
    neg = g.copy()
    neg[2, 89] = -1
    assert _check(p, c, neg, 3, None, 4) == BAD and _check(p, c, neg, 2, None, 4) == OK and not gn.params_ok(wn.params(), neg)
    assert _check(p, c, g, 2, sg, 4) == BAD and _check(p, c, g, 2, sg, 1) == OK    # an entry >= n_gauges, inside the window only
    assert not gn.params_ok(wn.params(), g[:2], sg, 4)
    for k, v in (("struct_size", 8), ("reference", 2), ("min_count", 0), ("margin", -1e-9), ("margin", 8.0000001),
                 ("margin", float("nan"))):
        q = api.WallMap.clearance_params()
        setattr(q, k, v)
        assert _check(p, q, g, 3, sg, 4) == BAD, (k, v)
    for m in (0.0, 8.0):
        assert _check(p, api.WallMap.clearance_params(margin=m), g, 3, sg, 4) == OK
    # R_q > 2^32: a radius above 4096 m
    assert _check(api.WallMap.params(radius=4096.0), c, g, 3, sg, 4) == OK
    for r in (4096.000001, float("inf"), 0.0):
        assert _check(api.WallMap.params(radius=r), c, g, 3, sg, 4) == BAD, r
    assert not gn.params_ok(wn.params(radius=4096.000001), g)
    q = api.WallMap.params()
    q.struct_size -= 8
    assert _check(q, c, g, 3, sg, 4) == BAD
    for ns in (0, 4097):
        assert _check(api.WallMap.params(n_sectors=ns), c, np.zeros((1, 4097), np.int32), 1, None, 0) == BAD


def _polygon_status(p, uv, n, off, out, cap, got):
    return _lib.load().gm_wall_gauge_from_polygon(C.byref(p) if p is not None else None, uv.ctypes.data_as(dp) if uv is not None else None,
                                                  n, off.ctypes.data_as(dp) if off is not None else None,
                                                  out.ctypes.data_as(i32p) if out is not None else None, cap, C.byref(got))


def test_polygon_refusals():
    p = api.WallMap.params(n_sectors=8)
    out, got = np.full(8, 7, np.int32), C.c_uint32(9)
    sq = np.array([(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)])
    zero = np.zeros(2)
    assert _polygon_status(p, sq, 4, zero, out, 8, got) == OK and got.value == 8
    assert _polygon_status(p, sq, 4, None, out, 8, got) == OK                      # NULL offset: no shift
    assert _polygon_status(p, sq[::-1].copy(), 4, zero, out, 8, got) == OK         # either orientation
    out[:] = 7
    assert _polygon_status(p, sq, 4, zero, out, 7, got) == CAP and got.value == 8 and np.all(out == 7)
    assert _polygon_status(p, sq, 4, zero, None, 0, got) == CAP and got.value == 8  # the count query
    assert _polygon_status(None, sq, 4, zero, out, 8, got) == BAD and _polygon_status(p, None, 4, zero, out, 8, got) == BAD
    assert _polygon_status(p, sq, 4, zero, None, 8, got) == BAD
    assert _polygon_status(p, sq, 2, zero, out, 8, got) == BAD
    many = np.stack([np.cos(np.arange(4097) * 2 * np.pi / 4097), np.sin(np.arange(4097) * 2 * np.pi / 4097)], axis=1).copy()
    assert _polygon_status(p, many, 4097, zero, out, 8, got) == BAD and _polygon_status(p, many, 4096, zero, out, 8, got) == OK
    bad = {
        "axis outside": (sq, np.array([2.5, 0.0])),
        "axis on an edge": (sq, np.array([1.0, 0.0])),
        "axis on a vertex": (sq, np.array([1.0, 1.0])),
        "bow tie": (np.array([(-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0)]), zero),
        "repeated vertex": (np.array([(-1.0, -1.0), (1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)]), zero),
        "fold back": (np.array([(-1.0, -1.0), (1.0, -1.0), (0.0, -1.0), (1.0, 1.0), (-1.0, 1.0)]), zero),
        "touching": (np.array([(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (0.0, -1.0), (-1.0, 1.0)]), zero),
        "not finite": (np.array([(-1.0, -1.0), (1.0, -1.0), (float("nan"), 1.0), (-1.0, 1.0)]), zero),
        "offset not finite": (sq, np.array([float("inf"), 0.0])),
        "too large": (sq * 2048.0, zero),
    }
    for name, (uv, off) in bad.items():
        uv = np.ascontiguousarray(uv)
        assert _polygon_status(p, uv, len(uv), off, out, 8, got) == BAD, name
        if "finite" not in name and name != "too large":
            assert not gn.polygon_ok(uv + off), name
    assert gn.gauge_from_polygon(sq * 2048.0, 8) is None
    for ns in (0, 4097):
        assert _polygon_status(api.WallMap.params(n_sectors=ns), sq, 4, zero, None, 0, got) == BAD
    with pytest.raises(_lib.GmError):
        api.wall_gauge_from_polygon(p, sq, offset=(2.5, 0.0))


def test_axis_centred_square():
    """Half-side 1, 8 sectors: every wedge of 45 degrees holds a corner or ends on the ray through one."""
    want = math.ceil(math.sqrt(2.0) * 2 ** 20)
    sq = np.array([(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)])
    g = api.wall_gauge_from_polygon(api.WallMap.params(n_sectors=8), sq)
    assert g.dtype == np.int32 and g.tolist() == [want] * 8
    assert gn.gauge_from_polygon(sq, 8).tolist() == [want] * 8
    assert api.wall_gauge_from_polygon(api.WallMap.params(n_sectors=1), sq).tolist() == [want]


@pytest.mark.parametrize("ns", (1, 2, 3, 8, 90, 4096))
@pytest.mark.parametrize("name,uv,off", POLYGONS, ids=[p[0] for p in POLYGONS])
def test_gauge_from_polygon_against_the_twin(name, uv, off, ns):
    """The fp64 error of a distance of a few metres is ~1e-15 m, far below 2^-20 m: only the ceil can flip, by one unit."""
    g = api.wall_gauge_from_polygon(api.WallMap.params(n_sectors=ns), uv, offset=off)
    w = gn.gauge_from_polygon(uv, ns, off)
    assert w is not None and g.shape == w.shape == (ns,) and g.dtype == np.int32
    assert np.abs(g.astype(np.int64) - w.astype(np.int64)).max() <= 1
    assert np.all(g > 0)
    P = uv + np.array(off)
    far = np.hypot(P[:, 0], P[:, 1]).max()
    assert g.max() == math.ceil(far * 2 ** 20) and (ns > 1 or g[0] == g.max())   # the farthest vertex lies in some wedge


@pytest.mark.parametrize("name,uv,off", POLYGONS, ids=[p[0] for p in POLYGONS])
def test_twin_polygon_rule_against_sampling(name, uv, off):
    """The rule is exact for the boundary inside the wedge; 800 000 boundary samples miss a wedge's maximum by at most
    their spacing (the perimeter over the sample count) and never exceed it."""
    P = uv + np.array(off)
    spacing = np.hypot(*(np.roll(P, -1, axis=0) - P).T).sum() / 800_000
    for ns in (8, 90):
        w = gn.gauge_from_polygon(uv, ns, off).astype(np.float64) * 2.0 ** -20
        s = gn.gauge_by_sampling(uv, ns, off)
        assert np.all(s <= w + 1e-12) and np.all(w - s <= 2 * spacing + 2.0 ** -20), (ns, (w - s).max())


def _stations(flags, seed=0):
    """Hand-made records: flagged stations get tight / infringed counts and a minimum below the margin."""
    rng = np.random.default_rng(seed)
    st = np.zeros(len(flags), gn.STATION)
    f = np.asarray(flags, bool)
    st["tight"] = np.where(f, rng.integers(0, 5, len(f)), 0)
    st["infringed"] = np.where(f & (st["tight"] == 0), 1, np.where(f, rng.integers(0, 3, len(f)), 0))
    st["usable"] = 60
    st["min_clearance"] = np.where(f, rng.integers(-3, 2, len(f)) * 1000, 200_000)   # ties among the flagged ones
    st["min_sector"] = rng.integers(0, 90, len(f))
    st["unsurveyed"] = 30
    return st


@pytest.mark.parametrize("gap", (0, 1, 5))
def test_runs_against_the_twin(gap):
    wall = wn.params(t_min=-3.7, station_length=0.3, n_sectors=90)
    p = api.WallMap.params(**wall)
    g = gap
    cases = {
        "none": [0] * 20,
        "all": [1] * 20,
        "ends": [1, 1] + [0] * (g + 3) + [1],
        "gap exactly": [0, 1] + [0] * g + [1, 0],
        "gap plus one": [0, 1] + [0] * (g + 1) + [1, 0],
        "chain": [1] + [0] * g + [1] + [0] * g + [1] + [0] * (g + 1) + [1],
        "one": [0, 0, 1, 0],
        "empty": [],
    }
    want_runs = {"none": 0, "all": 1, "ends": 2, "gap exactly": 1, "gap plus one": 2, "chain": 2, "one": 1, "empty": 0}
    for k, (name, flags) in enumerate(cases.items()):
        st = _stations(flags, seed=k)
        for s0 in (0, 1234):
            got = api.wall_clearance_runs(p, st, station0=s0, max_gap=gap)
            want = gn.runs(st, wall, s0, gap)
            assert got.dtype == api.WALL_CLEARANCE_RUN and got.tobytes() == want.tobytes(), (name, s0)
            assert len(got) == want_runs[name], name
            if len(got):
                assert got["station_from"][0] == s0 + flags.index(1)
                assert got["station_to"][-1] == s0 + len(flags) - 1 - flags[::-1].index(1)
                assert int(got["tight"].sum()) == int(st["tight"].sum()) and int(got["infringed"].sum()) == int(st["infringed"].sum())
                for r in got:
                    seg = st[r["station_from"] - s0:r["station_to"] - s0 + 1]
                    assert r["min_clearance"] == seg["min_clearance"].min()
                    assert r["min_station"] == r["station_from"] + int(seg["min_clearance"].argmin())
                    assert r["chainage_from"] == -3.7 + float(r["station_from"]) * 0.3


def test_runs_refusals_and_capacity():
    L = _lib.load()
    p = api.WallMap.params()
    st = _stations([1, 0, 0, 1])
    sp = st.ctypes.data_as(C.POINTER(_lib.WallClearanceStation))
    runs = np.zeros(2, api.WALL_CLEARANCE_RUN)
    rp = runs.ctypes.data_as(C.POINTER(_lib.WallClearanceRun))
    got = C.c_uint32(9)
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0, 0, None, 0, C.byref(got)) == OK and got.value == 2
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0, 0, rp, 1, C.byref(got)) == CAP and got.value == 2 and not runs.tobytes().strip(b"\0")
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0, 0, rp, 2, None) == OK and runs["station_to"].tolist() == [0, 3]
    assert L.gm_wall_clearance_runs(C.byref(p), None, 0, 0, 0, rp, 2, C.byref(got)) == OK and got.value == 0
    assert L.gm_wall_clearance_runs(None, sp, 4, 0, 0, rp, 2, C.byref(got)) == BAD
    assert L.gm_wall_clearance_runs(C.byref(p), None, 4, 0, 0, rp, 2, C.byref(got)) == BAD
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0, 0, None, 2, C.byref(got)) == BAD
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0xFFFFFFFD, 0, rp, 2, C.byref(got)) == BAD
    assert L.gm_wall_clearance_runs(C.byref(p), sp, 4, 0xFFFFFFFC, 0, rp, 2, C.byref(got)) == OK
    q = api.WallMap.params()
    q.struct_size -= 8
    assert L.gm_wall_clearance_runs(C.byref(q), sp, 4, 0, 0, rp, 2, C.byref(got)) == BAD


# ---- the twin's own arithmetic ----

SHAPES_N, SHAPES_NS, FILLS = (1, 2, 5, 65), (1, 2, 63, 64, 65, 257, 4096), (0.0, 0.03, 0.5, 1.0)


def shape_seed(n, ns):
    return 1000 * n + ns


def test_twin_classes_add_up_and_the_inputs_reach_every_class():
    """The inputs of the GPU shape sweep, on the CPU alone: the classes sum to the window, the list is the tight and the
    infringed cells in cell order, the station records add up to the totals, and at fill 0.5 every shape of 1000 cells or
    more holds all six classes with the margin of 0.05 m.  (Tight is about 3 % of the cells there; with a margin of 0
    nothing can be tight, with fewer cells a class may miss by chance.)"""
    for n in SHAPES_N:
        for ns in SHAPES_NS:
            rng = np.random.default_rng(shape_seed(n, ns))
            wall = wn.params(n_stations=n, n_sectors=ns, radius=2.5)
            for fill in FILLS:
                raw = gn.random_raw(rng, n, ns, fill)
                G = gn.random_gauges(rng, 1, ns, 2.5)
                for ref in (gn.MIN, gn.MEAN):
                    for margin in (0.0, 0.05):
                        info, st, cells = gn.clearance(raw, wall, 0, None, G, reference=ref, margin=margin)
                        assert sum(info[k] for k in gn.NAMES) == n * ns
                        assert len(cells) == info["tight"] + info["infringed"] == int(st["tight"].sum() + st["infringed"].sum())
                        assert np.all(np.diff(cells["cell"].astype(np.int64)) > 0) and np.all(cells["clearance"] < info["margin_q"])
                        assert int(st["usable"].sum()) == info["infringed"] + info["tight"] + info["clear"]
                        assert int(st["unsurveyed"].sum()) == info["empty"] + info["unusable"]
                        assert info["min_clearance"] == int(st["min_clearance"].min())
                        if margin == 0.0:
                            assert info["tight"] == 0
                        if fill == 0.0:
                            assert info["empty"] + info["ungauged"] == n * ns and info["min_cell"] == gn.U32_MAX
                        if fill == 0.5 and margin == 0.05 and n * ns >= 1000:
                            assert all(info[k] > 0 for k in gn.NAMES), (n, ns, ref, info)


def test_twin_modes_and_ties():
    """MIN is never more generous than MEAN on consistent cells; equal cells tie to sector 0 and the window's first cell."""
    rng = np.random.default_rng(4)
    wall = wn.params(n_stations=9, n_sectors=33)
    raw = gn.random_raw(rng, 9, 33, 1.0)
    G = np.full(33, gn.fixed(1.9), np.int32)
    _, smin, _ = gn.clearance(raw, wall, 0, None, G, reference=gn.MIN, min_count=1)
    _, smean, _ = gn.clearance(raw, wall, 0, None, G, reference=gn.MEAN, min_count=1)
    assert np.all(smin["min_clearance"] <= smean["min_clearance"] + 1)   # (the mean's division rounds toward zero)
    raw[:] = raw[0, 0]
    info, st, cells = gn.clearance(raw, wall, 2, 5, G, min_count=1, margin=8.0)
    assert np.all(st["min_sector"] == 0) and info["min_cell"] == 2 * 33 and len(cells) == 5 * 33
    assert cells["cell"][0] == 66 and len(set(cells["clearance"].tolist())) == 1
