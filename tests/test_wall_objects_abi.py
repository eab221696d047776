"""gm_wall_map_check_objects / gm_wall_check_objects without a GPU: the symbols, the struct layouts from plain C99, the
defaults, the host-only gm_wall_object_metrics against the twin (tests/wall_objects_np.py), the twin against a brute-force
pairwise-adjacency closure on random small grids, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_check_np as kn  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_objects_np as on  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_object_default_params", "gm_wall_map_check_objects", "gm_wall_check_objects", "gm_wall_object_metrics")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_object": _lib.WallObject,
        "gm_wall_object_params": _lib.WallObjectParams,
        "gm_wall_objects_info": _lib.WallObjectsInfo,
        "struct gm_wall_object_metrics": _lib.WallObjectMetrics,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    macros = ("GM_WALL_OBJECT_MAX_BLOCKS", "GM_WALL_OBJECT_TILE_ROWS", "GM_WALL_OBJECT_TILE_COLS")
    for e in macros:
        lines.append(f'printf("%u\\n", (unsigned){e});')
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
    want += [_lib.GM_WALL_OBJECT_MAX_BLOCKS, _lib.GM_WALL_OBJECT_TILE[0], _lib.GM_WALL_OBJECT_TILE[1]]
    assert out == want
    assert C.sizeof(_lib.WallObject) == 128 == api.WALL_OBJECT.itemsize == on.OBJECT.itemsize and on.OBJECT == api.WALL_OBJECT
    assert [api.WALL_OBJECT.fields[f][1] for f, _t in _lib.WallObject._fields_] == [getattr(_lib.WallObject, f).offset
                                                                                  for f, _t in _lib.WallObject._fields_]
    assert C.sizeof(_lib.WallObjectParams) == 32 and C.sizeof(_lib.WallObjectsInfo) == 64 and C.sizeof(_lib.WallObjectMetrics) == 96
    assert on.MAX_BLOCKS == _lib.GM_WALL_OBJECT_MAX_BLOCKS == 1 << 20


def test_defaults():
    L = _lib.load()
    p = _lib.WallObjectParams()
    L.gm_wall_object_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallObjectParams) and p.reserved == 0
    assert (p.block_stations, p.block_sectors, p.min_block_points, p.min_points, p.connectivity, p.half_window_stations) == (1, 1, 2, 8, 8, 128)
    for k, v in on.DEFAULTS.items():
        assert getattr(p, k) == v
    L.gm_wall_object_default_params(None)   # a NULL is ignored
    q = api.WallMap.object_params(connectivity=4, min_points=3)
    assert q.connectivity == 4 and q.min_points == 3 and q.block_stations == 1
    with pytest.raises(TypeError):
        api.WallMap.object_params(struct_size=8)


def _metrics_equal(got, want):
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), (k, got[k], v)
    assert set(got) == set(want)


def test_metrics_equal_twin():
    p = dict(wn.DEFAULTS, n_stations=300, n_sectors=90, station_length=0.3, t_min=-7.25)
    prm = api.WallMap.params(**p)
    rng = np.random.default_rng(5)
    rows = []
    # an object across sector 0, one in the middle of the ring, a negative one, a ring over every sector
    for cells, d in (([100 * 90 + k % 90 for k in range(85, 96)], 0.21), ([120 * 90 + k for k in range(30, 41)], 0.4),
                     ([140 * 90 + k for k in range(50, 60)] + [141 * 90 + 59], -0.33), ([160 * 90 + k for k in range(90)], 0.11)):
        cell = np.repeat(np.array(cells), 3)
        rows.append(on.make_rows(cell, (d * rng.uniform(0.5, 1.5, len(cell))).astype(np.float32), seed=len(rows)))
    rows = np.concatenate(rows)
    rows["index"] = rng.permutation(len(rows))
    info, obj, _ = on.objects(rows, 300, 90, 150)
    assert info["objects"] == 4 and obj["sign"].tolist() == [1, 1, -1, 1]
    seen = []
    for o in obj:
        got = api.object_metrics(prm, o)
        _metrics_equal(got, on.metrics(p, o))
        seen.append((got["angle_from_deg"], got["angle_to_deg"]))
        assert got["chainage_to"] - got["chainage_from"] == pytest.approx(0.3 * (int(o["station_max"]) - int(o["station_min"]) + 1))
        assert np.all(got["size"] >= 0) and np.all(np.abs(got["centroid"]) <= 5.0) and abs(got["peak_m"]) >= abs(got["mean_m"])
    assert seen == [(340.0, 24.0), (120.0, 164.0), (200.0, 240.0), (0.0, 360.0)]        # the first runs across 0
    # extreme sums and a single row
    o = np.zeros((), on.OBJECT)
    o["points"], o["sum_x"], o["sum_y"], o["sum_z"], o["sum_delta"], o["peak"] = 3, -(2 ** 62), 2 ** 62 + 12345, 7, -(2 ** 61) - 1, -(2 ** 31)
    o["box_min"], o["box_max"] = (-1e30, -0.0, 1.5), (1e30, 0.0, 1.5)
    _metrics_equal(api.object_metrics(prm, o), on.metrics(p, o))
    # refusals
    L = _lib.load()
    out = _lib.WallObjectMetrics()
    rec = np.zeros(1, api.WALL_OBJECT)
    rp = rec.ctypes.data_as(C.POINTER(_lib.WallObject))
    bad = _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_object_metrics(C.byref(prm), None, rp, C.byref(out)) == bad                      # points 0
    rec["points"] = 1
    assert L.gm_wall_object_metrics(C.byref(prm), None, rp, C.byref(out)) == _lib.GM_OK               # op may be NULL
    assert L.gm_wall_object_metrics(None, None, rp, C.byref(out)) == bad
    assert L.gm_wall_object_metrics(C.byref(prm), None, None, C.byref(out)) == bad
    assert L.gm_wall_object_metrics(C.byref(prm), None, rp, None) == bad
    op = api.WallMap.object_params()
    op.struct_size = 28
    assert L.gm_wall_object_metrics(C.byref(prm), C.byref(op), rp, C.byref(out)) == bad
    for f, v in (("sector_max", 90), ("sector_min", 1), ("sector_max_turned", 90), ("sector_min_turned", 1), ("station_min", 1)):
        r2 = rec.copy()
        r2[f] = v
        assert L.gm_wall_object_metrics(C.byref(prm), None, r2.ctypes.data_as(C.POINTER(_lib.WallObject)), C.byref(out)) == bad, f


def _closure(flagged, nJ, NK, conn8):
    """Components of a list of (Jl, K) blocks by the pairwise adjacency matrix and its transitive closure."""
    n = len(flagged)
    A = np.eye(n, dtype=bool)
    for a in range(n):
        for b in range(n):
            dj = abs(flagged[a][0] - flagged[b][0])
            dk = abs(flagged[a][1] - flagged[b][1])
            dk = min(dk, NK - dk)
            A[a, b] |= (dj + dk == 1) or (conn8 and dj == 1 and dk == 1) or (dj + dk == 0)
    while True:
        B = (A.astype(np.int64) @ A.astype(np.int64)) > 0
        if np.array_equal(B, A):
            break
        A = B
    return [frozenset(flagged[b] for b in np.flatnonzero(A[a])) for a in range(n)]


def test_twin_equals_pairwise_closure():
    rng = np.random.default_rng(2024)
    objects = components = 0
    for trial in range(300):
        n_stations, ns = int(rng.integers(1, 14)), int(rng.integers(1, 12))
        bs, bk = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        H = int(rng.integers(1, 8))
        anchor = int(rng.integers(-3, n_stations + 3))
        op = dict(block_stations=bs, block_sectors=bk, min_block_points=int(rng.integers(1, 4)), min_points=int(rng.integers(1, 7)),
                  connectivity=int(rng.choice([4, 8])), half_window_stations=H)
        n = int(rng.integers(0, 120))
        cell = rng.integers(-1, n_stations * ns + 1, n)
        delta = (rng.choice([-1.0, 1.0], n) * rng.choice([0.0, 0.1, 0.2, 0.4], n, p=[0.05, 0.35, 0.3, 0.3])).astype(np.float32)
        rows = on.make_rows(cell, delta, index=rng.permutation(n), seed=trial)
        info, obj, of_row = on.objects(rows, n_stations, ns, anchor, **op)
        J0, nJ, NK, _, _ = on.window(n_stations, ns, anchor, op)
        # the same classes and partition, restated row by row
        dq = kn.fix(rows["delta"])
        ok = (cell >= 0) & (cell < n_stations * ns) & (dq != 0)
        J, K = np.where(ok, cell, 0) // ns // bs, np.where(ok, cell, 0) % ns // bk
        live = ok & (J >= J0) & (J < J0 + nJ)
        assert info["rejected"] == int((~ok).sum()) and info["outside_window"] == int((ok & ~live).sum())
        expect = np.full(n, -1, np.int64)
        records = []
        for sign in (-1, 1):
            sel = live & (np.sign(dq) == sign)
            blocks = {}
            for i in np.flatnonzero(sel):
                blocks.setdefault((int(J[i] - J0), int(K[i])), []).append(int(i))
            flagged = sorted(b for b, idx in blocks.items() if len(idx) >= op["min_block_points"])
            comps = set(_closure(flagged, nJ, NK, op["connectivity"] == 8))
            components += len(comps)
            for comp in comps:
                idx = sorted(i for b in comp for i in blocks[b])
                if len(idx) >= op["min_points"]:
                    records.append((min((J0 + b[0]) * NK + b[1] for b in comp), sign, len(comp), idx))
        records.sort()
        assert info["objects"] == len(records) == len(obj)
        for pos, (label, sign, nblocks, idx) in enumerate(records):
            assert (obj[pos]["label"], obj[pos]["sign"], obj[pos]["blocks"], obj[pos]["points"]) == (label, sign, nblocks, len(idx))
            assert obj[pos]["sum_delta"] == int(dq[idx].sum()) and obj[pos]["peak"] == sign * int(np.abs(dq[idx]).max())
            expect[idx] = pos
        assert np.array_equal(of_row, expect)
        objects += len(records)
    assert objects > 150 and components > 600


def test_refusals_without_a_device():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    info, got = _lib.WallObjectsInfo(), C.c_uint32(7)
    ok = api.WallMap.object_params()
    assert L.gm_wall_map_check_objects(None, 0, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 0) == bad
    assert L.gm_wall_check_objects(None, None, 0, 0, C.byref(ok), C.byref(info), None, 0, C.byref(got), None) == bad
