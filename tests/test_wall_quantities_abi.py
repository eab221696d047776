"""gm_wall_map_quantities without a GPU: the symbols, the struct layouts from plain C99, the defaults, every refusal of
gm_wall_quantity_check_params one by one, and the host-only column, metrics and runs against the twin
(tests/wall_quantities_np.py) on hand-built inputs, with one exact analytic case."""
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
import wall_np as wn  # noqa: E402
import wall_quantities_np as qn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_quantity_default_params", "gm_wall_quantity_check_params", "gm_wall_quantity_column",
         "gm_wall_quantity_metrics", "gm_wall_quantity_runs", "gm_wall_map_quantities")
BAD, OK, CAP = _lib.GM_ERR_INVALID_ARG, _lib.GM_OK, _lib.GM_ERR_CAPACITY
SAT = 1 << 24
ONE = 1 << 20
# the class boundaries, shared with the GPU test: (name, sum, count, lo, hi, class) at min_count 8 and radius 2 m
BOUNDARY_COLUMNS = (
    ("toward zero", -7, 2, -3, -3, qn.UNUSABLE),             # count below min_count whatever the value
    ("v = lo - 1", 8 * 999, 8, 1000, 2000, qn.UNDER),
    ("v = lo", 8 * 1000, 8, 1000, 2000, qn.WITHIN),
    ("v = lo + 1", 8 * 1001, 8, 1000, 2000, qn.WITHIN),
    ("v = hi", 8 * 2000, 8, 1000, 2000, qn.WITHIN),
    ("v = hi + 1", 8 * 2001, 8, 1000, 2000, qn.OVER),
    ("count = min_count - 1", 7 * 5000, 7, 0, 0, qn.UNUSABLE),
    ("count = min_count", 8 * 5000, 8, 0, 0, qn.OVER),
    ("q saturates high", 8 * (SAT + 77), 8, 0, SAT, qn.WITHIN),
    ("q saturates low", -8 * (SAT + 77), 8, -SAT, 0, qn.WITHIN),
    ("negative sum", -8 * 300 - 5, 8, -200, 0, qn.UNDER),
    ("empty", 0, 0, 0, 0, qn.EMPTY),
)


def wall(**kw):
    d = wn.params(**kw)
    return api.WallMap.params(**d), d


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3
    assert api.WALL_QUANTITY_CLASSES == qn.CLASS_NAMES and api.WALL_QUANTITY_UNMEASURED == qn.NOT_MEASURED


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_quantity_params": _lib.WallQuantityParams,
        "gm_wall_quantity": _lib.WallQuantity,
        "gm_wall_quantities_info": _lib.WallQuantitiesInfo,
        "gm_wall_quantity_column_result": _lib.WallQuantityColumnResult,
        "struct gm_wall_quantity_metrics": _lib.WallQuantityMetrics,
        "gm_wall_quantity_run": _lib.WallQuantityRun,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    consts = ("GM_WALL_QUANTITY_MAX_PROFILES", "GM_WALL_QUANTITY_MAX_ZONES", "GM_WALL_QUANTITY_UNMEASURED",
              "GM_WALL_QUANTITY_CLASS_UNMEASURED", "GM_WALL_QUANTITY_CLASS_EMPTY", "GM_WALL_QUANTITY_CLASS_UNUSABLE",
              "GM_WALL_QUANTITY_CLASS_UNDER", "GM_WALL_QUANTITY_CLASS_OVER", "GM_WALL_QUANTITY_CLASS_WITHIN",
              "GM_WALL_QUANTITY_RUNS_ALL_ZONES")
    lines += [f'printf("%u\\n", (unsigned){c});' for c in consts]
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
    want += [qn.MAX_PROFILES, qn.MAX_ZONES, qn.NOT_MEASURED, qn.UNMEASURED, qn.EMPTY, qn.UNUSABLE, qn.UNDER, qn.OVER, qn.WITHIN,
             api.WALL_QUANTITY_RUNS_ALL_ZONES]
    assert out == want
    assert C.sizeof(_lib.WallQuantityParams) == 16 and C.sizeof(_lib.WallQuantitiesInfo) == 96
    assert C.sizeof(_lib.WallQuantityColumnResult) == 40 and C.sizeof(_lib.WallQuantityMetrics) == 136
    assert C.sizeof(_lib.WallQuantity) == 88 == api.WALL_QUANTITY.itemsize and qn.QUANTITY == api.WALL_QUANTITY
    assert C.sizeof(_lib.WallQuantityRun) == 136 == api.WALL_QUANTITY_RUN.itemsize and qn.RUN == api.WALL_QUANTITY_RUN
    for ct, dt in ((_lib.WallQuantity, api.WALL_QUANTITY), (_lib.WallQuantityRun, api.WALL_QUANTITY_RUN)):
        assert [dt.fields[f][1] for f, _t in ct._fields_] == [getattr(ct, f).offset for f, _t in ct._fields_]
    assert tuple(k for k, _t in _lib.WallQuantitiesInfo._fields_[1:]) == qn.INFO_KEYS


def test_defaults():
    L = _lib.load()
    p = _lib.WallQuantityParams()
    L.gm_wall_quantity_default_params(C.byref(p))
    assert (p.struct_size, p.section_stations, p.min_count, p.reserved) == (16, 4, 8, 0)
    assert dict(section_stations=p.section_stations, min_count=p.min_count) == qn.DEFAULTS
    L.gm_wall_quantity_default_params(None)   # a NULL is ignored
    with pytest.raises(TypeError):
        api.WallMap.quantity_params(struct_size=8)
    with pytest.raises(TypeError):
        api.WallMap.quantity_params(threshold=0.1)


def test_every_refusal_of_check_params_one_by_one():
    ns, n = 6, 10
    p, d = wall(n_stations=16, n_sectors=ns, radius=2.0)
    lo, hi = np.full((2, ns), -1000, np.int32), np.full((2, ns), 1000, np.int32)
    prof = np.array([0, 1, 1], np.uint8)       # NS = 3 at S = 4
    zone = np.array([0, 1, 2, 2, 0xFF, 0], np.uint8)

    def status(prm=p, lo=lo, hi=hi, profile=prof, zone=zone, n_zones=3, params=None, n_profiles=None, n=n):
        return api.wall_quantity_check_params(prm, lo, hi, n, profile, zone, n_zones, params, n_profiles)

    def twin(radius=2.0, lo=lo, hi=hi, profile=prof, zone=zone, n_zones=3, n_profiles=2, **kw):
        return qn.params_ok(radius, ns, lo, hi, n_profiles, profile, n, zone, n_zones, **kw)

    assert status() == OK and twin()
    assert status(profile=None, zone=None, n_zones=1) == OK and status(params=api.WallMap.quantity_params()) == OK
    L = _lib.load()
    i32 = C.POINTER(C.c_int32)
    assert L.gm_wall_quantity_check_params(None, None, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32), 2, None, n, None, 1) == BAD
    assert L.gm_wall_quantity_check_params(C.byref(p), None, None, hi.ctypes.data_as(i32), 2, None, n, None, 1) == BAD
    assert L.gm_wall_quantity_check_params(C.byref(p), None, lo.ctypes.data_as(i32), None, 2, None, n, None, 1) == BAD
    for k, v in (("struct_size", 8), ("section_stations", 0), ("min_count", 0)):
        q = api.WallMap.quantity_params()
        setattr(q, k, v)
        assert status(params=q) == BAD, k
        if k != "struct_size":
            assert not twin(**{k: v}), k
    assert status(n_profiles=0) == BAD and not twin(n_profiles=0)
    big_lo, big_hi = np.full((257, ns), -5, np.int32), np.full((257, ns), 5, np.int32)
    assert status(lo=big_lo, hi=big_hi, profile=None) == BAD and not twin(lo=big_lo, hi=big_hi, profile=None, n_profiles=257)
    assert status(lo=big_lo[:256], hi=big_hi[:256], profile=None) == OK and twin(lo=big_lo[:256], hi=big_hi[:256], n_profiles=256)
    for which, value in (("lo", -(SAT + 1)), ("hi", SAT + 1)):
        t = dict(lo=lo.copy(), hi=hi.copy())
        t[which][1, 3] = value
        assert status(**t) == BAD and not twin(**t), which
        t[which][1, 3] = value - 1 if value > 0 else value + 1   # the limit itself is allowed
        assert status(**t) == OK and twin(**t), which
    t = dict(lo=lo.copy(), hi=hi.copy())
    t["lo"][0, 5] = 1001                                      # lo > hi
    assert status(**t) == BAD and not twin(**t)
    t["lo"][0, 5] = 1000                                      # lo == hi is a line
    assert status(**t) == OK and twin(**t)
    bad_prof = np.array([0, 1, 2], np.uint8)                  # a profile index out of range, in the last section
    assert status(profile=bad_prof) == BAD and not twin(profile=bad_prof)
    assert status(profile=bad_prof, n=8) == OK and twin(profile=bad_prof[:2])   # two sections: the third entry is not read
    assert status(n_zones=0) == BAD and status(n_zones=9) == BAD and not twin(n_zones=0) and not twin(n_zones=9)
    assert status(n_zones=8) == OK and twin(n_zones=8)
    for entry in (3, 0xFE):                                   # between n_zones and 0xFE
        z = zone.copy()
        z[2] = entry
        assert status(zone=z) == BAD and not twin(zone=z), entry
    far, _ = wall(n_stations=16, n_sectors=ns, radius=4096.0 + 2.0 ** -20)   # R_q = 2^32 + 1
    assert status(prm=far) == BAD and not twin(radius=4096.0 + 2.0 ** -20)
    edge, _ = wall(n_stations=16, n_sectors=ns, radius=4096.0)
    assert status(prm=edge) == OK and twin(radius=4096.0)
    wide, _ = wall(n_stations=16, n_sectors=ns)
    wide.n_sectors = 4097
    assert status(prm=wide) == BAD


def _same_column(Rq, count, total, lo, hi, base=None, min_count=8, zone_entry=0):
    got = api.wall_quantity_column(Rq, count, total, lo, hi, base, min_count, zone_entry)
    want = qn.column(Rq, count, total, lo, hi, base, min_count, zone_entry)
    assert got == want, (got, want)
    return got


def test_column_against_the_twin_on_hand_built_inputs():
    Rq = 2 * ONE
    for name, total, count, lo, hi, cls in BOUNDARY_COLUMNS:
        c = _same_column(Rq, count, total, lo, hi)
        assert c["cls"] == cls, name
    assert _same_column(Rq, 2, -7, -10, 10, min_count=1)["v"] == -3                  # toward zero, not floor
    assert _same_column(Rq, 2, 7, -10, 10, min_count=1)["v"] == 3
    c = _same_column(Rq, 8, 8 * 999, 1000, 2000)
    assert c["over_line"] == -1 and c["under_area"] == (1 * (2 * Rq + 1999)) >> 20 and c["over_area"] == 0
    c = _same_column(Rq, 8, 8 * 2001, 1000, 2000)
    assert c["excess_area"] == (1 * (2 * Rq + 4001)) >> 20 and c["over_area"] == (1001 * (2 * Rq + 3001)) >> 20
    assert _same_column(Rq, 8, 8 * (SAT + 77), 0, SAT)["v"] == SAT and _same_column(Rq, 8, -8 * (SAT + 77), -SAT, 0)["v"] == -SAT
    # unmeasured: the value is kept, the areas are nobody's
    c = _same_column(Rq, 8, 8 * 5000, 0, 0, zone_entry=0xFF)
    assert c["cls"] == qn.UNMEASURED and c["v"] == 5000 and c["over_area"] == 0
    assert _same_column(Rq, 0, 0, 0, 0, zone_entry=0xFF)["cls"] == qn.UNMEASURED
    # a baseline: usable in both only, empty in both only
    assert _same_column(Rq, 8, 800, 0, 0, base=(7, 0))["cls"] == qn.UNUSABLE
    assert _same_column(Rq, 0, 0, 0, 0, base=(9, 90))["cls"] == qn.UNUSABLE
    assert _same_column(Rq, 0, 0, 0, 0, base=(0, 0))["cls"] == qn.EMPTY
    c = _same_column(Rq, 8, 8 * 100, 0, 0, base=(8, 8 * 400))                        # moved in by 300
    assert c["cls"] == qn.UNDER and c["v"] == -300 and c["under_area"] == (300 * (2 * Rq + 500)) >> 20
    c = _same_column(Rq, 8, 8 * 100, -300, -300, base=(8, 8 * 400))                  # exactly the required thickness
    assert c["cls"] == qn.WITHIN
    # a radius of 0.25 m, the baseline at -2^24 and lo = -2^24: L clamps at 0
    small = ONE // 4
    c = _same_column(small, 8, -8 * SAT, -SAT, 0, base=(8, -8 * SAT))
    assert c["cls"] == qn.WITHIN and c["v"] == 0 and c["over_line"] == SAT and c["over_area"] == 0   # x clamps too
    c = _same_column(small, 8, 8 * 1000, -SAT, 0, base=(8, -8 * SAT))
    x = small + 1000
    assert c["cls"] == qn.OVER and c["over_area"] == (x * x) >> 20 and c["excess_area"] == (x * x) >> 20
    L = _lib.load()
    out = _lib.WallQuantityColumnResult()
    for args in ((0, 8, 0, 0, 0, 0, 8, 0, 0, 0), (2 ** 32 + 1, 8, 0, 0, 0, 0, 8, 0, 0, 0), (Rq, 8, 0, 0, 0, 0, 0, 0, 0, 0),
                 (Rq, 8, 0, 0, 0, 0, 8, -SAT - 1, 0, 0), (Rq, 8, 0, 0, 0, 0, 8, 0, SAT + 1, 0), (Rq, 8, 0, 0, 0, 0, 8, 5, 4, 0)):
        assert L.gm_wall_quantity_column(*args, C.byref(out)) == BAD, args
    assert L.gm_wall_quantity_column(Rq, 8, 0, 0, 0, 0, 8, 0, 0, 0, None) == BAD


def _records(wall_dict, raw, lo, hi, **kw):
    return qn.quantities(raw, lo, hi, wall_dict["radius"], **kw)


def _same_metrics(p, d, r):
    got, want = api.wall_quantity_metrics(p, r), qn.metrics(d, r)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    return got


def test_the_exact_analytic_case():
    """Radius 2, 64 sectors, every column 0.125 m outside the design, lo = hi = 0."""
    ns = 64
    p, d = wall(n_stations=4, n_sectors=ns, radius=2.0, station_length=0.5, t_min=-1.0)
    raw = np.zeros((4, ns), wn.RAW_CELL)
    raw["count"], raw["sum"] = 16, 16 * 2 ** 17
    zero = np.zeros(ns, np.int32)
    info, rec, rows = _records(d, raw, zero, zero)
    assert rec.shape == (1, 1) and rec[0, 0]["over_area"] == 64 * (2 ** 19 + 2 ** 14) == rec[0, 0]["excess_area"]
    assert rec[0, 0]["over"] == 64 and np.all(rows == 2 ** 17) and rec[0, 0]["peak_over"] == 2 ** 17 and rec[0, 0]["peak_over_sector"] == 0
    m = _same_metrics(p, d, rec[0, 0])
    want = math.pi * (2.125 ** 2 - 2.0 ** 2)
    assert abs(m["over_area_m2"] - want) <= 1e-12 * want
    assert m["length"] == 2.0 and abs(m["over_volume_m3"] - 2.0 * want) <= 1e-12 * 2.0 * want and m["paid_area_m2"] == 0.0
    assert m["chainage_from"] == -1.0 and m["chainage_to"] == 1.0 and m["coverage"] == 1.0
    assert m["peak_over_m"] == 0.125 and m["peak_over_angle_deg"] == 360.0 / 128 and m["peak_under_angle_deg"] == 0.0


def _case(seed=5, n=11, ns=24, nz=3):
    rng = np.random.default_rng(seed)
    p, d = wall(n_stations=n, n_sectors=ns, radius=2.0, station_length=0.25, t_min=3.0)
    raw = np.zeros((n, ns), wn.RAW_CELL)
    raw["count"] = rng.integers(0, 12, (n, ns))
    raw["sum"] = raw["count"].astype(np.int64) * rng.integers(-200000, 200000, (n, ns))
    lo, hi = qn.random_tables(rng, 2, ns, 0.1)
    zone = rng.integers(0, nz, ns).astype(np.uint8)
    zone[3] = 0xFF
    info, rec, rows = _records(d, raw, lo, hi, zone=zone, n_zones=nz, section_profile=[0, 1, 0, 1], section_stations=3, min_count=4)
    return p, d, rec


def test_metrics_against_the_twin():
    p, d, rec = _case()
    assert rec.shape == (4, 3) and rec["under"].sum() > 0 and rec["over"].sum() > 0
    for r in rec.reshape(-1):
        m = _same_metrics(p, d, r)
        assert 0.0 <= m["coverage"] <= 1.0 and m["paid_area_m2"] >= 0.0
    none = np.zeros((), api.WALL_QUANTITY)
    none["stations"], none["peak_under_sector"], none["peak_over_sector"] = 1, qn.U32_MAX, qn.U32_MAX
    assert _same_metrics(p, d, none)["coverage"] == 0.0
    L = _lib.load()
    out = _lib.WallQuantityMetrics()
    rp = rec.ctypes.data_as(C.POINTER(_lib.WallQuantity))
    assert L.gm_wall_quantity_metrics(None, rp, C.byref(out)) == BAD and L.gm_wall_quantity_metrics(C.byref(p), None, C.byref(out)) == BAD
    assert L.gm_wall_quantity_metrics(C.byref(p), rp, None) == BAD
    none["stations"] = 0
    assert L.gm_wall_quantity_metrics(C.byref(p), none.reshape(1).ctypes.data_as(C.POINTER(_lib.WallQuantity)), C.byref(out)) == BAD


@pytest.mark.parametrize("run_sections", (1, 3, 9))
@pytest.mark.parametrize("all_zones", (False, True))
def test_runs_against_the_twin(run_sections, all_zones):
    p, d, rec = _case()
    got = api.wall_quantity_runs(p, rec, 3, run_sections, all_zones)
    want = qn.runs(d, rec, 3, run_sections, all_zones)
    assert got.dtype == api.WALL_QUANTITY_RUN and got.tobytes() == want.tobytes()
    NR = (4 + run_sections - 1) // run_sections
    assert len(got) == NR * (1 if all_zones else 3)
    assert got["sections"].reshape(NR, -1)[:, 0].tolist() == [min(run_sections, 4 - r * run_sections) for r in range(NR)]
    assert got["stations"].reshape(NR, -1)[:, 0].sum() == 11 and int(got["under"].sum()) == int(rec["under"].sum())
    assert int(got["peak_over"].max()) == int(rec["peak_over"].max())


def test_runs_refusals_and_conventions():
    L = _lib.load()
    p, d, rec = _case()
    rp, RP = rec.ctypes.data_as(C.POINTER(_lib.WallQuantity)), C.POINTER(_lib.WallQuantityRun)
    runs = np.zeros(8, api.WALL_QUANTITY_RUN)
    got = C.c_uint32(99)
    assert L.gm_wall_quantity_runs(C.byref(p), rp, 4, 3, 3, 0, None, 0, C.byref(got)) == OK and got.value == 6
    assert L.gm_wall_quantity_runs(C.byref(p), rp, 4, 3, 3, 0, runs.ctypes.data_as(RP), 5, C.byref(got)) == CAP and got.value == 6
    assert not runs.tobytes().strip(b"\0")
    assert L.gm_wall_quantity_runs(C.byref(p), rp, 4, 3, 3, 0, runs.ctypes.data_as(RP), 6, None) == OK
    assert L.gm_wall_quantity_runs(C.byref(p), None, 0, 3, 3, 0, runs.ctypes.data_as(RP), 8, C.byref(got)) == OK and got.value == 0
    for args in ((None, rp, 4, 3, 3, 0), (C.byref(p), None, 4, 3, 3, 0), (C.byref(p), rp, 4, 0, 3, 0), (C.byref(p), rp, 4, 9, 3, 0),
                 (C.byref(p), rp, 4, 3, 0, 0), (C.byref(p), rp, 4, 3, 3, 2)):
        assert L.gm_wall_quantity_runs(*args, runs.ctypes.data_as(RP), 8, C.byref(got)) == BAD, args[2:]
    assert L.gm_wall_quantity_runs(C.byref(p), rp, 4, 3, 3, 0, None, 8, C.byref(got)) == BAD


def test_the_call_refuses_a_null_map_without_a_device():
    L = _lib.load()
    info, got = _lib.WallQuantitiesInfo(), C.c_uint32(7)
    z = np.zeros(4, np.int32)
    zp = z.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.gm_wall_map_quantities(None, None, 0, 0, zp, zp, 1, None, None, 1, None, C.byref(info), None, 0, C.byref(got), None) == BAD
