"""gm_wall_alignment_check_objects and its kin without a GPU: the symbols, the struct layouts from plain C99, the host-only
gm_wall_alignment_object_window and _object_metrics against the twin (tests/wall_alignment_objects_np.py), the refusals
that need no device, and the ABI calls the binding's four methods make."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_objects_np as an  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_objects_np as on  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_alignment_check_objects", "gm_wall_alignment_check_objects_rows", "gm_wall_alignment_object_window",
         "gm_wall_alignment_object_metrics")
N_STATIONS = [12, 17, 12, 9]   # bases 0, 12, 29, 41; total 50
ELEMENTS = [dict(kind="straight", n_stations=12), dict(kind="arc", n_stations=17, turn=(0.0, 1.0), curvature=0.01),
            dict(kind="clothoid", n_stations=12, turn=(0.0, 1.0), curvature=0.01, rate=-1e-4), dict(kind="straight", n_stations=9)]
PRM = dict(wn.DEFAULTS, n_sectors=10, station_length=0.25, t_min=3.5)


def rule():
    return api.WallAlignmentRule(ELEMENTS, **{k: v for k, v in PRM.items() if k != "n_stations"})


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {"gm_wall_alignment_objects_info": _lib.WallAlignmentObjectsInfo,
              "struct gm_wall_alignment_object_metrics": _lib.WallAlignmentObjectMetrics}
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
    assert C.sizeof(_lib.WallAlignmentObjectsInfo) == 136 and C.sizeof(_lib.WallAlignmentObjectMetrics) == 112
    # the shared heads, at the same offsets
    for head, whole in ((_lib.WallObjectsInfo, _lib.WallAlignmentObjectsInfo), (_lib.WallObjectMetrics, _lib.WallAlignmentObjectMetrics)):
        for f, _t in head._fields_:
            assert getattr(head, f).offset == getattr(whole, f).offset, f
        assert getattr(whole, whole._fields_[len(head._fields_)][0]).offset == C.sizeof(head)


def plan_of(element, side_element, side_anchor):
    return dict(element=element, side_element=list(side_element), side_anchor=list(side_anchor))


WINDOW_CASES = [
    ("an anchor before 0", plan_of(0, [0, 1], [-40, -52]), dict(half_window_stations=8)),
    ("an anchor before 0 that still reaches in", plan_of(0, [0, 1], [-3, -15]), dict(half_window_stations=8, block_stations=3)),
    ("an anchor past total", plan_of(3, [2, 3], [40, 28]), dict(half_window_stations=8)),
    ("an anchor past total that still reaches in", plan_of(3, [2, 3], [14, 2 + 12]), dict(half_window_stations=8, block_stations=3)),
    ("clipped at both ends", plan_of(1, [0, 1, 2, 3], [20, 8, -9, -21]), dict(half_window_stations=200, block_stations=4)),
    ("bs does not divide base 12 + 17", plan_of(2, [1, 2], [19, 2]), dict(half_window_stations=3, block_stations=5, block_sectors=3)),
    ("bs does not divide base 12", plan_of(1, [1], [1]), dict(half_window_stations=2, block_stations=7)),
    ("one side, the sensor behind the element", plan_of(2, [2], [-1]), dict(half_window_stations=1, block_stations=2)),
]


@pytest.mark.parametrize("name,plan,prm", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_object_window_equals_twin(name, plan, prm):
    got = rule().object_window(plan, **prm)
    want = an.window(N_STATIONS, PRM["n_sectors"], plan, dict(on.DEFAULTS, **prm))
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    assert got["side_rows"] == [0] * len(plan["side_element"]) and all(got[c] == 0 for c in on.CLASSES)
    assert set(got) == set(an.INFO_KEYS)


def test_window_cases_cover_what_they_name():
    w = {c[0]: an.window(N_STATIONS, 10, c[1], dict(on.DEFAULTS, **c[2])) for c in WINDOW_CASES}
    assert w["an anchor before 0"]["blocks_stations"] == 0 and w["an anchor before 0"]["anchor_global"] < 0
    assert w["an anchor past total"]["blocks_stations"] == 0 and w["an anchor past total"]["anchor_global"] > 50
    assert (w["clipped at both ends"]["station0"], w["clipped at both ends"]["n_stations"]) == (0, 50)
    b = w["bs does not divide base 12 + 17"]
    assert b["side_first"] == [12, 29] and b["station0"] % 5 == 0 and b["station0"] < 29 < b["station0"] + b["n_stations"]
    assert w["an anchor before 0 that still reaches in"]["station0"] == 0
    t = w["an anchor past total that still reaches in"]
    assert t["station0"] + t["n_stations"] == 50   # the ragged last block row is clipped to total


def _metrics_equal(got, want):
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), (k, got[k], v)
    assert set(got) == set(want)


def test_object_metrics_equal_twin():
    r = rule()
    rng = np.random.default_rng(11)
    for st_min, st_max in ((0, 0), (10, 13), (11, 12), (28, 29), (5, 45), (41, 49), (49, 49)):
        o = np.zeros((), on.OBJECT)
        o["points"], o["sum_delta"], o["peak"] = 9, int(rng.integers(-2 ** 40, 2 ** 40)), int(rng.integers(-2 ** 30, 2 ** 30))
        o["sum_x"], o["sum_y"], o["sum_z"] = (int(x) for x in rng.integers(-2 ** 40, 2 ** 40, 3))
        o["station_min"], o["station_max"] = st_min, st_max
        o["sector_min"], o["sector_max"], o["sector_min_turned"], o["sector_max_turned"] = 0, 9, 2, 6
        o["box_min"], o["box_max"] = (-1.0, -2.0, -3.0), (1.5, 2.5, 3.5)
        got = r.object_metrics(o)
        _metrics_equal(got, an.metrics(PRM, N_STATIONS, o))
        assert got["chainage_from"] == 3.5 + st_min * 0.25 and got["chainage_to"] == 3.5 + (st_max + 1.0) * 0.25
    assert (got["element_from"], got["station_from"], got["element_to"], got["station_to"]) == (3, 8, 3, 8)
    o["station_min"], o["station_max"] = 11, 29
    got = r.object_metrics(o)
    assert (got["element_from"], got["station_from"], got["element_to"], got["station_to"]) == (0, 11, 2, 0)
    # refusals: past total, station_min > station_max, points 0
    for lo, hi, pts in ((49, 50, 9), (13, 12, 9), (3, 4, 0)):
        o["station_min"], o["station_max"], o["points"] = lo, hi, pts
        with pytest.raises(_lib.GmError) as e:
            r.object_metrics(o)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG


def _window_status(r, plan, **prm):
    try:
        r.object_window(plan, **prm)
    except _lib.GmError as e:
        return e.status
    return _lib.GM_OK


def test_refusals_without_a_device():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    info, got = _lib.WallAlignmentObjectsInfo(), C.c_uint32(7)
    ok = api.WallMap.object_params()
    plan = api._alignment_plan_struct(plan_of(0, [0], [0]))
    assert L.gm_wall_alignment_check_objects(None, 0, C.byref(ok), C.byref(info), None, 0, C.byref(got), None, 0) == bad
    assert L.gm_wall_alignment_check_objects_rows(None, None, 0, C.byref(plan), C.byref(ok), C.byref(info), None, 0, C.byref(got), None) == bad
    r = rule()
    assert _window_status(r, plan_of(0, [0], [0])) == _lib.GM_OK
    # the plan: no sides, too many, not consecutive, not ascending, past the alignment, an element that is not a side
    for p in (plan_of(0, [], []), plan_of(0, [0, 1, 2, 3, 3], [0] * 5), plan_of(0, [0, 2], [0, 0]), plan_of(1, [1, 0], [0, 0]),
              plan_of(3, [3, 4], [0, 0]), plan_of(2, [0, 1], [0, 0]), plan_of(0, [1, 2], [0, 0])):
        assert _window_status(r, p) == bad, p
    wrong = api._alignment_plan_struct(plan_of(0, [0], [0]))
    wrong.struct_size -= 8
    assert L.gm_wall_alignment_object_window(*r._head(), C.byref(wrong), C.byref(ok), C.byref(info)) == bad
    assert L.gm_wall_alignment_object_window(*r._head(), None, C.byref(ok), C.byref(info)) == bad
    assert L.gm_wall_alignment_object_window(*r._head(), C.byref(plan), C.byref(ok), None) == bad
    # the parameters; a window above GM_WALL_OBJECT_MAX_BLOCKS blocks cannot be reached with 50 stations
    assert _window_status(r, plan_of(0, [0], [0]), connectivity=5) == bad
    assert _window_status(r, plan_of(0, [0], [0]), block_stations=0) == bad
    # a refused alignment
    e = api.WallAlignmentRule([dict(kind="arc", n_stations=4, curvature=-1.0, turn=(0.0, 1.0))], n_sectors=10)
    assert _window_status(e, plan_of(0, [0], [0])) == bad


def test_the_size_rule_refuses_with_unsupported():
    """256 elements of 2^23 stations x 2 sectors: total = 2^31 fits, ceil(total / bs) NK = 2^32 does not with bs = bk = 1;
    with bs = 2 or bk = 2 it does."""
    els = [dict(kind="straight", n_stations=1 << 23)] * 256
    r = api.WallAlignmentRule(els, n_sectors=2, station_length=0.01)
    assert r.check() == _lib.GM_OK
    assert _window_status(r, plan_of(0, [0], [0])) == _lib.GM_ERR_UNSUPPORTED
    assert _window_status(r, plan_of(0, [0], [0]), block_sectors=2) == _lib.GM_OK
    assert _window_status(r, plan_of(255, [254, 255], [0, 0]), block_stations=2) == _lib.GM_OK
    assert r.object_window(plan_of(255, [255], [5]), block_stations=2)["anchor_global"] == 255 * (1 << 23) + 5


class Recorder:
    """Stands in for libgm_hip.so: logs (name, argument digest), scripts the counts, returns GM_OK."""

    def __init__(self, counts):
        self.log, self.counts = [], counts

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args):
            self.log.append((name, tuple(None if a is None else (int(a) if isinstance(a, (int, np.integer)) else "ptr") for a in args)))
            if name in ("gm_create", "gm_wall_alignment_create"):
                args[-1]._obj.value = 0x1000 + len(self.log)
            if name in self.counts:
                at, n = self.counts[name]
                args[at]._obj.value = n
            return _lib.GM_OK
        return call


@pytest.mark.parametrize("cap,rows,n_calls", [(0, False, 1), (3, False, 2), (0, True, 2), (3, True, 2)])
def test_the_binding_makes_a_count_query_then_the_sized_call(monkeypatch, cap, rows, n_calls):
    rec = Recorder({"gm_wall_alignment_get_check": (-1, 2), "gm_wall_alignment_check_objects": (-3, cap),
                    "gm_wall_alignment_check_objects_rows": (-2, cap)})
    monkeypatch.setattr(_lib, "_lib", rec)
    ctx = api.GeometricMapping(boxFilterBound=5.0)
    al = ctx.wall_alignment(ELEMENTS[:2], n_sectors=8)
    del rec.log[:]
    info, obj, metrics, of_row = al.check_objects(1, rows=rows, min_points=2)
    names = [c[0] for c in rec.log if not c[0].endswith("_default_params")]   # (every **params starts from the defaults)
    assert names == (["gm_wall_alignment_get_check"] if rows else []) + ["gm_wall_alignment_check_objects"] * n_calls + \
        ["gm_wall_alignment_object_metrics"] * cap
    calls = [c[1] for c in rec.log if c[0] == "gm_wall_alignment_check_objects"]
    assert calls[0][4:6] == (None, 0) and calls[0][7:] == (None, 0)           # the query: no records, no rows
    if n_calls == 2:
        assert calls[1][4:6] == ("ptr", cap) and calls[1][7:] == (("ptr", 2) if rows else (None, 0))
    assert len(obj) == len(metrics) == cap and (of_row is None) == (not rows) and (rows is False or len(of_row) == 2)
    assert set(info) == set(an.INFO_KEYS)
    del rec.log[:]
    info, obj, metrics, of_row = al.objects_of_rows(np.zeros(3, api.WALL_CHECK_POINT), plan_of(1, [0, 1], [4, 0]))
    assert [c[0] for c in rec.log if not c[0].endswith("_default_params")] == ["gm_wall_alignment_check_objects_rows"] * 2 + ["gm_wall_alignment_object_metrics"] * cap
    assert len(of_row) == 3 and len(obj) == cap
    ctx.close()
