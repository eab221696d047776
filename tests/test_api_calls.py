"""The ABI calls every WallMap, WallAlignmentRule and WallAlignment method makes, call for call, against a recording
stand-in for libgm_hip.so: tests/golden/api_calls.json holds the trace of each driven case.  Results cannot show a
method that started to run the device pipeline one time too many (the answers are the same and the launches double);
the trace does.  What it does not see: a digest holds None, the integer, the float or "ptr" per argument, so the length
of a buffer behind a pointer (a lost max(n, 1), say) is the GPU suite's to catch.  Needs neither the library nor a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_calls.json")

# where each counted call keeps its `got` out-parameter(s)
GOT = {
    "gm_wall_map_regions": (-2,), "gm_wall_map_cloud": (-1,), "gm_wall_map_mesh": (-2, -1), "gm_wall_map_clearance": (-1,),
    "gm_wall_map_sections": (-2,), "gm_wall_map_quantities": (-2,), "gm_wall_map_get_check": (-1,),
    "gm_wall_map_check_points": (10,), "gm_wall_map_get_align": (-1,), "gm_wall_map_align_points": (10,),
    "gm_wall_map_check_objects": (-3,), "gm_wall_check_objects": (-2,), "gm_wall_alignment_window": (-1,),
    "gm_wall_alignment_get_check": (-1,), "gm_wall_alignment_check_points": (10,), "gm_wall_alignment_get_align": (-1,),
    "gm_wall_alignment_align_points": (10,), "gm_wall_section_basis": (-1,),
}
# the calls that hand out a handle through their last argument
HANDLES = ("gm_create", "gm_wall_map_create", "gm_wall_map_create_arc", "gm_wall_map_create_clothoid",
           "gm_wall_alignment_create", "gm_wall_alignment_map")


def _digest(a):
    if a is None:
        return None
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, (float, np.floating)):
        return float(a)
    return "ptr"


class Recorder:
    """Every attribute is a function that logs (name, digest of the arguments), writes the scripted count of its name
    into the `got` out-parameter(s) and returns GM_OK.  A scripted list holds one count per call of the name, the query's
    first and the last one again for any further call; anything else is the count of every call."""

    def __init__(self):
        self.log, self.script = [], {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args):
            self.log.append([name, [_digest(a) for a in args]])
            if name in HANDLES:
                args[-1]._obj.value = 0x1000 + len(self.log)
            if name in self.script:
                count = self.script[name]
                if isinstance(count, list):
                    count = count.pop(0) if len(count) > 1 else count[0]
                for i, c in zip(GOT[name], count if isinstance(count, tuple) else (count,)):
                    args[i]._obj.value = c
            return _lib.GM_OK
        return call


ELEMENTS = [dict(kind="straight", n_stations=4), dict(kind="arc", n_stations=4, curvature=0.01)]
POSE = np.eye(4)[:3]
CLOUDS = {5: np.arange(15, dtype=np.float32).reshape(5, 3), 0: np.zeros((0, 3), np.float32)}
ROWS = np.zeros(3, api.WALL_CHECK_POINT)
GAUGE = np.zeros(8, np.int32)
TABLE = np.zeros(1, api.WALL_ALIGN_SCORE)


def _points(target, method, extra=(), script_name=None, tag="", **kw):
    """A *_points method on the 5-point and the empty cloud, with and without the per-point outputs, labels given once."""
    out = []
    for n in (5, 0):
        for outputs in (True, False):
            labels = np.zeros(n, np.uint8) if (n == 5 and outputs) else None
            script = {script_name: min(n, 3)} if script_name else {}
            out.append((target, method, f"{tag}n{n}_outputs{int(outputs)}",
                        lambda env, n=n, outputs=outputs, labels=labels: ((CLOUDS[n], POSE) + tuple(extra),
                                                                            dict(labels=labels, outputs=outputs, **kw)), script))
    return out


def _cases():
    """(class, method, variant, env -> (args, kwargs), script of counts per ABI name).  Counted calls get 0 and 3, so that
    both branches of every "skip the sized call" rule are taken; the align results take 1, the size of the table of an
    all-zero info, since their sized call is unconditional and a (2A + 1)(2B + 1) reshape follows."""
    c = []
    no = lambda env: ((), {})   # noqa: E731
    W, R, A = "WallMap", "WallAlignmentRule", "WallAlignment"
    # ---- WallMap ----
    c += [(W, "__init__", "straight", lambda env: ((env["ctx"],), dict(n_stations=4, n_sectors=8)), {}),
          (W, "__init__", "arc", lambda env: ((env["ctx"],), dict(arc=dict(curvature=(0, 0, 0.01)), n_stations=4, n_sectors=8)), {}),
          (W, "__init__", "clothoid", lambda env: ((env["ctx"],), dict(clothoid=dict(normal=(0, 1, 0), rate=1e-4), n_stations=4,
                                                                       n_sectors=8)), {}),
          (W, "_borrowed", "", lambda env: ((env["ctx"], C.c_void_p(2), env["WallMap"].prm), {}), {}),
          (W, "close", "", no, {}), (W, "arc_struct", "", no, {}), (W, "clothoid_struct", "", no, {}),
          (W, "sync", "", no, {}), (W, "info", "", no, {}),
          (W, "params", "", lambda env: ((), dict(n_stations=4, up=(0, 0, 1))), {}),
          (W, "add_frame", "", lambda env: ((1, POSE), {}), {}),
          (W, "read", "", lambda env: ((1, 2), {}), {}), (W, "read", "all", no, {}),
          (W, "read_raw", "", lambda env: ((1, 2), {}), {}),
          (W, "add_raw", "", lambda env: ((np.zeros((2, 8), api.RAW_CELL), 1), {}), {}),
          (W, "clear", "", lambda env: ((1, 2), {}), {})]
    for name in ("region", "cloud", "clearance", "section", "quantity", "check", "add_checked", "locate", "align", "object"):
        c.append((W, name + "_params", "", no, {}))
    for cap in (0, 3):
        for labels in (False, True):
            c.append((W, "regions", f"cap{cap}_labels{int(labels)}", lambda env, labels=labels: ((), dict(labels=labels)),
                      {"gm_wall_map_regions": cap}))
        c.append((W, "cloud", f"cap{cap}", lambda env: ((1, 2), dict(min_count=2)), {"gm_wall_map_cloud": cap}))
        for n in (0, 2):
            c.append((W, "clearance", f"cap{cap}_n{n}", lambda env, n=n: ((1, n, GAUGE), dict(station_gauge=np.zeros(n, np.uint8))),
                      {"gm_wall_map_clearance": cap}))
        c.append((W, "check_result", f"cap{cap}", lambda env: ((1,), {}), {"gm_wall_map_get_check": cap}))
        for rows in (False, True):
            c.append((W, "check_objects", f"cap{cap}_rows{int(rows)}", lambda env, rows=rows: ((1,), dict(rows=rows, min_points=2)),
                      {"gm_wall_map_get_check": 2, "gm_wall_map_check_objects": cap}))
        c.append((W, "objects_of_rows", f"cap{cap}", lambda env: ((ROWS, 2), {}), {"gm_wall_check_objects": cap}))
        for nt in (0, 2):
            c.append((W, "mesh", f"nv{cap}_nt{nt}", lambda env: ((), dict(flags=1, max_step=0.5)),
                      {"gm_wall_map_mesh": (cap, nt)}))
    # a sized call that reports fewer records than the query did
    c += [(W, "cloud", "cap3_got2", lambda env: ((1, 2), {}), {"gm_wall_map_cloud": [3, 2]}),
          (W, "check_result", "cap3_got2", lambda env: ((1,), {}), {"gm_wall_map_get_check": [3, 2]}),
          (W, "regions", "cap3_got2", no, {"gm_wall_map_regions": [3, 2]}),
          (W, "objects_of_rows", "cap3_got2", lambda env: ((ROWS, 2), {}), {"gm_wall_check_objects": [3, 2]}),
          (W, "clearance", "cap3_got2", lambda env: ((1, 2, GAUGE), {}), {"gm_wall_map_clearance": [3, 2]}),
          (A, "check_result", "cap3_got2", lambda env: ((1,), {}), {"gm_wall_alignment_get_check": [3, 2]})]
    c += [(W, "regions", "baseline", lambda env: ((), dict(baseline=env["base"])), {"gm_wall_map_regions": 0}),
          (W, "sections", "", lambda env: ((1, 2), {}), {"gm_wall_map_sections": 2}),
          (W, "sections", "sums_baseline", lambda env: ((), dict(baseline=env["base"], sums=True)), {"gm_wall_map_sections": 4}),
          (W, "section_basis", "", no, {"gm_wall_section_basis": 40}),
          (W, "section_solve", "", lambda env: ((np.zeros(1, api.WALL_SECTION_SUMS),), {}), {}),
          (W, "section_metrics", "", lambda env: ((np.zeros(1, api.WALL_SECTION),), {}), {}),
          (W, "quantities", "", lambda env: ((GAUGE, GAUGE, 1, 2), {}), {"gm_wall_map_quantities": 2}),
          (W, "quantities", "tables", lambda env: ((GAUGE, GAUGE), dict(baseline=env["base"], section_profile=np.zeros(4, np.uint8),
                                                                        zone=np.zeros(8, np.uint8), profile_rows=True)),
           {"gm_wall_map_quantities": 4}),
          (W, "quantity_metrics", "", lambda env: ((np.zeros(1, api.WALL_QUANTITY),), {}), {}),
          (W, "quantity_runs", "", lambda env: ((np.zeros(2, api.WALL_QUANTITY),), {}), {}),
          (W, "object_metrics", "", lambda env: ((np.zeros(1, api.WALL_OBJECT),), {}), {}),
          (W, "check_frame", "", lambda env: ((1, POSE), dict(threshold=0.1)), {}),
          (W, "add_frame_checked", "", lambda env: ((1, POSE), dict(skip=1)), {}),
          (W, "add_checked_result", "", lambda env: ((1,), {}), {}),
          (W, "locate_frame", "", lambda env: ((1, POSE), dict(gate=0.5)), {}),
          (W, "locate_result", "", lambda env: ((1,), {}), {}),
          (W, "align_frame", "", lambda env: ((1, POSE), dict(gate=0.5)), {}),
          (W, "align_result", "", lambda env: ((1,), {}), {"gm_wall_map_get_align": 1})]
    c += _points(W, "add_points") + _points(W, "check_points", script_name="gm_wall_map_check_points", threshold=0.1)
    c += _points(W, "add_points_checked", extra=(ROWS,)) + _points(W, "add_points_checked", extra=(ROWS[:0],), tag="norows_")[:1]
    c += _points(W, "locate_points", gate=0.5) + _points(W, "align_points", max_station_shift=1)
    # ---- WallAlignmentRule ----
    c += [(R, "__init__", "", lambda env: ((ELEMENTS,), dict(n_sectors=8)), {}), (R, "check", "", no, {}),
          (R, "element_params", "", lambda env: ((1,), {}), {}),
          (R, "project", "", lambda env: ((CLOUDS[5][:2],), {}), {}),
          (R, "point", "", lambda env: (([0.5, 1.5], 0.0, 2.0), {}), {})]
    for cap in (0, 3):
        c.append((R, "window", f"cap{cap}", lambda env: ((0.0, 1.0), {}), {"gm_wall_alignment_window": cap}))
    for target in (R, A):
        bound = (5.0,) if target == R else ()
        c += [(target, "add_plan", "", lambda env, bound=bound: ((POSE,) + bound, {}), {}),
              (target, "locate_plan", "", lambda env, bound=bound: ((POSE,) + bound, {}), {}),
              (target, "align_plan", "", lambda env, bound=bound: ((POSE,) + bound, dict(gate=0.5)), {})]
    c += [(R, "align_select", "", lambda env: ((POSE, 5.0, TABLE), dict(gate=0.5)), {}),
          (A, "align_select", "", lambda env: ((POSE, TABLE), dict(gate=0.5)), {})]
    # ---- WallAlignment ----
    c += [(A, "__init__", "", lambda env: ((env["ctx"], ELEMENTS), dict(n_sectors=8)), {}),
          (A, "close", "", no, {}), (A, "close", "with_element", no, {}),
          (A, "element", "", lambda env: ((1,), {}), {}), (A, "sync", "", no, {}), (A, "info", "", no, {}),
          (A, "add_frame", "", lambda env: ((1, POSE), {}), {}),
          (A, "locate_frame", "", lambda env: ((1, POSE), dict(gate=0.5)), {}), (A, "locate_result", "", lambda env: ((1,), {}), {}),
          (A, "align_frame", "", lambda env: ((1, POSE), dict(gate=0.5)), {}),
          (A, "align_result", "", lambda env: ((1,), {}), {"gm_wall_alignment_get_align": 1}),
          (A, "check_frame", "", lambda env: ((1, POSE), dict(threshold=0.1)), {}),
          (A, "add_frame_checked", "", lambda env: ((1, POSE), dict(skip=1)), {}),
          (A, "add_checked_result", "", lambda env: ((1,), {}), {})]
    for cap in (0, 3):
        c.append((A, "check_result", f"cap{cap}", lambda env: ((1,), {}), {"gm_wall_alignment_get_check": cap}))
    c += _points(A, "add_points") + _points(A, "check_points", script_name="gm_wall_alignment_check_points", threshold=0.1)
    c += _points(A, "add_points_checked", extra=(ROWS,)) + _points(A, "locate_points", gate=0.5)
    c += _points(A, "align_points", max_station_shift=1)
    return c


# the callables that make no ABI call of their own: handle arithmetic, pure converters, context-manager entries (close
# is driven), the properties over the driven *_struct methods, and file I/O around driven methods
EXCLUDED = {
    "WallMap.__enter__", "WallMap.__exit__", "WallMap._h", "WallMap._pose", "WallMap._add_info", "WallMap._check_info",
    "WallMap._add_checked_info", "WallMap._locate_info", "WallMap.arc", "WallMap.clothoid", "WallMap.save", "WallMap.load",
    "WallAlignmentRule.wall_element",
    "WallAlignment.__enter__", "WallAlignment.__exit__", "WallAlignment._h", "WallAlignment._locate_info",
    "WallAlignment._check_info", "WallAlignment.split_cell",
}
# the underscore names that tests and tools reach from outside; every other underscore helper runs only under a public
# method, and all of those are driven
REACHED = ("__init__", "__enter__", "__exit__", "_h", "_pose", "_add_info", "_check_info", "_add_checked_info", "_locate_info",
           "_borrowed")


def _trace(monkeypatch, case, with_result=False):
    target, method, variant, make, script = case
    rec = Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    ctx = api.GeometricMapping(boxFilterBound=5.0)
    env = dict(ctx=ctx, base=ctx.wall_map(n_stations=4, n_sectors=8))
    env["WallMap"] = ctx.wall_map(n_stations=4, n_sectors=8)
    env["WallAlignmentRule"] = api.WallAlignmentRule(ELEMENTS, n_sectors=8)
    env["WallAlignment"] = ctx.wall_alignment(ELEMENTS, n_sectors=8)
    if variant == "with_element":
        env["WallAlignment"].element(0)
    args, kwargs = make(env)
    del rec.log[:]
    rec.script = {k: (list(v) if isinstance(v, list) else v) for k, v in script.items()}
    if method == "__init__":
        result = getattr(api, target)(*args, **kwargs)
    else:
        result = getattr(env[target], method)(*args, **kwargs)
    log = list(rec.log)
    ctx.close()
    return (log, result) if with_result else log


def _key(case):
    return f"{case[0]}.{case[1]}" + (f"[{case[2]}]" if case[2] else "")


def record_golden():
    """Not collected: writes the golden file from the api.py that is importable (run on the commit to hold to)."""
    mp = pytest.MonkeyPatch()
    try:
        out = {_key(c): _trace(mp, c) for c in _cases()}
    finally:
        mp.undo()
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


CASES = _cases()


def test_case_keys_are_unique_and_all_recorded(golden):
    keys = [_key(c) for c in CASES]
    assert len(set(keys)) == len(keys)
    assert set(keys) == set(golden)


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_calls_equal_the_recorded_trace(monkeypatch, golden, case):
    have = json.loads(json.dumps(_trace(monkeypatch, case)))
    want = golden[_key(case)]
    assert [h[0] for h in have] == [w[0] for w in want]
    assert have == want


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "cap3_got2"], ids=_key)
def test_records_are_trimmed_to_what_the_sized_call_reports(monkeypatch, case):
    """The query said 3, the sized call 2: two records come back, and the per-record metrics are made for two."""
    log, result = _trace(monkeypatch, case, with_result=True)
    records = result[2] if case[1] == "clearance" else result[1]
    assert len(records) == 2
    assert sum(1 for c in log if c[0] in ("gm_wall_region_metrics", "gm_wall_object_metrics")) == (2 if len(result) == 4 else 0)


def test_every_callable_is_driven_or_makes_no_call():
    """Every public callable and property of the three classes, inherited ones under the class that defines them (under
    each user for a shared base's), and the underscore names others reach: driven, or listed as making no call."""
    three = (api.WallMap, api.WallAlignmentRule, api.WallAlignment)
    driven = {f"{c[0]}.{c[1]}" for c in CASES}
    seen = set()
    for cls in three:
        for name in dir(cls):
            if name.startswith("_") and name not in REACHED:
                continue
            owner = next(k for k in cls.__mro__ if name in vars(k))
            if owner is object:
                continue
            attr = vars(owner)[name]
            if not (callable(attr) or isinstance(attr, (staticmethod, classmethod, property))):
                continue
            key = f"{(owner if owner in three else cls).__name__}.{name}"
            seen.add(key)
            assert (key in driven) != (key in EXCLUDED), key
    assert EXCLUDED <= seen and driven <= seen and len(seen) > 80


def test_the_skip_rules_take_both_branches(golden):
    """The count query alone when nothing is to fetch, the sized call after it otherwise -- per rule of the binding."""
    def n(key, name):
        return sum(1 for c in golden[key] if c[0] == name)
    assert (n("WallMap.cloud[cap0]", "gm_wall_map_cloud"), n("WallMap.cloud[cap3]", "gm_wall_map_cloud")) == (1, 2)
    assert (n("WallMap.check_result[cap0]", "gm_wall_map_get_check"), n("WallMap.check_result[cap3]", "gm_wall_map_get_check")) == (1, 2)
    assert [n(f"WallMap.regions[cap{c}_labels{l}]", "gm_wall_map_regions") for c in (0, 3) for l in (0, 1)] == [1, 2, 2, 2]
    assert [n(f"WallMap.check_objects[cap{c}_rows{r}]", "gm_wall_map_check_objects") for c in (0, 3) for r in (0, 1)] == [1, 2, 2, 2]
    assert [n(f"WallMap.objects_of_rows[cap{c}]", "gm_wall_check_objects") for c in (0, 3)] == [2, 2]
    assert [n(f"WallMap.mesh[nv{v}_nt{t}]", "gm_wall_map_mesh") for v in (0, 3) for t in (0, 2)] == [1, 1, 2, 2]
    assert [n(f"WallMap.clearance[cap{c}_n{k}]", "gm_wall_map_clearance") for c in (0, 3) for k in (0, 2)] == [1, 2, 1, 2]
    assert n("WallMap.align_result", "gm_wall_map_get_align") == 2
    assert n("WallAlignment.align_result", "gm_wall_alignment_get_align") == 2
    assert [n(f"WallAlignment.check_result[cap{c}]", "gm_wall_alignment_get_check") for c in (0, 3)] == [1, 2]
    for k in golden:   # a *_points method is one device call, whatever it returns
        if "_points" in k:
            assert sum(1 for c in golden[k] if c[0].endswith(k.split(".")[1].split("[")[0])) == 1, k


if __name__ == "__main__":
    record_golden()
