"""gm_wall_alignment_regions and its kin without a GPU: the symbols, the struct layouts from plain C99, the host-only
gm_wall_alignment_region_window and _region_metrics against the twin (tests/wall_alignment_regions_np.py), the refusals that
need no device, and the ABI calls the binding's methods make."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_np as rn  # noqa: E402
import wall_alignment_regions_np as an  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_alignment_regions", "gm_wall_alignment_region_window", "gm_wall_alignment_region_metrics")
N_STATIONS = [12, 17, 12, 9]   # bases 0, 12, 29, 41; total 50
ELEMENTS = [dict(kind="straight", n_stations=12), dict(kind="clothoid", n_stations=17, turn=(0.0, 1.0), curvature=0.0, rate=0.01 / 4.25),
            dict(kind="arc", n_stations=12, turn=(0.0, 1.0), curvature=0.01), dict(kind="straight", n_stations=9)]
PRM = dict(wn.DEFAULTS, n_sectors=10, station_length=0.25, t_min=3.5)
STATUS = {"ok": _lib.GM_OK, "invalid": _lib.GM_ERR_INVALID_ARG, "unsupported": _lib.GM_ERR_UNSUPPORTED}


def rule(elements=ELEMENTS, **over):
    return api.WallAlignmentRule(elements, **{k: v for k, v in dict(PRM, **over).items() if k != "n_stations"})


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {"gm_wall_alignment_regions_info": _lib.WallAlignmentRegionsInfo,
              "struct gm_wall_alignment_region_metrics": _lib.WallAlignmentRegionMetrics}
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("%u\\n", (unsigned)GM_WALL_ALIGNMENT_REGION_MAX_CELLS);')
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
    assert out == want + [an.MAX_CELLS]
    assert C.sizeof(_lib.WallAlignmentRegionsInfo) == 112 and C.sizeof(_lib.WallAlignmentRegionMetrics) == 120
    # the shared heads, at the same offsets
    for head, whole in ((_lib.WallRegionsInfo, _lib.WallAlignmentRegionsInfo), (_lib.WallRegionMetrics, _lib.WallAlignmentRegionMetrics)):
        for f, _t in head._fields_:
            assert getattr(head, f).offset == getattr(whole, f).offset, f
        assert getattr(whole, whole._fields_[len(head._fields_)][0]).offset == C.sizeof(head)


def _window_status(r, station0, n):
    try:
        r.region_window(station0, n)
    except _lib.GmError as e:
        return e.status
    return _lib.GM_OK


B = an.bases(N_STATIONS)
WINDOWS = ([(b, 1) for b in B[:-1]] + [(b - 1, 1) for b in B[1:]] + [(b - 1, 2) for b in B[1:-1]] +      # starts, ends, joints
           [(B[i], N_STATIONS[i]) for i in range(4)] + [(0, 50), (5, 30), (12, 29), (13, 27), (29, 0), (50, 0), (0, 0)])


@pytest.mark.parametrize("station0,n", WINDOWS)
def test_region_window_equals_twin(station0, n):
    assert an.window_status(N_STATIONS, 10, station0, n) == "ok"
    got = rule().region_window(station0, n)
    assert got == an.window(PRM, N_STATIONS, station0, n)
    assert set(got) == set(an.INFO_KEYS) and all(got[k] == 0 for k in an.COUNTS)
    if n:   # the fields determine the pieces: consecutive elements that cover the window
        rows = sum(N_STATIONS[got["element_from"]:got["element_to"] + 1]) - got["station_from"] - (N_STATIONS[got["element_to"]] - 1 - got["station_to"])
        assert rows == n and B[got["element_from"]] + got["station_from"] == station0


def test_region_window_on_256_elements_of_one_station():
    els = [dict(kind="arc", n_stations=1, turn=(0.0, 1.0), curvature=0.01) if i % 3 == 0 else dict(kind="straight", n_stations=1)
           for i in range(256)]
    r = rule(els)
    for s0, n in ((0, 256), (100, 57), (255, 1), (0, 1)):
        assert r.region_window(s0, n) == an.window(PRM, [1] * 256, s0, n)
    assert r.region_window(0, 256)["n_pieces"] == 256


@pytest.mark.parametrize("station0,n", [(50, 1), (0, 51), (49, 2), (2 ** 32 - 1, 2), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_region_window_refuses_a_window_outside(station0, n):
    assert an.window_status(N_STATIONS, 10, station0, n) == "invalid"
    assert _window_status(rule(), station0, n) == _lib.GM_ERR_INVALID_ARG


def test_the_size_rule_refuses_with_unsupported():
    """128 elements of 4096 stations x 4096 sectors hold 2^31 cells: one too many for an int32 label; with 127 the labels
    fit, and a window of 2^26 cells is the largest."""
    el = dict(kind="straight", n_stations=4096)
    big, fits = rule([el] * 128, n_sectors=4096), rule([el] * 127, n_sectors=4096)
    assert big.check() == _lib.GM_OK
    for r, ns, cases in ((big, [4096] * 128, [(0, 1), (0, 0), (2 ** 31, 5)]),
                         (fits, [4096] * 127, [(0, 1), (0, 16384), (0, 16385), (500000, 16385), (127 * 4096, 1), (127 * 4096 - 16384, 16384)])):
        for s0, n in cases:
            assert _window_status(r, s0, n) == STATUS[an.window_status(ns, 4096, s0, n)], (s0, n)
    assert _window_status(big, 0, 1) == _lib.GM_ERR_UNSUPPORTED            # the first arm, ahead of the window
    assert _window_status(fits, 0, 16384) == _lib.GM_OK
    assert _window_status(fits, 0, 16385) == _lib.GM_ERR_UNSUPPORTED       # the second arm
    assert _window_status(fits, 127 * 4096 - 3, 16385) == _lib.GM_ERR_INVALID_ARG   # ... behind the window
    assert fits.region_window(4095, 4098)["n_pieces"] == 3


def region(st_min, st_max, peak_station, peak_sector, peak, ns=10):
    r = np.zeros((), rn.REGION)
    r["label"], r["sign"], r["cells"] = st_min * ns + 2, (1 if peak > 0 else -1), 7
    r["station_min"], r["station_max"] = st_min, st_max
    r["sector_min"], r["sector_max"], r["sector_min_turned"], r["sector_max_turned"] = 0, 9, 3, 6
    r["peak_cell"], r["peak"], r["sum_d"], r["points"] = peak_station * ns + peak_sector, peak, 5 * peak + 3, 99
    return r


def _metrics_equal(got, want):
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), (k, got[k], v)
    assert set(got) == set(want)


METRIC_CASES = [("inside one element", region(14, 20, 17, 4, 300001), (1, 2, 1, 8, 1, 5, 4)),
                ("across one joint", region(10, 13, 12, 0, -222222), (0, 10, 1, 1, 1, 0, 0)),
                ("across two joints", region(27, 43, 30, 9, 77777), (1, 15, 3, 2, 2, 1, 9)),
                ("the first cell", region(0, 0, 0, 0, 60000), (0, 0, 0, 0, 0, 0, 0)),
                ("the last cell", region(49, 49, 49, 9, -60000), (3, 8, 3, 8, 3, 8, 9))]


@pytest.mark.parametrize("name,r,want", METRIC_CASES, ids=[c[0] for c in METRIC_CASES])
def test_region_metrics_equal_twin(name, r, want):
    A = rule()
    got = A.region_metrics(r)
    _metrics_equal(got, an.metrics(A, PRM, N_STATIONS, r))
    assert tuple(got[k] for k in ("element_from", "station_from", "element_to", "station_to", "peak_element", "peak_station",
                                  "peak_sector")) == want
    # the peak's design position: gm_wall_alignment_point of the stated arguments, bit for bit
    G, k = divmod(int(r["peak_cell"]), 10)
    chainage, angle, rho = 3.5 + (G + 0.5) * 0.25, an.TWO_PI * (k + 0.5) / 10.0, 2.0 + int(r["peak"]) * 2.0 ** -20
    assert (chainage, angle, rho) == an.peak_arguments(PRM, r)
    assert got["peak_point"].tobytes() == A.point(chainage, angle, rho)[0].tobytes()
    assert got["chainage_from"] == 3.5 + int(r["station_min"]) * 0.25
    head = api.wall_region_metrics(A.prm, r)
    assert all(got[k] == head[k] for k in head)


def test_region_metrics_refusals():
    A, L = rule(), _lib.load()
    bad = [region(49, 50, 49, 0, 1), region(13, 12, 12, 0, 1), region(3, 4, 50, 0, 1), region(3, 4, 2 ** 32 // 10, 5, 1)]
    for f, v in (("cells", 0), ("sector_max", 10), ("sector_max_turned", 10), ("sector_min", 10)):
        r = region(3, 4, 3, 0, 1)
        r[f] = v
        bad.append(r)
    for r in bad:
        with pytest.raises(_lib.GmError) as e:
            A.region_metrics(r)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
    ok = np.ascontiguousarray(region(3, 4, 3, 0, 1).reshape(1))
    rp, out = ok.ctypes.data_as(C.POINTER(_lib.WallRegion)), _lib.WallAlignmentRegionMetrics()
    assert L.gm_wall_alignment_region_metrics(*A._head(), rp, C.byref(out)) == _lib.GM_OK
    assert L.gm_wall_alignment_region_metrics(*A._head(), None, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_alignment_region_metrics(*A._head(), rp, None) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_alignment_region_metrics(None, A._els, 4, rp, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_alignment_region_metrics(C.byref(A.prm), A._els, 0, rp, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    # a refused alignment
    e = api.WallAlignmentRule([dict(kind="arc", n_stations=4, curvature=-1.0, turn=(0.0, 1.0))], n_sectors=10)
    with pytest.raises(_lib.GmError):
        e.region_metrics(region(0, 1, 0, 0, 1))
    assert _window_status(e, 0, 1) == _lib.GM_ERR_INVALID_ARG


def test_refusals_without_a_device():
    L = _lib.load()
    info, got = _lib.WallAlignmentRegionsInfo(), C.c_uint32(7)
    ok = api.WallMap.region_params()
    assert L.gm_wall_alignment_regions(None, None, 0, 1, C.byref(ok), C.byref(info), None, 0, C.byref(got), None) == _lib.GM_ERR_INVALID_ARG
    r = rule()
    assert L.gm_wall_alignment_region_window(*r._head(), 0, 1, None) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_alignment_region_window(None, r._els, 4, 0, 1, C.byref(info)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_alignment_region_window(C.byref(r.prm), None, 4, 0, 1, C.byref(info)) == _lib.GM_ERR_INVALID_ARG
    assert not hasattr(r, "regions")   # the device call is a WallAlignment's


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


@pytest.mark.parametrize("cap,labels,n_calls", [(0, False, 1), (3, False, 2), (0, True, 2), (3, True, 2)])
def test_the_binding_makes_a_count_query_then_the_sized_call(monkeypatch, cap, labels, n_calls):
    rec = Recorder({"gm_wall_alignment_regions": (-2, cap)})
    monkeypatch.setattr(_lib, "_lib", rec)
    ctx = api.GeometricMapping(boxFilterBound=5.0)
    al = ctx.wall_alignment(ELEMENTS[:2], n_sectors=8)
    base = ctx.wall_alignment(ELEMENTS[:2], n_sectors=8)
    del rec.log[:]
    info, reg, metrics, lab = al.regions(3, labels=labels, baseline=base, min_cells=2)
    names = [c[0] for c in rec.log if not c[0].endswith("_default_params")]   # (every **params starts from the defaults)
    assert names == ["gm_wall_alignment_regions"] * n_calls + ["gm_wall_alignment_region_metrics"] * cap
    calls = [c[1] for c in rec.log if c[0] == "gm_wall_alignment_regions"]
    assert all(c[1] == "ptr" and c[2:4] == (3, 12 + 17 - 3) for c in calls)   # the baseline; n None: to the alignment's end
    assert calls[0][6:8] == (None, 0) and calls[0][9] is None                 # the query: no records, no labels
    if n_calls == 2:
        assert calls[1][6:8] == ("ptr", cap) and calls[1][9] == ("ptr" if labels else None)
    assert len(reg) == len(metrics) == cap and (lab is None) == (not labels) and (not labels or lab.shape == (26, 8))
    assert set(info) == set(an.INFO_KEYS)
    del rec.log[:]
    al.regions(0, 0)
    assert [c[1][2:4] for c in rec.log if c[0] == "gm_wall_alignment_regions"] == [(0, 0)] * (2 if cap else 1)
    al.region_window(2, 5)
    assert rec.log[-1][0] == "gm_wall_alignment_region_window" and rec.log[-1][1][3:5] == (2, 5)
    ctx.close()
