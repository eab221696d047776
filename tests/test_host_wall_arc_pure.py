"""The host-only entries of the wall map on a circular-arc design axis (gm_wall_arc_*) against the twin
(tests/wall_arc_np.py): the design frame at a chainage, project, point, the per-add frame, every refusal of
gm_wall_map_create_arc's rule, and the structs' layout.  No GPU: the library is loaded, no context is made.  The same
entries also run under AddressSanitizer and UBSan in host/gm_wall_arc_host_test.cpp, a stand-alone program linked with
csrc/gm_wall_host.hip alone; nothing loaded into Python is sanitised."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_arc_np as wa  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NEW = ("gm_wall_map_create_arc", "gm_wall_map_get_arc", "gm_wall_arc_check_params", "gm_wall_arc_add_frame", "gm_wall_arc_frame",
       "gm_wall_arc_project", "gm_wall_arc_point")
CASES = {
    "horizontal": (dict(), dict(curvature=(0.0, 1 / 80.0, 0.0), point_chainage=0.0)),
    "vertical": (dict(n_stations=1600), dict(curvature=(0.0, 0.0, -1 / 300.0), point_chainage=120.0)),
    # an oblique plane of curvature on an oblique axis; the curvature's component along the axis is dropped
    "oblique": (dict(point=(3.0, -2.0, 1.0), direction=(1.0, 0.05, 0.02), n_stations=480, t_min=-20.0),
                dict(curvature=(0.004, 0.006, 0.008), point_chainage=12.5)),
}


def _case(name):
    kw, arc = CASES[name]
    p = wn.params(**dict(dict(n_stations=400), **kw))
    return p, arc, api.WallMap.params(**p), api.wall_arc(**arc), wa.design(p, arc)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1.0))


def test_arc_entry_points_and_struct_layouts():
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    fields = {
        "gm_wall_arc": (_lib.WallArc, ("struct_size", "reserved", "curvature", "point_chainage")),
        "gm_wall_arc_add_info": (_lib.WallArcAddInfo, tuple(k for k, _ in _lib.WallArcAddInfo._fields_)),
    }
    lines = []
    for name, (_, fs) in fields.items():
        lines.append(f'printf("%zu ", sizeof({name}));')
        lines += [f'printf("%zu ", offsetof({name}, {f}));' for f in fs]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gm_hip.h"\nint main(void) {\n' + "\n".join(lines) +
           '\nprintf("%zu %zu %zu\\n", sizeof(gm_wall_params), sizeof(gm_wall_add_info), sizeof(gm_wall_info));\nreturn 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = []
    for _, (T, fs) in fields.items():
        want.append(C.sizeof(T))
        want += [getattr(T, f).offset for f in fs]
    assert out[:-3] == want and C.sizeof(_lib.WallArc) == 40 and C.sizeof(_lib.WallArcAddInfo) == 120
    assert out[-3:] == [144, 80, 168]   # gm_wall_params, gm_wall_add_info and gm_wall_info keep their size


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_project_point_against_the_twin(name):
    p, arc, P, A, D = _case(name)
    assert _lib.load().gm_wall_arc_check_params(C.byref(P), C.byref(A)) == _lib.GM_OK
    lo, hi = p["t_min"], p["t_min"] + p["n_stations"] * p["station_length"]
    for s in np.linspace(lo, hi, 7):
        got, want = api.wall_arc_frame(P, A, s), wa.frame(D, s)
        for g, w in zip(got, want):
            assert _rel(g, w) <= 1e-12
    rng = np.random.default_rng(4)
    s, phi, rho = rng.uniform(lo, hi, 2000), rng.uniform(0.0, 2 * np.pi, 2000), 2.0 + rng.uniform(-0.25, 0.25, 2000)
    x = api.wall_arc_point(P, A, s, phi, rho)
    assert _rel(x, wa.point(D, s, phi, rho)) <= 1e-12
    gs, gphi, ge = api.wall_arc_project(P, A, x)
    ws, wphi, we = wa.project(D, x)
    assert _rel(gs, ws) <= 1e-12 and _rel(gphi, wphi) <= 1e-12 and np.abs(ge - we).max() <= 1e-12
    # ... and the library's own round trip
    dphi = np.abs(np.mod(gphi - phi + np.pi, 2 * np.pi) - np.pi)
    assert np.abs(gs - s).max() <= 1e-9 and np.abs(ge - (rho - 2.0)).max() <= 1e-9 and (dphi * rho).max() <= 1e-9


@pytest.mark.parametrize("name", sorted(CASES))
def test_add_frame_against_the_twin(name):
    p, arc, P, A, D = _case(name)
    lo = p["t_min"]
    rng = np.random.default_rng(6)
    for k in range(12):
        s = lo + (0.05 + 0.9 * rng.random()) * p["n_stations"] * p["station_length"]
        o, a, u, v = wa.frame(D, s)
        local = synth.pose_matrix((0, 0, 0), yaw_deg=rng.uniform(-5, 5), roll_deg=rng.uniform(-4, 4), pitch_deg=rng.uniform(-3, 3))
        pose = np.concatenate([np.stack([a, -v, u], axis=1) @ local[:, :3], (o + 0.2 * u - 0.15 * v).reshape(3, 1)], axis=1)
        got, want = api.wall_arc_add_frame(P, A, pose), wa.add_frame(D, p, pose)
        assert got["anchor_station"] == want["anchor"]
        assert abs(got["sensor_chainage"] - want["sensor_chainage"]) <= 1e-12 * max(abs(want["sensor_chainage"]), 1.0)
        assert abs(got["anchor_chainage"] - want["anchor_chainage"]) <= 1e-12 * max(abs(want["anchor_chainage"]), 1.0)
        assert want["anchor_chainage"] <= want["sensor_chainage"] < want["anchor_chainage"] + p["station_length"]
        for key in ("a", "n", "b"):
            assert np.array_equal(got[key], want[key].astype(np.float32)), key
        ulp = np.spacing(np.abs(want["o"].astype(np.float32)))   # (o' is a difference of map-sized numbers: test_chainage's ulp)
        assert np.all(np.abs(got["o"].astype(np.float64) - want["o"]) <= ulp)
        for key in ("kappa", "un", "ub", "vn", "vb", "R"):
            assert float(got[key]) == want[key], key
        assert float(got["station_length"]) == want["ds"] and float(got["gate"]) == want["gate"]
        assert float(got["sector_angle"]) == want["dtheta"]


def test_every_refusal():
    L = _lib.load()
    ok = lambda p, a: L.gm_wall_arc_check_params(C.byref(p), C.byref(a)) == _lib.GM_OK  # noqa: E731
    short, long_ = api.WallMap.params(n_stations=40), api.WallMap.params(n_stations=4000)
    arc = lambda r, s0=0.0, toward=(0.0, 1.0, 0.0): api.wall_arc(np.asarray(toward) / r, s0)  # noqa: E731
    assert ok(short, arc(80.0)) and ok(short, arc(1.0e6)) and ok(short, arc(4.6))
    assert not ok(short, arc(1.1e6))                                     # kappa < 1e-6
    assert not ok(short, arc(4.4))                                       # (R + gate) kappa > 0.5
    assert not ok(long_, arc(300.0)) and ok(long_, arc(300.0, 500.0))    # |psi| > 3 at the far end of the map
    assert not ok(long_, arc(160.0, 500.0))                              # ... at both ends
    assert ok(api.WallMap.params(n_stations=400, t_min=-300.0), arc(100.0)) and not ok(api.WallMap.params(n_stations=400, t_min=-301.0), arc(100.0))
    for bad in (float("nan"), float("inf")):
        assert not ok(short, api.wall_arc((0.0, bad, 0.0), 0.0)) and not ok(short, api.wall_arc((0.0, 0.01, 0.0), bad))
    assert not ok(short, api.wall_arc((0.5, 0.0, 0.0), 0.0))             # along the axis: no curvature is left
    a = arc(80.0)
    a.struct_size = 32
    assert not ok(short, a)
    bad_p = api.WallMap.params(n_stations=40)
    bad_p.radius = -1.0
    assert not ok(bad_p, arc(80.0))
    assert L.gm_wall_arc_check_params(None, C.byref(arc(80.0))) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_arc_check_params(C.byref(short), None) == _lib.GM_ERR_INVALID_ARG
    # the four rules refuse what the check refuses, a NULL, a value that is not finite and a pose that is no rotation
    good, flat = arc(80.0), arc(1.1e6)
    i = _lib.WallArcAddInfo()
    pose = np.ascontiguousarray(np.eye(4)[:3])
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert L.gm_wall_arc_add_frame(C.byref(short), C.byref(good), dp(pose), C.byref(i)) == _lib.GM_OK
    assert i.struct_size == 120 and i.anchor_station == 0 and i.reserved == 0
    assert L.gm_wall_arc_add_frame(C.byref(short), C.byref(flat), dp(pose), C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_arc_add_frame(C.byref(short), C.byref(good), None, C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_arc_add_frame(C.byref(short), C.byref(good), dp(pose), None) == _lib.GM_ERR_INVALID_ARG
    for bad_pose in (pose * 1.01, np.where(np.eye(4)[:3] == 1.0, -1.0, 0.0), np.full((3, 4), np.nan)):
        bp = np.ascontiguousarray(bad_pose, np.float64)
        assert L.gm_wall_arc_add_frame(C.byref(short), C.byref(good), dp(bp), C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    with pytest.raises(_lib.GmError):
        api.wall_arc_frame(short, flat, 1.0)
    with pytest.raises(_lib.GmError):
        api.wall_arc_frame(short, good, float("nan"))
    with pytest.raises(_lib.GmError):
        api.wall_arc_project(short, good, [[0.0, float("inf"), 0.0]])
    with pytest.raises(_lib.GmError):
        api.wall_arc_point(short, good, 1.0, float("nan"), 2.0)
    with pytest.raises(_lib.GmError):
        api.wall_arc_point(short, flat, 1.0, 0.0, 2.0)


def test_arc_host_entries_run_cleanly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gm_wall_arc_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_wall_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_arc_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_arc_host_test ok"), r.stdout + r.stderr
