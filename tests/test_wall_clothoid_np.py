"""CPU tests of the wall map on a clothoid design axis (gm_wall_map_create_clothoid): the twin tests/wall_clothoid_np.py
against itself (the device's fp32 chain against the converged fp64 one, P(s) against an independent quadrature), the
host-only entries gm_wall_clothoid_* through ctypes against the twin, every refusal, and the continuity of a
straight -> clothoid -> arc alignment at its two junctions.  No GPU: the library is loaded, no context is made."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_clothoid_np as wl  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NEW = ("gm_wall_map_create_clothoid", "gm_wall_map_get_clothoid", "gm_wall_clothoid_check_params", "gm_wall_clothoid_add_frame",
       "gm_wall_clothoid_frame", "gm_wall_clothoid_project", "gm_wall_clothoid_point")
CASES = {
    # straight to an 80 m radius over 100 m
    "horizontal": (dict(), dict(normal=(0.0, 1.0, 0.0), curvature=0.0, rate=1 / 8000.0, point_chainage=0.0)),
    # a vertical curve that flattens, far along the alignment
    "vertical": (dict(n_stations=800, t_min=5000.0),
                 dict(normal=(0.0, 0.0, -2.0), curvature=1 / 150.0, rate=-1 / 30000.0, point_chainage=5000.0)),
    # an S-transition in an oblique plane on an oblique axis; the normal's component along the axis is dropped
    "oblique_s": (dict(point=(3.0, -2.0, 1.0), direction=(1.0, 0.05, 0.02), n_stations=480, t_min=-20.0),
                  dict(normal=(0.3, 0.6, 0.8), curvature=-1 / 120.0, rate=1 / 7000.0, point_chainage=12.5)),
}


def _case(name):
    kw, cl = CASES[name]
    p = wn.params(**dict(dict(n_stations=400), **kw))
    return p, cl, api.WallMap.params(**p), api.wall_clothoid(**cl), wl.design(p, cl)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1.0))


# ---- the chain ----

def _sweep_case(rng, n, k0, rate, reach, off=2.5):
    """n points at true (t, yc, z) around the anchor section of a frame with (kappa_f, rate), seen from a random sensor
    frame: fp32 points, and the frame as gm_wall_clothoid_add_frame reports it.  The positions come from a 32-node
    quadrature of their own."""
    t = rng.uniform(-reach, reach, n)
    ang, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.5, off, n)
    yc, z = r * np.cos(ang), r * np.sin(ang)
    x32, w32 = np.polynomial.legendre.leggauss(32)
    sg = t[:, None] * (0.5 + 0.5 * x32[None, :])
    ps = (k0 + 0.5 * rate * sg) * sg
    X, Y = 0.5 * t * (np.cos(ps) @ w32), 0.5 * t * (np.sin(ps) @ w32)
    psi = (k0 + 0.5 * rate * t) * t
    px, py = X - yc * np.sin(psi), Y + yc * np.cos(psi)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(A) < 0:
        A[:, 2] = -A[:, 2]
    o = rng.uniform(-0.5, 0.5, 3)
    P = o + px[:, None] * A[:, 0] + py[:, None] * A[:, 1] + z[:, None] * A[:, 2]
    f = dict(o=wl._f32(o), a=wl._f32(A[:, 0]), n=wl._f32(A[:, 1]), b=wl._f32(A[:, 2]), kappa=float(np.float32(k0)),
             rate=float(np.float32(rate)), un=1.0, ub=0.0, vn=0.0, vb=1.0, R=2.0, anchor=50000)
    return P.astype(np.float32), f


def _next_pow2(x):
    return 2.0 ** math.ceil(math.log2(x))


def test_fp32_chain_against_the_converged_fp64_chain():
    """20 000 points per case: kappa_f from 0 to 1 / 80 of either sign and radii up to 100 km, rates up to
    +-1 / (80 * 40) m^-2, S-transitions whose curvature changes sign within the reach, reach 10 to 30 m, offsets up to
    2.5 m.  Measured (and recorded in DESIGN.md): worst |e32 - e64| 2.6e-6 m, worst |t32 - t64| 6.0e-6 m, worst final |g|
    4.8e-6 m, so GM_WALL_CLOTHOID_G_BOUND = 2^-14 m."""
    rng = np.random.default_rng(1)
    p = dict(station_length=0.25, gate=1e9, n_sectors=90, n_stations=100000)
    cases = [(k0, rate, reach) for k0 in (0.0, 1e-5, 1 / 1000.0, 1 / 300.0, 1 / 80.0, -1 / 80.0, 1 / 1e5)
             for rate in (1 / 3200.0, -1 / 3200.0, 2.6e-5, 1e-7, -1e-9) for reach in (10.0, 20.0, 30.0)]
    for reach in (10.0, 20.0, 30.0):
        cases += [(1 / 400.0, -1 / 3200.0, reach), (-1 / 200.0, 1 / 3200.0, reach), (1e-4, -1e-4, reach)]
    worst = dict(e=0.0, t=0.0, g=0.0)
    for k0, rate, reach in cases:
        xyz, f = _sweep_case(rng, 20_000, k0, rate, reach)
        r64, r32 = wl.points(xyz, None, f, p), wl.points_f32(xyz, f)
        assert r64["g"].max() <= 1e-12 and np.all(r64["cls"] == wl.MAPPED)
        assert np.all(r32["cy"] > 0.5) and r32["den"].min() > 0.9
        worst["e"] = max(worst["e"], float(np.abs(r32["e"].astype(np.float64) - r64["e"]).max()))
        worst["t"] = max(worst["t"], float(np.abs(r32["t"].astype(np.float64) - r64["t"]).max()))
        worst["g"] = max(worst["g"], float(np.abs(r32["g"]).max()))
    print(f"sweep: worst |e32 - e64| = {worst['e']:.3e} m, |t32 - t64| = {worst['t']:.3e} m, final |g| = {worst['g']:.3e} m")
    assert worst["e"] <= 5e-6          # the arc tests' tolerance
    assert worst["t"] <= 1e-5
    assert _next_pow2(8.0 * worst["g"]) == wl.G_BOUND == 2.0 ** -14


def test_one_newton_step_is_not_enough(monkeypatch):
    rng = np.random.default_rng(2)
    p = dict(station_length=0.25, gate=1e9, n_sectors=90, n_stations=100000)
    xyz, f = _sweep_case(rng, 20_000, 1 / 80.0, 1 / 3200.0, 30.0)
    r64 = wl.points(xyz, None, f, p)
    monkeypatch.setattr(wl, "DEVICE_NEWTON", 1)
    dt = np.abs(wl.points_f32(xyz, f)["t"].astype(np.float64) - r64["t"]).max()
    print(f"one step: worst |t32 - t64| = {dt:.3e} m")
    assert dt > 2e-5


def test_axis_against_an_independent_quadrature():
    """P(s) over a 1 km map at chainage 5 km against composite Simpson at 24 points per metre: 1e-9 m."""
    p = wn.params(n_stations=1000, station_length=1.0, t_min=5000.0)
    cl = dict(normal=(0.0, 1.0, 0.0), curvature=-1 / 400.0, rate=1 / 200000.0, point_chainage=5000.0)
    P, Cl, D = api.WallMap.params(**p), api.wall_clothoid(**cl), wl.design(p, cl)
    n = 24 * 1000
    tau = np.linspace(0.0, 1000.0, n + 1)
    psi = cl["curvature"] * tau + 0.5 * cl["rate"] * tau * tau
    w = np.ones(n + 1)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    h = tau[1] - tau[0]
    worst = 0.0
    for m in (n, n // 2, 7 * 24 + 12, 333 * 24):      # even counts of intervals: Simpson up to tau[m]
        ws = w[:m + 1].copy()
        ws[-1] = 1.0
        X, Y = h / 3.0 * np.sum(ws * np.cos(psi[:m + 1])), h / 3.0 * np.sum(ws * np.sin(psi[:m + 1]))
        s = 5000.0 + tau[m]
        o = api.wall_clothoid_frame(P, Cl, s)[0]
        tw = wl.frame(D, s)[0]
        worst = max(worst, abs(o[0] - X), abs(o[1] - Y), float(np.abs(o - tw).max()))
    print(f"P(s): worst difference from Simpson and the twin {worst:.3e} m")
    assert worst <= 1e-9


# ---- the host entries ----

def test_entry_points_and_struct_layouts(tmp_path):
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    fields = {"gm_wall_clothoid": _lib.WallClothoid, "gm_wall_clothoid_add_info": _lib.WallClothoidAddInfo}
    lines = []
    for name, T in fields.items():
        lines.append(f'printf("%zu ", sizeof({name}));')
        lines += [f'printf("%zu ", offsetof({name}, {f}));' for f, _ in T._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gm_hip.h"\nint main(void) {\n' + "\n".join(lines) +
           '\nprintf("%zu %zu %zu\\n", sizeof(gm_wall_params), sizeof(gm_wall_arc), sizeof(gm_wall_arc_add_info));\nreturn 0; }\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = []
    for T in fields.values():
        want.append(C.sizeof(T))
        want += [getattr(T, f).offset for f, _ in T._fields_]
    assert out[:-3] == want and C.sizeof(_lib.WallClothoid) == 56 and C.sizeof(_lib.WallClothoidAddInfo) == 128
    assert out[-3:] == [144, 40, 120]   # the structs beside them keep their size


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_project_point_against_the_twin(name):
    p, cl, P, Cl, D = _case(name)
    assert api.wall_clothoid_check_params(P, Cl) == _lib.GM_OK
    lo, hi = p["t_min"], p["t_min"] + p["n_stations"] * p["station_length"]
    for s in np.linspace(lo, hi, 7):
        got, want = api.wall_clothoid_frame(P, Cl, s), wl.frame(D, s)
        for g, w in zip(got[:5], want):
            assert _rel(g, w) <= 1e-12
        assert np.abs(np.cross(got[1], got[5]) - D["b"]).max() <= 1e-12      # n(s): a(s) x n(s) = b
    rng = np.random.default_rng(4)
    s, phi, rho = rng.uniform(lo, hi, 500), rng.uniform(0.0, 2 * np.pi, 500), 2.0 + rng.uniform(-0.25, 0.25, 500)
    x = api.wall_clothoid_point(P, Cl, s, phi, rho)
    assert _rel(x, wl.point(D, s, phi, rho)) <= 1e-12
    gs, gphi, ge = api.wall_clothoid_project(P, Cl, x)
    ws, wphi, we, wg = wl.project(D, x)
    print(f"{name}: the host's Newton leaves |g| <= {wg.max():.2e} m")
    assert wg.max() <= 1e-10
    assert _rel(gs, ws) <= 1e-12 and _rel(gphi, wphi) <= 1e-12 and np.abs(ge - we).max() <= 1e-12
    # ... and the library's own round trip
    dphi = np.abs(np.mod(gphi - phi + np.pi, 2 * np.pi) - np.pi)
    assert np.abs(gs - s).max() <= 1e-9 and np.abs(ge - (rho - 2.0)).max() <= 1e-9 and (dphi * rho).max() <= 1e-9


@pytest.mark.parametrize("name", sorted(CASES))
def test_add_frame_against_the_twin(name):
    p, cl, P, Cl, D = _case(name)
    lo = p["t_min"]
    rng = np.random.default_rng(6)
    for k in range(12):
        s = lo + (0.05 + 0.9 * rng.random()) * p["n_stations"] * p["station_length"]
        o, a, u, v, _ = wl.frame(D, s)
        local = synth.pose_matrix((0, 0, 0), yaw_deg=rng.uniform(-5, 5), roll_deg=rng.uniform(-4, 4), pitch_deg=rng.uniform(-3, 3))
        pose = np.concatenate([np.stack([a, -v, u], axis=1) @ local[:, :3], (o + 0.2 * u - 0.15 * v).reshape(3, 1)], axis=1)
        got, want = api.wall_clothoid_add_frame(P, Cl, pose), wl.add_frame(D, p, pose)
        assert got["anchor_station"] == want["anchor"]
        assert abs(got["sensor_chainage"] - want["sensor_chainage"]) <= 1e-12 * max(abs(want["sensor_chainage"]), 1.0)
        assert abs(got["sensor_chainage"] - s) <= 1e-9
        assert abs(got["anchor_chainage"] - want["anchor_chainage"]) <= 1e-12 * max(abs(want["anchor_chainage"]), 1.0)
        assert want["anchor_chainage"] <= want["sensor_chainage"] < want["anchor_chainage"] + p["station_length"]
        for key in ("a", "n", "b"):
            assert np.abs(got[key].astype(np.float64) - want[key]).max() <= 6e-8, key
        ulp = np.spacing(np.abs(want["o"].astype(np.float32)))
        assert np.all(np.abs(got["o"].astype(np.float64) - want["o"]) <= ulp)
        assert abs(float(got["kappa"]) - want["kappa"]) <= 1e-9 * max(abs(want["kappa"]), 1e-3)
        for key in ("rate", "un", "ub", "vn", "vb", "R"):
            assert float(got[key]) == want[key], key
        assert float(got["station_length"]) == want["ds"] and float(got["gate"]) == want["gate"]
        assert float(got["sector_angle"]) == want["dtheta"]


def test_every_refusal():
    L = _lib.load()
    ok = lambda p, c: api.wall_clothoid_check_params(p, c) == _lib.GM_OK  # noqa: E731
    short, long_ = api.WallMap.params(n_stations=400), api.WallMap.params(n_stations=4000)     # 100 m, 1000 m
    cl = lambda k0=0.0, rate=1 / 8000.0, s0=0.0, normal=(0.0, 1.0, 0.0): api.wall_clothoid(normal, k0, rate, s0)  # noqa: E731
    for p, c in ((short, cl()), (short, cl(1 / 80.0, -1 / 8000.0)), (long_, cl(0.0, 1 / 2.0e5))):
        assert ok(p, c)
    for p, c in ((short, cl()), (long_, cl(0.0, 1 / 2.0e5))):
        assert wl.accepted(dict(wn.params(n_stations=int(p.n_stations))), dict(normal=c.normal[:], curvature=c.curvature,
                                                                               rate=c.rate, point_chainage=c.point_chainage))
    assert ok(short, cl(rate=1.1e-8)) and not ok(short, cl(rate=0.9e-8))        # |rate| L < 1e-6: an arc or a straight
    assert not ok(short, cl(rate=0.0)) and not ok(short, cl(k0=0.01, rate=-0.9e-8))
    tiny = api.WallMap.params(n_stations=40)                                    # 10 m: |psi| stays below 3 at these curvatures
    assert ok(tiny, cl(k0=0.22, rate=1e-5)) and not ok(tiny, cl(k0=0.2222, rate=1e-4))   # (R + gate) max |kappa| > 0.5 at the end
    assert ok(tiny, cl(k0=-0.22, rate=1e-5)) and not ok(tiny, cl(k0=-0.2223, rate=1e-5))  # ... at the map's start
    assert ok(long_, cl(rate=5.9e-6)) and not ok(long_, cl(rate=6.1e-6))        # |psi| > 3 at the far end (rate L^2 / 2)
    assert not ok(long_, cl(rate=5.9e-6, s0=-20.0))                             # ... of a map that starts 20 m on
    # |psi| > 3 only where kappa = 0, inside the map: psi rises to k0^2 / (2 |rate|) = 3.2 at 400 m and is back at 3.0 by 500 m
    assert not ok(api.WallMap.params(n_stations=2000), cl(k0=0.016, rate=-4.0e-5))
    assert ok(api.WallMap.params(n_stations=2000), cl(k0=0.015, rate=-4.0e-5))  # 2.8 there
    for bad in (float("nan"), float("inf")):
        assert not ok(short, cl(k0=bad)) and not ok(short, cl(rate=bad)) and not ok(short, cl(s0=bad))
        assert not ok(short, cl(normal=(0.0, bad, 0.0)))
    assert not ok(short, cl(normal=(0.5, 0.0, 0.0))) and not ok(short, cl(normal=(0.0, 0.0, 0.0)))   # nothing across the axis
    assert not ok(short, cl(normal=(1.0, 0.9e-6, 0.0))) and ok(short, cl(normal=(1.0, 1.1e-6, 0.0)))
    c = cl()
    c.struct_size = 48
    assert not ok(short, c)
    c = cl()
    c.reserved = 1
    assert not ok(short, c)
    bad_p = api.WallMap.params(n_stations=40)
    bad_p.radius = -1.0
    assert not ok(bad_p, cl())
    assert L.gm_wall_clothoid_check_params(None, C.byref(cl())) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_clothoid_check_params(C.byref(short), None) == _lib.GM_ERR_INVALID_ARG
    # the four rules refuse what the check refuses, a NULL, a value that is not finite and a pose that is no rotation
    good, flat = cl(), cl(rate=0.0)
    i = _lib.WallClothoidAddInfo()
    pose = np.ascontiguousarray(np.eye(4)[:3])
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(good), dp(pose), C.byref(i)) == _lib.GM_OK
    assert i.struct_size == 128 and i.anchor_station == 0 and i.reserved[0] == 0 and i.reserved[1] == 0
    assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(flat), dp(pose), C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(good), None, C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(good), dp(pose), None) == _lib.GM_ERR_INVALID_ARG
    for bad_pose in (pose * 1.01, np.where(np.eye(4)[:3] == 1.0, -1.0, 0.0), np.full((3, 4), np.nan)):
        bp = np.ascontiguousarray(bad_pose, np.float64)
        assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(good), dp(bp), C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    far = np.ascontiguousarray(np.eye(4)[:3])
    far[0, 3] = 1.0e300                                                        # a pose whose anchor is out of range
    assert L.gm_wall_clothoid_add_frame(C.byref(short), C.byref(good), dp(far), C.byref(i)) == _lib.GM_ERR_INVALID_ARG
    with pytest.raises(_lib.GmError):
        api.wall_clothoid_frame(short, flat, 1.0)
    with pytest.raises(_lib.GmError):
        api.wall_clothoid_frame(short, good, float("nan"))
    with pytest.raises(_lib.GmError):
        api.wall_clothoid_project(short, good, [[0.0, float("inf"), 0.0]])
    with pytest.raises(_lib.GmError):
        api.wall_clothoid_point(short, good, 1.0, float("nan"), 2.0)
    with pytest.raises(_lib.GmError):
        api.wall_clothoid_point(short, flat, 1.0, 0.0, 2.0)


def _straight_project(D, w):
    """The straight rule in closed form on world points: chainage, angle, e."""
    q = w - D["o"]
    t = q @ D["a"]
    wv = q - t[:, None] * D["a"]
    return t, np.mod(np.arctan2(wv @ D["v"], wv @ D["u"]), 2 * np.pi), np.linalg.norm(wv, axis=1) - D["R"]


def test_junctions_of_a_straight_a_clothoid_and_an_arc():
    """An alignment of a 60 m straight, a 130 m clothoid to R = 300 m and an arc: the clothoid map takes its point and
    direction from the straight's end; the arc map's (point, direction, up) and its curvature kappa n(s) are what
    gm_wall_clothoid_frame reports at the clothoid's end.

    Agreement to 1e-9 (e, angle, and chainage: every map here counts along the whole alignment, the element offset is 0) is
    asserted on the world points of the junctions' own cross-sections, out to the gate: they all lie within 5 m of the
    junction point.  It cannot hold on the rest of a 5 m ball: off the junction section one of the two maps measures
    against its element continued PAST its end, and a clothoid leaves its osculating line or circle by rate t^3 / 6
    (5.3e-4 m at t = 5 m with this rate), which is the reason the feature exists.  There the two maps are asserted to agree
    within that envelope; measured over 4 m either way along the axis: |de| 2.7e-4 m at both junctions, chainages apart by
    up to 4.4e-4 m."""
    Rr, Lc = 300.0, 130.0
    ps = wn.params(n_stations=280, t_min=0.0)                                  # the straight: chainage 0 .. 70
    pc = wn.params(n_stations=600, t_min=50.0, point=(60.0, 0.0, 0.0))         # the clothoid: 50 .. 200, its point at 60
    cl = dict(normal=(0.0, 0.6, 0.8), curvature=0.0, rate=1.0 / (Rr * Lc), point_chainage=60.0)
    Pc, Cl = api.WallMap.params(**pc), api.wall_clothoid(**cl)
    assert api.wall_clothoid_check_params(Pc, Cl) == _lib.GM_OK
    end = 60.0 + Lc
    o, a, u, v, kappa, n = api.wall_clothoid_frame(Pc, Cl, end)
    assert abs(kappa - 1.0 / Rr) <= 1e-15
    pa = wn.params(n_stations=400, t_min=180.0, point=tuple(o), direction=tuple(a), up=tuple(u), forward=tuple(a))
    arc = api.wall_arc(kappa * n, end)
    Pa = api.WallMap.params(**pa)
    assert _lib.load().gm_wall_arc_check_params(C.byref(Pa), C.byref(arc)) == _lib.GM_OK
    D = wn.design_frame(ps)
    rng = np.random.default_rng(8)
    envelope = cl["rate"] * 5.0 ** 3 / 6.0

    def both(w, junction):
        cs_, cphi, ce = api.wall_clothoid_project(Pc, Cl, w)
        os_, ophi, oe = _straight_project(D, w) if junction == 60.0 else api.wall_arc_project(Pa, arc, w)
        dphi = np.abs(np.mod(cphi - ophi + np.pi, 2 * np.pi) - np.pi)
        return np.abs(cs_ - os_).max(), dphi.max(), np.abs(ce - oe).max()

    for junction in (60.0, end):
        jo = api.wall_clothoid_frame(Pc, Cl, junction)[0]
        phi, rho = rng.uniform(0.0, 2 * np.pi, 300), 2.0 + rng.uniform(-0.25, 0.25, 300)
        w = api.wall_clothoid_point(Pc, Cl, np.full(300, junction), phi, rho)
        assert np.linalg.norm(w - jo, axis=1).max() < 5.0
        ds, dphi, de = both(w, junction)
        print(f"junction at {junction}: its section |ds| {ds:.2e} m, |dphi| {dphi:.2e}, |de| {de:.2e} m")
        assert ds <= 1e-9 and dphi <= 1e-9 and de <= 1e-9
        w = api.wall_clothoid_point(Pc, Cl, rng.uniform(junction - 4.0, junction + 4.0, 300), phi, rho)
        assert np.linalg.norm(w - jo, axis=1).max() < 5.0
        ds, dphi, de = both(w, junction)
        print(f"junction at {junction}: a ball of 5 m |ds| {ds:.2e} m, |dphi| {dphi:.2e}, |de| {de:.2e} m (envelope {envelope:.2e} m)")
        assert de <= envelope and ds <= 2.25 * cl["rate"] * 12.5 + envelope and dphi <= 1e-3


def test_host_entries_run_cleanly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gm_wall_clothoid_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_wall_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_clothoid_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_clothoid_host_test ok"), r.stdout + r.stderr
