"""The frames and the guard clouds of tests/test_gpu_wall_curved_chain.py, built on the CPU from the twins alone
(tests/wall_arc_np.py, tests/wall_clothoid_np.py).  tests/test_wall_curved_chain_np.py holds them to the conditions the
GPU file relies on: the share of points that are not `uncertain`, the number of points per guard family, and that the
pins tell a subtly wrong chain from the right one.
"""
import functools

import numpy as np

import fp32_np as fp
import wall_arc_np as wa
import wall_clothoid_np as wl
import wall_np as wn
from geometric_mapping_amd import api, synth

F = np.float32
N = 4097                         # a ragged last wave and a second trip of a 4096-point block
OBLIQUE = (0.0, 0.6, 0.8)
# test_gpu_wall_arc.py's three curvatures, each toward both sides
ARCS = {
    "horizontal_80": dict(arc_radius=80.0, toward=(0.0, 1.0, 0.0)),
    "horizontal_80_right": dict(arc_radius=80.0, toward=(0.0, -1.0, 0.0)),
    "vertical_300": dict(arc_radius=300.0, toward=(0.0, 0.0, -1.0)),
    "vertical_300_up": dict(arc_radius=300.0, toward=(0.0, 0.0, 1.0)),
    "oblique": dict(arc_radius=120.0, toward=OBLIQUE, yaw_deg=8.0, roll_deg=6.0, lateral=0.4),
    "oblique_opposite": dict(arc_radius=120.0, toward=(0.0, -0.6, -0.8), yaw_deg=8.0, roll_deg=6.0, lateral=0.4),
}
# test_gpu_wall_clothoid.py's CURVES (the osculating-arc start: kappa_f at the anchor is far above 1e-6) ...
CLOTHOIDS = {
    "horizontal_from_straight": dict(curvature=0.0, rate=1 / (80.0 * 48.0), toward=(0.0, 1.0, 0.0)),
    "vertical_flattening": dict(curvature=1 / 100.0, rate=-1 / 6000.0, toward=(0.0, 0.0, -1.0)),
    "oblique_s": dict(curvature=-1 / 150.0, rate=1 / (150.0 * 24.0), toward=OBLIQUE, yaw_deg=8.0, roll_deg=6.0, lateral=0.4),
}
# ... and two posed AT params.point (start 0, no lateral offset), where kappa_f is the clothoid's own curvature: exactly 0,
# and 5e-7, both below the 1e-6 of the tangent start.  The strongest rate a 26 m map accepts and a reach of 26 m: the phases go up
# to +-2.7 rad, through two steps of the reduction by pi / 2, and the last bit of a polynomial coefficient moves a sine by
# a good part of its own last bit.  Past 17 m the two Newton steps from the tangent no longer reach the bound on |g|: those
# points are beyond_gate, and their e is compared like any other.
TANGENTS = {
    "tangent_zero": dict(curvature=0.0, rate=0.008, toward=(0.0, 1.0, 0.0), start=0.0, lateral=0.0, reach=26.0),
    "tangent_tiny": dict(curvature=5.0e-7, rate=-0.008, toward=OBLIQUE, start=0.0, lateral=0.0, reach=26.0),
}
NAMES = tuple(f"arc:{k}" for k in list(ARCS) + ["ties"]) + tuple(f"clothoid:{k}" for k in list(CLOTHOIDS) + list(TANGENTS))
GATE, CHECK_GATE = 0.025, 0.01   # the map's gate and the check's own: 2.5 and 1 sigma of the wall's noise, so both reject points


def labels_of(n, every=11):
    return (np.arange(n) % every == 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(kind "arc" | "clothoid", axis (the arc= or clothoid= dict of wall_map), p (wall_np.params), cloud float32
    [N, 3], pose, labels): one frame of the synthetic drive."""
    kind, key = name.split(":")
    if key == "ties":
        return _ties_case()
    if kind == "arc":
        drive = synth.arc_drive(2, N, seed=11, **ARCS[key])
        axis = drive["arc"]
    else:
        drive = synth.clothoid_drive(2, N, seed=11, **dict(CLOTHOIDS, **TANGENTS)[key])
        axis = drive["clothoid"]
    cloud, pose = drive["frames"][0 if key in TANGENTS else 1]
    # 13 m of map (15 m on the tangent frames): the far points of the frame are `outside`
    p = wn.params(n_stations=60 if key in TANGENTS else 52, gate=GATE, **drive["design"])
    return dict(kind=kind, axis=axis, p=p, cloud=cloud, pose=pose, labels=labels_of(N))


def _ties_case():
    """The horizontal 80 m arc seen under the identity pose from params.point: the reported frame is then o' = 0 and
    a', n', b' the unit vectors, so x, y, z of the chain are the point's own coordinates.  Among the wall's points stand 60
    on the outer wall 17.8 .. 18.3 m ahead with x = m 2^-8, m odd (13 bits), y = 2^-40 and z = 0 or 0.01: x x is then
    exactly the midpoint of two fp32 and y y = 2^-80 lies above it, so h = fma(x, x, y y) rounds up, where a sum taken in
    fp64 and rounded again has lost y y and goes to even.  yc is about -2 there, so that ulp of h is an ulp of e."""
    kw = ARCS["horizontal_80"]
    drive = synth.arc_drive(1, 1, **kw)
    p = wn.params(n_stations=52 + 38, gate=GATE, **drive["design"])
    rng = np.random.default_rng(23)
    t, phi = rng.uniform(0.0, 16.5, N), rng.uniform(0.0, 2 * np.pi, N)
    P, _, u, v = synth.arc_sections(t, **kw)
    rr = 2.0 + rng.normal(0.0, 0.01, N)
    cloud = (P + (rr * np.cos(phi))[:, None] * u + (rr * np.sin(phi))[:, None] * v).astype(F)
    m = np.arange(4561, 4681, 2)
    ties = np.stack([m * 2.0 ** -8, np.full(len(m), 2.0 ** -40), np.where(np.arange(len(m)) % 2, 0.01, 0.0)], axis=1).astype(F)
    cloud[5:5 + 67 * len(m):67] = ties
    labels = labels_of(N)
    labels[5:5 + 67 * len(m):67] = 0
    return dict(kind="arc", axis=drive["arc"], p=p, cloud=np.ascontiguousarray(cloud), pose=np.eye(4)[:3], labels=labels,
                ties=np.arange(5, 5 + 67 * len(m), 67))


def reported_frame(c, pose=None):
    """The frame the library reports for the case's map under the pose (host only, no device)."""
    prm = api.WallMap.params(**c["p"])
    pose = c["pose"] if pose is None else pose
    if c["kind"] == "arc":
        return api.wall_arc_add_frame(prm, api.wall_arc(**c["axis"]), pose)
    return api.wall_clothoid_add_frame(prm, api.wall_clothoid(**c["axis"]), pose)


def twin(c, f, xyz, labels, gate=None, shifts=None):
    """The fp32 twin's whole chain on the frame f."""
    return (wa if c["kind"] == "arc" else wl).points_f32(xyz, f, labels, c["p"], gate, shifts)


def share(r):
    """The share of non-plane points that are not uncertain."""
    live = r["cls"] != wn.PLANE
    return float((live & ~r["uncertain"]).sum()) / float(live.sum())


# ---- the guard clouds: points that the header's class lists send to beyond_gate (or outside) before any conversion or index
DESIGN = dict(point=(0.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), radius=2.0, up=(0.0, 0.0, 1.0), forward=(1.0, 0.0, 0.0))
G_ARC = dict(arc_radius=80.0, toward=OBLIQUE)          # 237.5 m of map: |psi| up to 2.97
# the strongest rate a 26 m map of this tunnel accepts: (R + gate) kappa reaches 0.47 and |psi| 2.7 at its end
G_RATE = 0.008
GUARD_POSES = {"arc": 9.5, "clothoid:tangent": 0.0, "clothoid:turned": 22.0}   # the sensor's chainage
PER_FAMILY = 32                  # what a family needs after the plane labels took their share of the DRAWN it starts with
DRAWN = 40
BIG = 1.0e30


def _sections(kind, t):
    if kind == "arc":
        return synth.arc_sections(t, **G_ARC)
    return synth.clothoid_sections(t, 0.0, G_RATE, OBLIQUE)[:4]


def _tube(kind, pose, t, phi, rr):
    """Sensor coordinates (float32) of the points at chainage t, angle phi, radius rr of the guard map's tube."""
    P, _, u, v = _sections(kind, t)
    world = P + (rr * np.cos(phi))[:, None] * u + (rr * np.sin(phi))[:, None] * v
    return np.ascontiguousarray(((world - pose[:, 3]) @ pose[:, :3]).astype(F))


def _specials():
    """1e30 coordinates, then NaN and +-inf coordinates: DRAWN points each."""
    rng = np.random.default_rng(5)
    big = rng.uniform(-3.0, 3.0, (DRAWN, 3))
    odd = rng.uniform(-3.0, 3.0, (DRAWN, 3))
    for i in range(DRAWN):
        big[i, i % 3] = BIG * (-1.0) ** (i // 3)
        if i >= 30:
            big[i, (i + 1) % 3] = -BIG                                  # two at once
        odd[i, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    return big.astype(F), odd.astype(F)


@functools.lru_cache(maxsize=None)
def guard_case(name):
    """One guard cloud: dict(kind, axis, p, pose, cloud float32 [n, 3], labels, family int [n] (-1: an ordinary point of
    the wall near the sensor), names (the families' names)).  The families are chosen with the twin's nominal chain from
    pools drawn here; tests/test_wall_curved_chain_np.py counts them with the whole twin.  The guard points stand at lanes
    0, 17, 31 and 63 of every wave, between ordinary points; every eleventh point is labelled plane."""
    kind = name.split(":")[0]
    rng = np.random.default_rng(17)
    s0 = GUARD_POSES[name]
    P, a_s, u_s, v_s = (x[0] for x in _sections(kind, [s0]))
    local = synth.pose_matrix((0.0, 0.0, 0.0), yaw_deg=3.0, roll_deg=2.0)
    pose = np.concatenate([np.stack([a_s, -v_s, u_s], axis=1) @ local[:, :3], P.reshape(3, 1)], axis=1)
    if kind == "arc":
        drive = synth.arc_drive(1, 1, **G_ARC)
        axis, p = drive["arc"], wn.params(n_stations=950, **DESIGN)
    else:
        n = np.asarray(OBLIQUE) / np.linalg.norm(OBLIQUE)
        axis, p = dict(normal=tuple(n), curvature=0.0, rate=G_RATE, point_chainage=0.0), wn.params(n_stations=104, **DESIGN)
    c = dict(kind=kind, axis=axis, p=p, pose=pose)
    f = reported_frame(c)
    tw = lambda xyz: twin(c, f, xyz, None, shifts=(0,))  # noqa: E731
    gate = F(p["gate"])

    def pool(lo, hi, m, dr=0.2):
        return _tube(kind, pose, rng.uniform(lo, hi, m), rng.uniform(0.0, 2 * np.pi, m), 2.0 + rng.uniform(-dr, dr, m))

    def pick(xyz, mask, count=PER_FAMILY + 16):
        return xyz[np.flatnonzero(mask)[:count]]

    fams = {}
    if kind == "arc":
        # cy <= 0 and |e| within the gate: the wall a quarter turn and more along the arc, ahead (inside the map: a dropped
        # guard maps them) and behind (below station 0); and points beyond the centre of curvature beside the sensor
        R = G_ARC["arc_radius"]
        xyz = np.concatenate([pool(s0 + R * np.deg2rad(100.0), s0 + R * np.deg2rad(170.0), 40),
                              pool(s0 - R * np.deg2rad(170.0), s0 - R * np.deg2rad(100.0), 16)])
        r = tw(xyz)
        fams["cy_in_gate"] = pick(xyz, (r["cy"] < F(-0.05)) & (np.abs(r["e"]) <= gate))
        centre = P + R * np.asarray(OBLIQUE)                            # OBLIQUE is a unit vector
        far = centre + rng.uniform(-1.0, 1.0, (16, 3)) * np.array([30.0, 1.0, 1.0]) + 25.0 * np.asarray(OBLIQUE)
        fams["cy_past_centre"] = ((far - pose[:, 3]) @ pose[:, :3]).astype(F)
    elif name == "clothoid:tangent":
        # the wall far up the axis, where the tangent start is poor: a first or second Newton denominator <= 0.25; a
        # final |g| above the bound with e within the gate (what a dropped bound would map)
        xyz = pool(17.0, 26.0, 4000)
        r = tw(xyz)
        den = ~(r["dens"][0] > F(0.25)) | ~(r["dens"][1] > F(0.25))
        fams["den"] = pick(xyz, den)
        fams["g_in_gate"] = pick(xyz, ~den & (np.abs(r["g"]) > F(wl.G_BOUND)) & (np.abs(r["e"]) <= gate))
        # the search for denominator points that end within the gate and the bound: the wall just past the map's end,
        # which a dropped denominator test would class outside
        xyz = pool(29.4, 30.3, 30_000, dr=0.25)
        r = tw(xyz)
        den = ~(r["dens"][0] > F(0.25)) | ~(r["dens"][1] > F(0.25))
        fams["den_in_gate"] = pick(xyz, den & (np.abs(r["g"]) <= F(wl.G_BOUND)) & (np.abs(r["e"]) <= gate) & np.isfinite(r["t"]), 24)
        # a phase of 2^20 and more at the start: 1e5 .. 1e6 m up the axis
        ph = rng.uniform(-3.0, 3.0, (DRAWN, 3))
        ph[:, 0] = rng.uniform(1.0e5, 1.0e6, DRAWN) * np.where(np.arange(DRAWN) % 2, -1.0, 1.0)
        fams["phase"] = ph.astype(F)
    else:
        # cy <= 0 with e within the gate and every other guard quiet: the wall behind a sensor 22 m into the transition
        xyz = pool(0.0, 13.0, 400)
        r = tw(xyz)
        quiet = (r["dens"][0] > F(0.25)) & (r["dens"][1] > F(0.25)) & (np.abs(r["g"]) <= F(wl.G_BOUND))
        fams["cy_in_gate"] = pick(xyz, (r["cy"] < F(-0.05)) & quiet & (np.abs(r["e"]) <= gate))
    fams["big"], fams["not_finite"] = _specials()
    names = tuple(fams)
    guards = np.concatenate([fams[k] for k in names])
    family = np.concatenate([np.full(len(fams[k]), i) for i, k in enumerate(names)])
    order = rng.permutation(len(guards))                                # the families mixed among the lanes
    guards, family = guards[order], family[order]
    waves = -(-len(guards) // 4)
    n_pts = waves * 64 + 1
    slots = (np.arange(waves)[:, None] * 64 + np.array([0, 17, 31, 63])[None, :]).reshape(-1)[:len(guards)]
    cloud = _tube(kind, pose, rng.uniform(max(0.0, s0 - 5.0), s0 + 5.0, n_pts), rng.uniform(0.0, 2 * np.pi, n_pts),
                  2.0 + rng.normal(0.0, 0.01, n_pts))
    fam = np.full(n_pts, -1)
    cloud[slots], fam[slots] = guards, family
    c.update(cloud=np.ascontiguousarray(cloud), labels=labels_of(n_pts), family=fam, names=names)
    return c


GUARD_NAMES = tuple(GUARD_POSES)


# ---- the |jl| < 4e18 rule of wall_station on the curved axes: stations so short that a point a few centimetres from the
# anchor section lies 1e19 stations away.  (The straight axis has this case in tests/test_gpu_wall_add_edges.py,
# test_both_sides_of_the_lds_window: points at t = +-1e17 .. +-3e38 within the gate.)
@functools.lru_cache(maxsize=None)
def far_station_case(kind):
    """dict(kind, axis, p, pose, cloud, labels None, beyond: the points whose |jl| the twin puts at 4e18 or more)."""
    if kind == "arc":
        # 1e-20 m stations on the 80 m arc, the sensor at params.point (farther along, the anchor station itself is beyond
        # 4e18 and the pose refused): |t| = 0.01, 0.03 (jl = 1e18, 3e18: merely outside)
        # and 0.05, 0.5, 2 (5e18 and more) on both sides
        p = wn.params(n_stations=200, station_length=1.0e-20, **DESIGN)
        axis = synth.arc_drive(1, 1, **G_ARC)["arc"]
        P, a_s, u_s, v_s = (x[0] for x in synth.arc_sections([0.0], **G_ARC))
        pose = np.concatenate([np.stack([a_s, -v_s, u_s], axis=1), P.reshape(3, 1)], axis=1)
        t = np.repeat([0.01, -0.01, 0.03, -0.03, 0.05, -0.05, 0.5, -0.5, 2.0, -2.0], 8)
        phi = np.tile(np.linspace(0.3, 5.9, 8), 10)
        Pt, _, u, v = synth.arc_sections(t, **G_ARC)
        world = Pt + 2.0 * np.cos(phi)[:, None] * u + 2.0 * np.sin(phi)[:, None] * v
        cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(F)
    else:
        # 1e-32 m stations and the rate 2e23 / m^2 that a map of 1000 of them needs (|rate| L >= 1e-6); the sensor at
        # params.point with the identity pose, the points at (x, 0, +-R) exactly: y = 0 keeps the denominators at 1 however
        # large rate t is.  x = 1e-14, 3e-14 (jl = 1e18, 3e18) and 1e-13, 3e-13, 1e-12 (1e19 and more), both signs
        p = wn.params(n_stations=1000, station_length=1.0e-32, **DESIGN)
        axis = dict(normal=(0.0, 1.0, 0.0), curvature=0.0, rate=2.0e23, point_chainage=0.0)
        pose = np.eye(4)[:3]
        x = np.repeat([1e-14, -1e-14, 3e-14, -3e-14, 1e-13, -1e-13, 3e-13, -3e-13, 1e-12, -1e-12], 8)
        cloud = np.stack([x, np.zeros(80), np.tile([2.0, -2.0, 2.125, -1.875], 20)], axis=1).astype(F)
    return dict(kind=kind, axis=axis, p=p, pose=pose, cloud=np.ascontiguousarray(cloud), labels=None)


# ---- the assertions of tests/test_gpu_wall_curved_chain.py.  They stand here so that tests/test_wall_curved_chain_np.py
# can show, on the CPU, that they fail on the outputs of a subtly wrong chain.
def same_bits(x, y):
    return np.array_equal(np.asarray(x, F).view(np.uint32), np.asarray(y, F).view(np.uint32))


def exact_e(c, r):
    """Whether e does not depend on atan2f on this frame: every arc frame, and a clothoid frame with the tangent start."""
    return c["kind"] == "arc" or bool(r["tangent"])


def assert_chain(c, r, res, cell, counts=None):
    """One add's per-point outputs (res, cell) against the twin's whole chain r: NaN and cell -1 on plane points; e bit for
    bit where it is free of atan2f, else inside the twin's envelope over the thirteen starts widened by one ulp (and NaN or
    not as all thirteen say); the cell on every point that is not uncertain.  counts: the device's (mapped, outside,
    beyond_gate, plane) over the points that are not uncertain.  Returns the worst |device - twin| of e in fp32 ulps."""
    res, cell = np.asarray(res, F), np.asarray(cell, np.int64)
    live = r["cls"] != wn.PLANE
    assert np.all(np.isnan(res[~live])) and np.all(cell[~live] == -1)
    if exact_e(c, r):
        assert np.array_equal(np.isnan(res), np.isnan(r["e"]))
        ok = ~np.isnan(r["e"])
        bad = np.flatnonzero(ok & (res.view(np.uint32) != r["e"].view(np.uint32)))
        assert not len(bad), (len(bad), bad[:5], res[bad[:5]], r["e"][bad[:5]])
    else:
        sure = live & ~r["e_mixed"]
        nan = np.isnan(r["e_lo"])
        assert np.array_equal(np.isnan(res[sure]), nan[sure])
        ok = sure & ~nan
        with np.errstate(invalid="ignore"):
            inside = (res >= fp.ulp_steps(r["e_lo"], -1)) & (res <= fp.ulp_steps(r["e_hi"], 1))
        bad = np.flatnonzero(ok & ~inside)
        assert not len(bad), (len(bad), bad[:5], res[bad[:5]], r["e_lo"][bad[:5]], r["e_hi"][bad[:5]])
    fin = ok & np.isfinite(r["e"]) & np.isfinite(res)
    worst = int(np.abs(fp.ulp_distance(r["e"][fin], res[fin])).max()) if fin.any() else 0
    keep = ~r["uncertain"]
    bad = np.flatnonzero(keep & (cell != r["cell"]))
    assert not len(bad), (len(bad), bad[:5], cell[bad[:5]], r["cell"][bad[:5]])
    if counts is not None:
        assert tuple(counts) == wa.class_counts(r, keep), (counts, wa.class_counts(r, keep))
    return worst


def assert_check(r, out, info=None):
    """A check's per-point (cls, cell) against the twin's chain r under the check's own gate, on the points that are not
    uncertain: plane 0, beyond_gate 1, outside 2, and one of the map's classes (3 and up) on a mapped point."""
    keep = ~r["uncertain"]
    want = np.select([r["cls"] == wn.PLANE, r["cls"] == wn.BEYOND, r["cls"] == wn.OUTSIDE], [0, 1, 2], 3)
    got = np.minimum(out["cls"].astype(np.int64), 3)
    bad = np.flatnonzero(keep & (got != want))
    assert not len(bad), (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(out["cell"].astype(np.int64)[keep], r["cell"][keep])
    if info is not None and keep.all():
        mapped, outside, beyond, plane = wa.class_counts(r)
        assert (info["plane"], info["beyond_gate"], info["outside"]) == (plane, beyond, outside)
        assert sum(info[k] for k in ("plane", "beyond_gate", "outside", "unsurveyed", "unchanged", "changed_pos", "changed_neg")) == len(keep)


def assert_guards(c, r, res, cell, counts):
    """A guard cloud's add: assert_chain, and every guard point has cell -1, the counts add up to n, nothing is uncertain."""
    assert not r["uncertain"].any() and sum(counts) == len(res)
    assert np.all(np.asarray(cell)[c["family"] >= 0] == -1)
    return assert_chain(c, r, res, cell, counts)


def thirds(n):
    """The rows that select every third point for a checked add (tests/wall_check_np.POINT records)."""
    import wall_check_np as kn
    rows = np.zeros(len(range(1, n, 3)), kn.POINT)
    rows["index"] = np.arange(1, n, 3)
    rows["delta"] = np.where(rows["index"] % 2 == 0, 1.0, -1.0)
    return rows
