"""Stray points of a stage call on the kernels over a wall alignment's plan (k_wall_add_joint and its masked form, the joint
check's predicate, k_wall_locate_joint, k_wall_align_bin_joint) and on the single map's locate and align: the clouds, the
fp32 twin of "owner, then the owner's chain", and the assertions of tests/test_gpu_wall_stray.py.  The assertions stand
here so that tests/test_wall_stray_np.py can turn them on a deliberately wrong twin.

include/gm_hip.h promises of every such call: a point whose residual is not finite is beyond_gate (locate: gated); a
curved chain's guards class the point before any integer conversion; a station with |jl| >= 4e18 is outside (align:
outside_patch).  A case is an alignment, a pose and a cloud of ordinary tube points (wall_alignment_np.frame: 90 sectors,
ds 0.25) with stray points planted at lanes 0, 17, 31 and 63 of every wave, as curved_chain_cases.guard_case does; every
eleventh point is labelled plane; n = 64 waves + 1.  The families (family: -1 is an ordinary point):

  not_finite, big   the NaN / +-inf / 1e30 rows of curved_chain_cases._specials(), as they are
  plane_nan         per joint, points whose fp32 d (wall_alignment_np.joint_d32) is NaN: an infinite coordinate along a
                    component where aJ' has the other sign or is 0; and points with d = +inf and d = -inf
  far_ahead,        within the gate of a straight end side's wall, 1e17 stations and more from its anchor.  They exist
  far_behind        where that side's a' is an axis vector up to 1e-16: the plans whose first side is the alignment's first
                    straight carry an identity-rotation pose for that.  A last straight side behind a curve has an oblique
                    a' under every pose (its direction is a rounded cosine and sine), and no fp32 point 1e16 m along an
                    oblique line is within 0.25 m of it: far_ahead exists on the one-side straight plan alone
  cy_in_gate        per arc or clothoid side, the wall a quarter turn and more along that side's own curve (drawn in the
                    side's reported frame, cy < -0.05, every other guard quiet, |e| within the gate) that the planes
                    give to that side: what a dropped guard would map or class outside
  g_in_gate         per clothoid side, the wall a quarter turn and more along that side's own curve that the planes give to it,
                    whose two Newton steps from the osculating start do not reach the bound on |g| (or leave a denominator
                    <= 0.25) while e ends within the gate and t finite: nothing but the chain's `ok` keeps these from
                    surf_station, the window and the table.  (No such point has cy < -0.05 on these transitions of 20 m and
                    less, so cy_in_gate, picked as curved_chain_cases.guard_case's clothoid:turned is, stays empty there)
  past_centre       per arc side, points beyond its centre of curvature that the planes give to it
  on_joint          per joint, points with d == +0.0 exactly (and -0.0 where found), a metre and more off the wall, in front
                    of every earlier joint: the later side owns them.  Per joint Jo' itself, a pool of 10^6 draws in the
                    joint's plane and a lattice aimed at an exact cancellation, picked by joint_d32; a plan in which that
                    finds no more than eight goes without the family

Which plan holds which family is counted by tests/test_wall_stray_np.py (REQUIRED is what it insists on).
"""
import contextlib
import functools

import numpy as np

import curved_chain_cases as cc
import fp32_np as fp
import wall_alignment_locate_cases as lc
import wall_alignment_locate_np as aln
import wall_alignment_np as al_np
import wall_arc_np as wa
import wall_clothoid_np as wl
import wall_np as wn
from geometric_mapping_amd import api

F = np.float32
BOUND = 5.0                       # boxFilterBound of the alignment tests
GATE, CHECK_GATE = 0.25, 0.01     # the maps' gate and the check's narrower one (two sigma of the frame's noise)
LANES = (0, 17, 31, 63)
PER_FAMILY = 8                    # what a family needs after the plane labels took their share
JOINT_PLANS = tuple(sorted(lc.JOINTS))
PLANS = JOINT_PLANS + ("three_sides", "four_sides", "one_straight", "one_arc", "one_clothoid")
ONE_SIDE = {"one_straight": 20.0, "one_arc": 100.0, "one_clothoid": 60.0}   # wall_alignment_locate_cases.LONE's mid-element frames
FAULTS = ("owner_le", "nan_first", "no_guard", "no_4e18", "nonfinite_outside")


def plan_of(name):
    """(elements, the sensor's chainage, the sides the plan must have)."""
    if name in ONE_SIDE:
        return lc.LONE, ONE_SIDE[name], 1
    return lc.record_case(name if name.endswith("_sides") else name + ":before")


@functools.lru_cache(maxsize=None)
def rule_of(name):
    return api.WallAlignmentRule(plan_of(name)[0], **lc.prm())


def _pose_of(name, rule, s):
    """wall_alignment_np.frame's pose; where the plan's first side is the alignment's first straight (which runs along +x
    with u = +z), the identity rotation at frame()'s lateral offset instead: that side's a' is then an axis vector."""
    pose = al_np.frame(rule, s, 1, seed=0)[1]
    if plan_of(name)[0][0]["kind"] == "straight" and rule.add_plan(pose, BOUND)["side_element"][0] == 0:
        return np.concatenate([np.eye(3), np.array([[s], [0.2], [-0.1]])], axis=1)
    return pose


def tube(rule, pose, s, n, seed):
    """wall_alignment_np.frame's wall seen from chainage s, in the sensor coordinates of `pose`: float32 [n, 3]."""
    cloud, p0 = al_np.frame(rule, s, n, seed=seed)
    world = cloud.astype(np.float64) @ p0[:, :3].T + p0[:, 3]
    return np.ascontiguousarray(((world - pose[:, 3]) @ pose[:, :3]).astype(F))


# ---- the sides of a plan and the twin of a joint call -------------------------------------------------------------------
KINDS = {aln.STRAIGHT: "straight", aln.ARC: "arc", aln.CLOTHOID: "clothoid"}


def sides_of(rule, pose, bound=BOUND):
    """(the add's plan dict, per side dict(kind, element, p, f)): f is the frame the element's own add reports under the
    pose (api.wall_arc_add_frame / wall_clothoid_add_frame; a straight side's by wall_np.add_frame), p
    what the chains' twins read of the element's gm_wall_params."""
    lp = rule.locate_plan(pose, bound)
    add = lp["add"]
    blk = aln.blocks(lp, dict(o=lp["c"], a=lp["d"], u=lp["u"], v=lp["v"]))
    out = []
    for k, i in enumerate(add["side_element"]):
        ep, arc, cl = rule.element_params(i)
        p = dict(n_stations=int(ep.n_stations), n_sectors=int(ep.n_sectors), station_length=float(ep.station_length), gate=float(ep.gate))
        if cl is not None:
            kind, f = "clothoid", api.wall_clothoid_add_frame(ep, cl, pose)
        elif arc is not None:
            kind, f = "arc", api.wall_arc_add_frame(ep, arc, pose)
        else:
            # wall_np.add_frame, the host's rule for an element map's own add restated.  (The plan's start holds the same
            # four vectors as images under the home section, equal to the last bit but for components of 1e-17, which a
            # point 1e19 m along the axis multiplies into metres.)
            kind = "straight"
            wp = wn.params(t_min=float(ep.t_min), point=tuple(ep.point), direction=tuple(ep.direction), radius=float(ep.radius),
                           up=tuple(ep.up), forward=tuple(ep.forward), **p)
            w = wn.add_frame(wn.design_frame(wp), wp, pose)
            f = dict(o=w["o"].astype(F), a=w["a"].astype(F), u=w["u"].astype(F), v=w["v"].astype(F), anchor_station=int(w["anchor"]),
                     R=F(w["R"]), station_length=F(w["ds"]), sector_angle=F(w["dtheta"]), gate=F(w["gate"]))
            assert np.abs(np.stack([f[q] for q in "oauv"]) - blk["side"][k]).max() < 1e-15
        assert kind == KINDS[lp["side_kind"][k]] and int(f["anchor_station"]) == int(add["side_anchor"][k])
        out.append(dict(kind=kind, element=int(i), p=p, f=f))
    return add, out


def straight_points_f32(xyz, f, labels=None, p=None, gate=None, shifts=None):
    """wall_chain on a straight side in float32, operation by operation (surf_residual, surf_station, wall_station,
    surf_sector): wall_clothoid_np.points_f32's dict.  Two operations are the device's own.  surf_rho takes its root with
    __fsqrt_rn, which is the bare v_sqrt_f32 here (csrc/gm_device.hpp says so at sqrt_rn) and good to one ulp: e_lo and e_hi
    are e with the root one ulp down and up, and a point whose class differs among the three is uncertain.  The sector's
    angle is atan2f(w.v', w.u'), moved by the shifts as in wall_arc_np.points_f32."""
    e, t, w, rho = aln.straight_f32(xyz, [f["o"], f["a"]], f["R"])
    u, v = np.asarray(f["u"], F), np.asarray(f["v"], F)
    with np.errstate(all="ignore"):
        cu = fp.fma32(w[:, 0], u[0], fp.fma32(w[:, 1], u[1], w[:, 2] * u[2]))
        cv = fp.fma32(w[:, 0], v[0], fp.fma32(w[:, 1], v[1], w[:, 2] * v[2]))
        e_lo, e_hi = (fp.ulp_steps(rho, -1) - F(f["R"])).astype(F), (fp.ulp_steps(rho, 1) - F(f["R"])).astype(F)
    # arc_sector's twin on (cu, cv) with un = vb = 1, ub = vn = 0 is atan2f(cv, cu)
    fr = dict(f, un=1.0, ub=0.0, vn=0.0, vb=1.0)
    shifts = wa.SHIFTS if shifts is None else shifts
    ok = np.ones(len(e), bool)
    out = dict(e=e, t=t, tangent=False, e_lo=e_lo, e_hi=e_hi, e_mixed=np.zeros(len(e), bool))
    out.update(wa.bin_f32([(e, ok, t, cu, cv), (e_lo, ok, t, cu, cv), (e_hi, ok, t, cu, cv)], fr, p, labels, gate, shifts))
    out["e"] = np.where(out["cls"] == wn.PLANE, F(np.nan), e)
    return out


def side_twin(side, xyz, labels, gate=None, rows=None, shifts=None):
    """The whole chain of one side on float32 points.  rows: (row0, n_rows) in the place of the map's (anchor, n_stations):
    an align's patch, whose cell is jr n_sectors + k."""
    f, p = side["f"], side["p"]
    if rows is not None:
        f, p = dict(f, anchor_station=int(rows[0])), dict(p, n_stations=int(rows[1]))
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    if side["kind"] == "straight":
        return straight_points_f32(xyz, f, labels, p, gate, shifts)
    return cc.twin(dict(kind=side["kind"], p=p), f, xyz, labels, gate, shifts)


def owner_side(xyz, add, fault=None):
    """The owner of every point as an index into the plan's sides (wall_alignment_np.owner32's rule)."""
    ns = add["n_sides"]
    with np.errstate(invalid="ignore", over="ignore"):
        if fault is None:
            return al_np.owner32(xyz, dict(add, side_element=list(range(ns)))).astype(np.int64)
        side = np.full(len(xyz), ns - 1, np.int64)
        nan = np.zeros(len(xyz), bool)
        for k in range(ns - 2, -1, -1):
            d = al_np.joint_d32(xyz, add["joint_o"][k], add["joint_a"][k])
            side[(d <= 0.0) if fault == "owner_le" else (d < 0.0)] = k
            nan |= np.isnan(d)
        if fault == "nan_first":
            side[nan] = 0
        return side


@contextlib.contextmanager
def _no_guard(on):
    """The chains' twins without their guards: cy > 0 on both curved axes; on a clothoid also the denominators, the
    finiteness of t and the bound on |g| (everything `ok` holds)."""
    old = wa.GUARD_CY, wl.GUARD_DEN, wl.GUARD_G
    wa.GUARD_CY = wl.GUARD_DEN = wl.GUARD_G = not on
    try:
        yield
    finally:
        wa.GUARD_CY, wl.GUARD_DEN, wl.GUARD_G = old


def joint_twin(add, sides, xyz, labels, gate=None, rows=None, fault=None, shifts=None):
    """Owner, then the owner's chain: dict(side, element, e float32, cls (wall_np's classes), cell, uncertain, jl, r (per
    side: the side's own twin dict on the rows idx[k])).  fault: one of FAULTS, a kernel that is wrong in one line."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    side = owner_side(xyz, add, fault if fault in ("owner_le", "nan_first") else None)
    out = dict(side=side, element=np.asarray(add["side_element"], np.int32)[side], e=np.full(n, np.nan, F), cls=np.full(n, wn.PLANE, np.int8),
               cell=np.full(n, -1, np.int64), uncertain=np.zeros(n, bool), jl=np.zeros(n, F), r=[], idx=[])
    for k, S in enumerate(sides):
        idx = np.flatnonzero(side == k)
        with _no_guard(fault == "no_guard"):
            r = side_twin(S, xyz[idx], lab[idx], gate, None if rows is None else rows[k], shifts)
        if fault == "no_4e18":       # the conversion of any jl, saturating as numpy's does, and the station clamped into the map
            nst = int(S["p"]["n_stations"] if rows is None else rows[k][1])
            anchor = int(S["f"]["anchor_station"] if rows is None else rows[k][0])
            with np.errstate(all="ignore"):
                far = (r["cls"] == wn.OUTSIDE) & ~(np.abs(r["jl"]) < F(4.0e18))
                j = np.clip(np.clip(np.nan_to_num(r["jl"].astype(np.float64), nan=0.0), -2.0 ** 62, 2.0 ** 62).astype(np.int64) + anchor, 0, nst - 1)
            r["cls"] = np.where(far, wn.MAPPED, r["cls"]).astype(np.int8)
            r["cell"] = np.where(far, j * int(S["p"]["n_sectors"]), r["cell"])
        if fault == "nonfinite_outside":
            with np.errstate(all="ignore"):
                bad = (r["cls"] == wn.BEYOND) & ~np.isfinite(r["e"])
            r["cls"] = np.where(bad, wn.OUTSIDE, r["cls"]).astype(np.int8)
        out["r"].append(r)
        out["idx"].append(idx)
        for q in ("e", "cls", "cell", "uncertain", "jl"):
            out[q][idx] = r[q]
    return out


def class_rows(tw, keep=None):
    """[n_sides, 4] (mapped, outside, beyond_gate, plane) of a twin over the rows of `keep`: the sides' totals after an add."""
    keep = np.ones(len(tw["side"]), bool) if keep is None else keep
    return np.array([[int((keep & (tw["side"] == k) & (tw["cls"] == q)).sum()) for q in (wn.MAPPED, wn.OUTSIDE, wn.BEYOND, wn.PLANE)]
                     for k in range(len(tw["r"]))], np.int64)


# ---- the clouds -----------------------------------------------------------------------------------------------------------
def _curve_xy(kind, f, t):
    """(x, y, psi) of the side's own axis at arc length t from the anchor section, in the side's frame (a', n'): the circle,
    or the clothoid by the midpoint rule on 4000 panels."""
    k = float(f["kappa"])
    if kind == "arc":
        psi = k * t
        return np.sin(psi) / k, (1.0 - np.cos(psi)) / k, psi
    c = float(f["rate"])
    m = 4000
    s = (np.arange(m) + 0.5)[None, :] / m * t[:, None]
    ps = (k + 0.5 * c * s) * s
    return t * np.cos(ps).mean(axis=1), t * np.sin(ps).mean(axis=1), (k + 0.5 * c * t) * t


def _quarter_turn_pool(side, rng, m):
    """Wall points (radius 2 +- 0.2) of the side's own curve continued 95 .. 265 degrees of turn from the anchor section, on
    both sides of it, in sensor coordinates."""
    f, kind = side["f"], side["kind"]
    k, c = float(f["kappa"]), float(f.get("rate", 0.0))
    turn = np.deg2rad(rng.uniform(95.0, 265.0, m)) * np.where(rng.uniform(size=m) < 0.5, -1.0, 1.0)
    if kind == "arc":
        t = turn / k
    else:   # psi(t) = (k + c t / 2) t = turn: the root on the side where the curvature grows in magnitude
        sg = np.where(rng.uniform(size=m) < 0.5, -1.0, 1.0)
        disc = k * k + 2.0 * c * turn
        t = np.where(disc >= 0.0, (-k + sg * np.sqrt(np.abs(disc))) / c, np.nan)
        t = t[np.isfinite(t) & (np.abs(t) < 400.0)]
    x, y, psi = _curve_xy(kind, f, t)
    phi, rr = rng.uniform(0.0, 2 * np.pi, len(t)), 2.0 + rng.uniform(-0.2, 0.2, len(t))
    yc, z = rr * np.cos(phi), rr * np.sin(phi)
    o, a, nn, b = (np.asarray(f[q], np.float64) for q in ("o", "a", "n", "b"))
    px, py = x - yc * np.sin(psi), y + yc * np.cos(psi)
    return (o + px[:, None] * a + py[:, None] * nn + z[:, None] * b).astype(F)


def _far_pool(side, sign):
    """Points of a straight side's wall 1e17 .. 1.2e39 stations along sign * a' (the construction of
    test_gpu_wall_add_edges.py::test_both_sides_of_the_lds_window, with the side's own o', a', u', v')."""
    f = side["f"]
    o, a, u, v = (np.asarray(f[q], np.float64) for q in ("o", "a", "u", "v"))
    st = np.repeat([1e17, 1e18, 3.9e18, 4.1e18, 1e19, 1e20, 4e30, 1.2e39], 4) * float(f["station_length"]) * sign
    phi = np.linspace(0.3, 5.9, len(st))
    w = 2.0 * np.cos(phi)[:, None] * u + 2.0 * np.sin(phi)[:, None] * v
    with np.errstate(over="ignore"):
        return (o + st[:, None] * a + w).astype(F)


def _joint_pool(jo, ja, m=1_000_000, seed=0):
    """10^6 float32 points about the joint's plane: Jo' + r1 e1 + r2 e2, e1 and e2 spanning the plane, |r| = 1 so that the
    point is a metre inside the design tube (beyond every gate here)."""
    rng = np.random.default_rng([29, seed])
    a = np.asarray(ja, np.float64)
    e1 = np.cross(a, [0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    phi = rng.uniform(0.0, 2 * np.pi, m)
    return (np.asarray(jo, np.float64) + np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2).astype(F)


def _joint_lattice(jo, ja, seed=0):
    """Float32 points aimed at d == 0 on an oblique plane whose aJ' has two components that are not 0: q_a = -2^-k along the
    larger one (its product with aJ'_a is then exact, for k = -2 .. 13 and both signs) and every float32 p_b within 3000
    ulps of the q_b that cancels it; the third coordinate is drawn.  192 032 points per joint; none where aJ' is an axis vector
    (_joint_pool serves that)."""
    rng = np.random.default_rng([41, seed])
    jo, ja = np.asarray(jo, F), np.asarray(ja, F)
    order = np.argsort(-np.abs(ja))
    ia, ib, ic = (int(x) for x in order)
    if ja[ib] == 0.0:
        return np.zeros((0, 3), F)
    out = []
    for k, sg in [(k, sg) for k in range(-2, 14) for sg in (-1.0, 1.0)]:
        pa = F(jo[ia] + F(sg * 2.0 ** -k))
        qa = F(pa - jo[ia])
        qb = F(-(np.float64(qa) * np.float64(ja[ia])) / np.float64(ja[ib]))
        pb = _ulp_range(F(jo[ib] + qb), 3000)
        p = np.zeros((len(pb), 3), F)
        p[:, ia], p[:, ib], p[:, ic] = pa, pb, jo[ic] + rng.uniform(-0.5, 0.5, len(pb)).astype(F)
        out.append(p)
    return np.concatenate(out)


def _ulp_range(x, m):
    """The 2 m + 1 float32 values within m ulps of x (finite, not near 0)."""
    i = np.asarray(x, F).view(np.int32).astype(np.int64) + np.arange(-m, m + 1)
    return i.astype(np.int32).view(F)


def _neg_zero(x):
    return (x == 0.0) & np.signbit(x)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, rule, els, s, pose, add (the plan), sides, cloud float32 [n, 3], labels, family int [n], names, found:
    per family the points drawn before the plane labels, neg_zeros: the on_joint points with d == -0.0)."""
    els, s, want = plan_of(name)
    rule = rule_of(name)
    pose = _pose_of(name, rule, s)
    add, sides = sides_of(rule, pose)
    assert add["n_sides"] == want
    ns = add["n_sides"]
    rng = np.random.default_rng([31, PLANS.index(name)])
    nominal = lambda xyz: joint_twin(add, sides, xyz, None, shifts=(0,))  # noqa: E731
    fams, neg_zeros = {}, 0
    big, odd = cc._specials()
    fams["not_finite"], fams["big"] = odd, big
    with np.errstate(all="ignore"):
        if ns > 1:   # plane_nan: NaN, +inf and -inf d at every joint
            rows = []
            for j in range(ns - 1):
                jo, ja = add["joint_o"][j], add["joint_a"][j]
                pool = rng.uniform(-3.0, 3.0, (96, 3)).astype(F)
                for i in range(96):
                    pool[i, i % 3] = (np.inf, -np.inf)[(i // 3) % 2]
                    if i >= 48:
                        pool[i, (i + 1) % 3] = (np.inf, -np.inf)[(i // 6) % 2]      # two at once: inf - inf where the signs say so
                d = al_np.joint_d32(pool, jo, ja)
                rows += [pool[np.isnan(d)][:12], pool[d == np.inf][:6], pool[d == -np.inf][:6]]
            fams["plane_nan"] = np.concatenate(rows)
            zeros = []
            for j in range(ns - 1):
                jo, ja = add["joint_o"][j], add["joint_a"][j]
                pool = np.concatenate([np.asarray(jo, F).reshape(1, 3), _joint_lattice(jo, ja, seed=j), _joint_pool(jo, ja, seed=j)])
                d = al_np.joint_d32(pool, jo, ja)
                mine = np.zeros(len(pool), bool)     # in front of every earlier joint: the side behind joint j owns it
                z = np.flatnonzero(d == 0.0)
                mine[z] = owner_side(pool[z], add) == j + 1
                pos, neg = pool[mine & ~np.signbit(d)], pool[mine & _neg_zero(d)]
                zeros += [pos[:10], neg[:6]]
            if sum(len(z) for z in zeros) > PER_FAMILY:      # (Jo' itself is always one: a family needs more than that)
                fams["on_joint"] = np.concatenate(zeros)
            neg_zeros = sum(len(z) for z in zeros[1::2])
        for k, S in enumerate(sides):
            if S["kind"] == "straight" and k in (0, ns - 1):
                for sign, fam in ((-1.0, "far_behind"), (1.0, "far_ahead")):
                    if (k == 0 and sign < 0) or (k == ns - 1 and sign > 0):
                        xyz = _far_pool(S, sign)
                        r = nominal(xyz)
                        ok = (r["side"] == k) & (r["cls"] == wn.OUTSIDE) & ~(np.abs(r["jl"]) < F(1.0e17))
                        if ok.any():
                            fams[fam] = xyz[ok]
            if S["kind"] != "straight":
                xyz = _quarter_turn_pool(S, rng, 6000)
                r = nominal(xyz)
                rs = side_twin(S, xyz, None, shifts=(0,))
                quiet = np.ones(len(xyz), bool)
                if S["kind"] == "clothoid":
                    quiet = np.all(rs["dens"] > F(0.25), axis=0) & (np.abs(rs["g"]) <= F(wl.G_BOUND)) & np.isfinite(rs["t"])
                ok = (r["side"] == k) & (rs["cy"] < F(-0.05)) & quiet & (np.abs(rs["e"]) <= F(GATE))
                if ok.any():
                    fams["cy_in_gate"] = np.concatenate([fams.get("cy_in_gate", np.zeros((0, 3), F)), xyz[ok][:14]])
                if S["kind"] == "clothoid":
                    # the same wall where nothing but `ok` stops it: e within the gate, t finite, and beyond_gate in the
                    # whole twin at every one of the thirteen starts (curved_chain_cases.guard_case's g_in_gate)
                    pick = np.flatnonzero((r["side"] == k) & (r["cls"] == wn.BEYOND) & np.isfinite(rs["t"]) & (np.abs(rs["e"]) <= F(GATE)))[:80]
                    whole = side_twin(S, xyz[pick], None)
                    sure = ~whole["uncertain"] & ~whole["e_mixed"] & (whole["cls"] == wn.BEYOND) & (np.abs(whole["e_hi"]) <= F(GATE)) & (np.abs(whole["e_lo"]) <= F(GATE))
                    if sure.any():
                        fams["g_in_gate"] = np.concatenate([fams.get("g_in_gate", np.zeros((0, 3), F)), xyz[pick[sure]][:14]])
            if S["kind"] == "arc":
                f = S["f"]
                o, a, nn, b = (np.asarray(f[q], np.float64) for q in ("o", "a", "n", "b"))
                m = 4000
                kap = float(f["kappa"])
                x = rng.uniform(-30.0, 30.0, m)
                y = 1.0 / kap + np.sign(kap) * rng.uniform(5.0, 50.0, m)      # 5 .. 50 m beyond the centre of curvature
                far = (o + x[:, None] * a + y[:, None] * nn + rng.uniform(-1.0, 1.0, m)[:, None] * b).astype(F)
                r = nominal(far)
                ok = (r["side"] == k) & (side_twin(S, far, None, shifts=(0,))["cy"] < F(0.0))
                if ok.any():
                    fams["past_centre"] = np.concatenate([fams.get("past_centre", np.zeros((0, 3), F)), far[ok][:10]])
    names = tuple(fams)
    stray = np.concatenate([fams[q] for q in names])
    family = np.concatenate([np.full(len(fams[q]), i) for i, q in enumerate(names)])
    order = rng.permutation(len(stray))
    stray, family = stray[order], family[order]
    waves = max(-(-len(stray) // 4), 16)
    if name in ("clothoid_arc", "four_sides"):
        waves = 64                                      # 4097 points: a second trip of a 4096-point block
    assert len(stray) <= 4 * waves <= 256, (name, len(stray))
    n = 64 * waves + 1
    slots = (np.arange(waves)[:, None] * 64 + np.array(LANES)[None, :]).reshape(-1)
    again = np.arange(len(slots)) % len(stray)          # every wave carries four: the rows are dealt round again
    stray, family = stray[again], family[again]
    cloud = tube(rule, pose, s, n, seed=61 + PLANS.index(name))
    fam = np.full(n, -1)
    cloud[slots], fam[slots] = stray, family
    return dict(name=name, rule=rule, els=els, s=s, pose=pose, add=add, sides=sides, cloud=np.ascontiguousarray(cloud),
                labels=cc.labels_of(n), family=fam, names=names, found={q: len(fams[q]) for q in names}, neg_zeros=neg_zeros)


_COMMON, _JOINT = ("not_finite", "big"), ("plane_nan",)
_ARC_END = ("cy_in_gate", "past_centre")      # an END side that is an arc: a middle side's wedge closes at its centre of curvature
_CLOTHOID = ("g_in_gate",)                    # an END side that is a clothoid: a middle side owns the slab between its two planes,
#                                               which holds its wall only where the chain converges (100 000 draws found none)
REQUIRED = {
    "arc_arc": _COMMON + _JOINT + _ARC_END, "arc_clothoid": _COMMON + _JOINT + _ARC_END + _CLOTHOID,
    "clothoid_arc": _COMMON + _JOINT + _ARC_END + _CLOTHOID, "clothoid_straight": _COMMON + _JOINT + _CLOTHOID,
    "straight_clothoid": _COMMON + _JOINT + _CLOTHOID + ("far_behind", "on_joint"),
    "three_sides": _COMMON + _JOINT + ("far_behind", "on_joint"), "four_sides": _COMMON + _JOINT + ("far_behind", "on_joint"),
    "one_straight": _COMMON + ("far_behind", "far_ahead"), "one_arc": _COMMON + _ARC_END, "one_clothoid": _COMMON + _CLOTHOID,
}


def stray(c):
    return c["family"] >= 0


def of_family(c, fam):
    return c["family"] == c["names"].index(fam) if fam in c["names"] else np.zeros(len(c["family"]), bool)


# ---- the single straight map: families 1 and 3 ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straight_case():
    """dict(p (wall_np.params: 176 stations), pose, cloud, labels, family, names): synth.tunnel_drive's wall seen under the
    identity rotation with not_finite, big, far_ahead and far_behind at the stray lanes."""
    from geometric_mapping_amd import synth
    drive = synth.tunnel_drive(1, 1025, seed=5)
    p = wn.params(n_stations=176, **drive["design"])
    pose = np.concatenate([np.eye(3), np.array([[20.0], [0.2], [-0.1]])], axis=1)
    f = wn.add_frame(wn.design_frame(p), p, pose)
    side = dict(kind="straight", element=0, p=p, f=dict(o=f["o"].astype(F), a=f["a"].astype(F), u=f["u"].astype(F), v=f["v"].astype(F),
                                                          anchor_station=f["anchor"], R=F(f["R"]), station_length=F(f["ds"]),
                                                          sector_angle=F(f["dtheta"]), gate=F(f["gate"])))
    big, odd = cc._specials()
    fams = {"not_finite": odd, "big": big, "far_ahead": _far_pool(side, 1.0), "far_behind": _far_pool(side, -1.0)}
    names = tuple(fams)
    rng = np.random.default_rng(37)
    stray_, family = np.concatenate([fams[q] for q in names]), np.concatenate([np.full(len(fams[q]), i) for i, q in enumerate(names)])
    order = rng.permutation(len(stray_))
    stray_, family = stray_[order], family[order]
    waves = -(-len(stray_) // 4)
    n = 64 * waves + 1
    slots = (np.arange(waves)[:, None] * 64 + np.array(LANES)[None, :]).reshape(-1)[:len(stray_)]
    t, phi = 20.0 + rng.uniform(-4.5, 4.5, n), rng.uniform(0.0, 2 * np.pi, n)
    rr = 2.0 + synth.wall_texture(t, phi, seed=5) + rng.normal(0.0, 0.005, n)
    D = wn.design_frame(p)
    world = D["o"] + t[:, None] * D["a"] + (rr * np.cos(phi))[:, None] * D["u"] + (rr * np.sin(phi))[:, None] * D["v"]
    cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(F)
    fam = np.full(n, -1)
    cloud[slots], fam[slots] = stray_, family
    add = dict(n_sides=1, side_element=[0], side_anchor=[f["anchor"]], joint_o=np.zeros((0, 3), F), joint_a=np.zeros((0, 3), F))
    return dict(name="straight_map", p=p, pose=pose, add=add, sides=[side], cloud=np.ascontiguousarray(cloud), labels=cc.labels_of(n),
                family=fam, names=names)


# ---- the assertions of tests/test_gpu_wall_stray.py -------------------------------------------------------------------------
def want_class(c, tw, gate=None):
    """Per stray row the class its family was built for, as wall_np's: plane where labelled; outside for far_ahead and
    far_behind (whose |e| is within the map's gate; under a narrower gate those whose |e| exceeds it are beyond_gate) and
    for a `big` row that the twin puts 4e18 stations and more away with a finite e inside the gate (a 1e30 coordinate along
    an a' that is an axis vector); beyond_gate otherwise."""
    gate = F(GATE if gate is None else gate)
    with np.errstate(invalid="ignore"):
        far = (of_family(c, "far_ahead") | of_family(c, "far_behind")) & (np.abs(tw["e"]) <= gate)
        far |= of_family(c, "big") & (tw["cls"] == wn.OUTSIDE) & ~(np.abs(tw["jl"]) < F(4.0e18))
    return np.where(c["labels"] == 1, wn.PLANE, np.where(far, wn.OUTSIDE, wn.BEYOND))


def assert_twin_classes(c, tw, gate=None):
    """The conditions on a case's twin: no stray point is uncertain, every one has its family's class and no cell."""
    s = stray(c)
    assert not tw["uncertain"][s].any()
    assert np.array_equal(tw["cls"][s], want_class(c, tw, gate)[s]) and np.all(tw["cell"][s] == -1)


def assert_add(c, tw, element, res, cell, totals):
    """One joint add's outputs against the twin tw (joint_twin of the case under the map's gate).  element, res, cell: the
    per-point outputs; totals [n_sides, 4]: the sides' (mapped, outside, beyond_gate, plane) after an add of the rows that are
    not uncertain.  The owner is owner32's on every row; per side curved_chain_cases.assert_chain (e bit for bit or inside
    the envelope, class counts and cells of the decidable points); every stray row has cell -1; the totals add up."""
    n = len(c["cloud"])
    with np.errstate(invalid="ignore", over="ignore"):
        owner = al_np.owner32(c["cloud"], c["add"])
    bad = np.flatnonzero(np.asarray(element) != owner)
    assert not len(bad), (len(bad), bad[:5], np.asarray(element)[bad[:5]], owner[bad[:5]])
    assert set(np.unique(owner)) <= set(c["add"]["side_element"])
    assert np.all(np.asarray(cell)[stray(c)] == -1)
    assert not tw["uncertain"][stray(c)].any()
    totals = np.asarray(totals, np.int64)
    assert int(totals.sum()) == int((~tw["uncertain"]).sum()) and n == len(res) == len(cell)
    worst = 0
    for k, S in enumerate(c["sides"]):
        idx, r = tw["idx"][k], tw["r"][k]
        worst = max(worst, cc.assert_chain(dict(kind=S["kind"]), r, np.asarray(res)[idx], np.asarray(cell)[idx], tuple(int(v) for v in totals[k])))
    return worst


def assert_check(c, tw, out, info, gate=None):
    """One joint check's outputs against the twin tw under the check's gate: owner, per side curved_chain_cases.assert_check
    on class and cell, side_class rows summing to the summed classes and to n, stray rows without a cell and plane (0),
    beyond_gate (1) or, far_ahead and far_behind, outside (2)."""
    n = len(c["cloud"])
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(out["element"], al_np.owner32(c["cloud"], c["add"]))
    for k in range(len(c["sides"])):
        idx = tw["idx"][k]
        cc.assert_check(tw["r"][k], {q: out[q][idx] for q in ("cls", "cell")})
    sc = np.asarray(info["side_class"], np.int64)
    assert int(sc.sum()) == n == info["n_points"]
    names = ("plane", "beyond_gate", "outside", "unsurveyed", "unchanged", "changed_pos", "changed_neg")
    assert [int(info[q]) for q in names] == [int(v) for v in sc.sum(axis=0)]
    s = stray(c)
    assert np.all(out["cell"][s] == -1)
    want = np.select([want_class(c, tw, gate) == wn.PLANE, want_class(c, tw, gate) == wn.BEYOND], [0, 1], 2)
    assert np.array_equal(out["cls"][s].astype(np.int64), want[s])
    if not tw["uncertain"].any():
        rows = class_rows(tw)
        assert np.array_equal(sc[:, :3], rows[:, [3, 2, 1]]) and np.array_equal(sc[:, 3:].sum(axis=1), rows[:, 0])


def assert_align(c, tw, out, info):
    """One align's per-point outputs and counts against the twin tw (joint_twin over the patch rows under the align's
    gate): owner, cell -1 on stray rows, e NaN or not as the twin says, cell on the decidable rows, and plane, beyond_gate,
    outside_patch, binned (and the side_class rows) the twin's."""
    s = stray(c)
    if "element" in out:
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.array_equal(out["element"], al_np.owner32(c["cloud"], c["add"]))
    assert np.all(out["cell"][s] == -1) and not tw["uncertain"][s].any()
    assert np.array_equal(np.isnan(out["e"][s]), np.isnan(tw["e"][s]))
    keep = ~tw["uncertain"]
    assert np.array_equal(out["cell"].astype(np.int64)[keep], tw["cell"][keep])
    rows = class_rows(tw)[:, [3, 2, 1, 0]]   # plane, beyond_gate, outside_patch, binned
    slack = int(tw["uncertain"].sum())
    got = np.array([info[q] for q in ("plane", "beyond_gate", "outside_patch", "binned")], np.int64)
    assert got.sum() == len(s) and np.abs(got - rows.sum(axis=0)).max() <= slack, (got, rows.sum(axis=0), slack)
    if "side_class" in info:
        sc = np.asarray(info["side_class"], np.int64)
        assert np.array_equal(sc.sum(axis=0), got) and np.abs(sc - rows).max() <= slack, (sc, rows)
