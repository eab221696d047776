"""numpy twin of the locate on a wall alignment (gm_wall_alignment_locate_*, csrc/k_wall_locate_joint.hip +
gm_wall_alignment.hip; include/gm_hip.h states the rule).

A plan (WallAlignmentRule.locate_plan) holds what a locate starts from: the state, s0, the home section and every side's
block and every joint plane as attached vectors h in the home section.  image() / blocks() are the header's image of those
under a state.  one_pass() is one Gauss-Newton pass on blocks a pass REPORTED (or on any blocks): the owner by the fp32
rule of wall_alignment_np.owner32, the owner's chain in float32 by the chains' own twins (straight_f32 here,
wall_arc_np.points_f32, wall_clothoid_np.points_f32), the radial direction, the row J, the sums and the solve in fp64.
exact=True runs the chains in fp64 as well (wall_clothoid_np.points' converged foot): the variant whose result is the
floor of what any fp32 chain can reach.  locate() is the whole call: three passes, the update, the attached vectors
following, the composed pose.  A plan of one straight side IS the element map's locate (wall_locate_np.locate), as in the
header.

FAULTS names three deliberate errors (a wrong owner at a joint, a tilt about c instead of the sensor's foot, a side left
unmoved by the update) that the assertions shared with the GPU test must catch: tests/test_wall_alignment_locate_np.py.
"""
import numpy as np

import fp32_np as fp
import wall_alignment_np as al_np
import wall_arc_np as wa
import wall_clothoid_np as wcl
import wall_locate_np as ln

F = np.float32
DESIGN, MAP = ln.DESIGN, ln.MAP
OK, DEGENERATE, SINGULAR, FAILED_MASK, NOT_CONVERGED = ln.OK, ln.DEGENERATE, ln.SINGULAR, ln.FAILED_MASK, ln.NOT_CONVERGED
STRAIGHT, ARC, CLOTHOID = 0, 1, 2
CLASSES = ln.CLASSES
FAULTS = ("owner", "tilt_about_c", "side_unmoved")


def _f32(x):
    return np.asarray(x, np.float64).astype(F).astype(np.float64)


def image(h, point, state):
    """The header's image of an attached vector h [.., 3] under the state (o = c, a = d, u, v), fp64."""
    h = np.asarray(h, np.float64)
    r = (h[..., 0:1] * state["a"] + h[..., 1:2] * state["u"]) + h[..., 2:3] * state["v"]
    return state["o"] + r if point else r


def blocks(plan, state, rounded=True):
    """dict(side [ns, 4, 3], joint_o, joint_a [ns - 1, 3]) of the plan under the state; rounded to fp32 once unless told."""
    side = np.concatenate([image(plan["side"][:, :1], True, state), image(plan["side"][:, 1:], False, state)], axis=1)
    jo, ja = image(plan["joint"][:, 0], True, state), image(plan["joint"][:, 1], False, state)
    rd = _f32 if rounded else (lambda x: np.asarray(x, np.float64))
    return dict(side=rd(side), joint_o=rd(jo), joint_a=rd(ja))


def straight_f32(xyz, blk, R):
    """The straight side's chain in float32, operation by operation: e, t, w (float32)."""
    x = np.asarray(xyz, F).reshape(-1, 3)
    o, a = np.asarray(blk[0], F), np.asarray(blk[1], F)
    with np.errstate(all="ignore"):
        q = x - o
        t = fp.fma32(q[:, 0], a[0], fp.fma32(q[:, 1], a[1], q[:, 2] * a[2]))
        w = np.stack([fp.fma32(-t, a[k], q[:, k]) for k in range(3)], axis=1)
        rho = np.sqrt(fp.fma32(w[:, 0], w[:, 0], fp.fma32(w[:, 1], w[:, 1], w[:, 2] * w[:, 2])))
        return (rho - F(R)).astype(F), t, w, rho


def _curved_frame(blk, axis, R, anchor, grid):
    return dict(o=blk[0], a=blk[1], n=blk[2], b=blk[3], kappa=float(axis[0]), rate=float(axis[1]), un=float(axis[2]), ub=float(axis[3]),
                vn=float(axis[4]), vb=float(axis[5]), R=float(F(R)), anchor=int(anchor), ds=float(F(grid["station_length"])),
                dtheta=float(F(2 * np.pi / grid["n_sectors"])), gate=1.0e30)


def side_chain(xyz, kind, blk, axis, grid, anchor, n_stations, exact=False):
    """One side's chain on its block [4, 3]: dict(e, t, rho, nrm [n, 3] fp64, guard, cell (the twin's own, -1 outside the
    side's map), e_lo / e_hi (the clothoid chain's atan2f envelope; e itself elsewhere)).  exact: everything in fp64."""
    R = float(F(grid["radius"]))
    ns = int(grid["n_sectors"])
    ds, dth = float(F(grid["station_length"])), float(F(2 * np.pi / ns))
    b64 = np.asarray(blk, np.float64)
    x64 = np.asarray(xyz, F).astype(np.float64).reshape(-1, 3)
    n = len(x64)
    guard = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if kind == STRAIGHT:
            if exact:
                q = x64 - b64[0]
                t = q @ b64[1]
                w = q - t[:, None] * b64[1]
                rho = np.sqrt((w * w).sum(1))
                e = rho - R
            else:
                e, t, w, rho = straight_f32(xyz, blk, R)
            e_lo = e_hi = e
            w64 = np.asarray(w, np.float64)
            nrm = w64 / np.asarray(rho, np.float64)[:, None]
            phi = np.mod(np.arctan2(w64 @ b64[3], w64 @ b64[2]), 2 * np.pi)
        else:
            f = _curved_frame(b64, axis, R, anchor, grid)
            p = dict(n_stations=int(n_stations), n_sectors=ns, station_length=grid["station_length"], gate=8.0)
            mod = wa if kind == ARC else wcl
            if exact:
                r = mod.points(x64, None, f, p, gate=1.0e30)
                e, t, yc, z = r["e"], r["t"], r["yc"], r["z"]
                guard = r["cls"] != mod.BEYOND
                e_lo = e_hi = e
            else:
                r = mod.points_f32(xyz, f, labels=None, p=p, gate=1.0e30)
                e, t, yc, z = r["e"], r["t"], r["yc"], r["z"]
                guard = r["cls"] != mod.BEYOND
                e_lo, e_hi = (r["e_lo"], r["e_hi"]) if kind == CLOTHOID else (e, e)
            t64, yc64, z64 = (np.asarray(v, np.float64) for v in (t, yc, z))
            psi = f["kappa"] * t64 if kind == ARC else (f["kappa"] + 0.5 * f["rate"] * t64) * t64
            nt = np.cos(psi)[:, None] * b64[2] - np.sin(psi)[:, None] * b64[1]
            rho = np.sqrt(yc64 * yc64 + z64 * z64)
            nrm = (yc64[:, None] * nt + z64[:, None] * b64[3]) / rho[:, None]
            phi = np.mod(np.arctan2(yc64 * f["vn"] + z64 * f["vb"], yc64 * f["un"] + z64 * f["ub"]), 2 * np.pi)
        t64 = np.asarray(t, np.float64)
        fin = np.isfinite(t64) & guard
        j = anchor + np.floor(np.where(fin, t64 / ds, 0.0)).astype(np.int64)
        k = np.minimum(np.floor(np.where(np.isfinite(phi), phi / dth, 0.0)), ns - 1).astype(np.int64)
        cell = np.where(fin & (j >= 0) & (j < n_stations), j * ns + k, -1)
    return dict(e=np.asarray(e), t=t64, rho=np.asarray(rho, np.float64), nrm=nrm, guard=guard, cell=cell, e_lo=np.asarray(e_lo),
                e_hi=np.asarray(e_hi))


def one_pass(xyz, labels, home, s0, blk, gate, plan, grid, n_stations, raws=None, min_count=8, cells=None, exact=False,
             fault=None):
    """One pass.  home: the pass's state (o, a, u, v as the points saw it); blk: blocks()' dict or a pass record's side,
    joint_o, joint_a; plan: side_element, side_kind, side_axis, side_anchor (an info dict or locate_plan()'s);
    n_stations: per side; raws: per side the owner's raw cells (MAP) or None (DESIGN); cells: the device's own cell per point.
    Returns wall_locate_np.one_pass's dict plus element (the owner's element per point) and res_lo / res_hi."""
    x = np.asarray(xyz, F).reshape(-1, 3)
    n = len(x)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    ns = len(plan["side_element"])
    g = float(F(gate))
    owner_plan = dict(n_sides=ns, side_element=list(range(ns)), joint_o=blk["joint_o"], joint_a=blk["joint_a"])
    side = al_np.owner32(x, owner_plan).astype(np.int64)
    if fault == "owner" and ns > 1:   # the plane of the first joint ignored
        side = np.where(side == 0, 1, side)
    e = np.full(n, np.nan)
    e_lo, e_hi = np.full(n, np.nan), np.full(n, np.nan)
    rho, t = np.zeros(n), np.zeros(n)
    nrm = np.zeros((n, 3))
    guard = np.zeros(n, bool)
    cell = np.full(n, -1, np.int64)
    m = np.zeros(n)
    unsurveyed = np.zeros(n, bool)
    for k in range(ns):
        sel = side == k
        if not sel.any():
            continue
        anchor = int(plan["side_anchor"][k])
        r = side_chain(x[sel], plan["side_kind"][k], blk["side"][k], plan["side_axis"][k], grid, anchor, n_stations[k], exact=exact)
        e[sel], e_lo[sel], e_hi[sel], rho[sel], t[sel], nrm[sel], guard[sel] = r["e"], r["e_lo"], r["e_hi"], r["rho"], r["t"], r["nrm"], r["guard"]
        if raws is not None:
            ck = r["cell"] if cells is None else np.asarray(cells, np.int64)[sel]
            cell[sel] = ck
            has = ck >= 0
            cnt = raws[k]["count"].reshape(-1).astype(np.int64)
            un = np.zeros(len(ck), bool)
            un[has] = cnt[ck[has]] < min_count
            mk = np.zeros(len(ck))
            okc = has & ~un
            mk[okc] = ln.mean_q(raws[k])[ck[okc]].astype(np.float64) * 2.0 ** -20
            unsurveyed[sel], m[sel] = un, mk
    plane = lab == 1
    with np.errstate(invalid="ignore"):
        bad = ~plane & (~np.isfinite(e) | ~guard)
        live = ~plane & ~bad
        outside = live & (cell < 0) if raws is not None else np.zeros(n, bool)
        unsurveyed = live & ~outside & unsurveyed
        at_gate = live & ~outside & ~unsurveyed
        mm = m if exact else m.astype(F)
        res = (e - mm) if exact else (e.astype(F) - mm).astype(F).astype(np.float64)
        res_lo, res_hi = e_lo - m, e_hi - m
        used = at_gate & (np.abs(res) < g) & (rho > 0)
        amb = at_gate & ((np.abs(np.abs(res) - g) < 1e-5) | (np.abs(np.abs(res_lo) - g) < 1e-5) | (np.abs(np.abs(res_hi) - g) < 1e-5))
    gated = bad | (at_gate & ~used)
    cls = np.full(n, 3, np.int8)
    cls[plane], cls[outside], cls[unsurveyed], cls[used] = 0, 1, 2, 4
    o, a, u, v = (np.asarray(home[q], np.float64) for q in ("o", "a", "u", "v"))
    c0 = o if fault == "tilt_about_c" else o + s0 * a
    q = x[used].astype(np.float64) - c0
    nn, ru = nrm[used], res[used]
    J = -np.stack([nn @ u, nn @ v, (nn * np.cross(v, q)).sum(1), -(nn * np.cross(u, q)).sum(1)], axis=1) if used.any() else np.zeros((0, 4))
    A, gv = J.T @ J, J.T @ ru
    nu = int(used.sum())
    res2 = float(ru @ ru)
    status, step = OK, None
    if nu < 4:
        status = DEGENERATE
    else:
        step = ln.solve(A, gv)
        if step is None or not np.all(np.isfinite(step)):
            status, step = SINGULAR, None
    classes = dict(plane=int(plane.sum()), outside=int(outside.sum()), unsurveyed=int(unsurveyed.sum()), gated=int(gated.sum()), used=nu)
    el = np.asarray(plan["side_element"], np.int64)[side].astype(np.int32)
    return dict(A=A, g=gv, used=nu, res2=res2, step=step, status=status, rms=(np.sqrt(res2 / nu) if nu else np.nan), classes=classes,
                cls=cls, res=np.where(used, res, np.nan), res_lo=np.where(used, res_lo, np.nan), res_hi=np.where(used, res_hi, np.nan),
                cell=cell, element=el, ambiguous=int(amb.sum()))


def update(state, x, s0):
    """The header's update: c0 = c + s0 d + x0 u' + x1 v', the frame turned, c slid back to -c.d = s0."""
    c, d, u, v = (np.asarray(state[k], np.float64) for k in ("o", "a", "u", "v"))
    c0 = (c + s0 * d) + x[0] * u + x[1] * v
    d = d + x[2] * u + x[3] * v
    d = d / np.linalg.norm(d)
    u = u - (u @ d) * d
    u = u / np.linalg.norm(u)
    v = np.cross(d, u)
    return dict(o=c0 - (c0 @ d) * d - s0 * d, a=d, u=u, v=v)


def compose(plan, state):
    """Rm' = [a u v] [d u' v']^T with the home section's columns, tr' = o_f - Rm' c: the (3, 4) pose."""
    rm = np.outer(plan["a"], state["a"]) + np.outer(plan["fu"], state["u"]) + np.outer(plan["fv"], state["v"])
    return np.concatenate([rm, (plan["o_f"] - rm @ state["o"]).reshape(3, 1)], axis=1)


def plan_fields(plan):
    """What one_pass reads of a plan, from locate_plan()'s dict."""
    return dict(side_element=plan["add"]["side_element"], side_anchor=plan["add"]["side_anchor"], side_kind=plan["side_kind"],
                side_axis=plan["side_axis"])


def locate(xyz, labels, plan, grid, n_stations, raws=None, reference=DESIGN, min_count=8, gate=0.25, exact=False, fault=None):
    """The whole call on a plan that is not one straight side (that one is wall_locate_np.locate on the element map).
    Returns wall_locate_np.locate's dict; every pass also holds home, blocks and gate.  exact: nothing is rounded to fp32."""
    state = dict(o=plan["c"], a=plan["d"], u=plan["u"], v=plan["v"])
    s0 = float(plan["s0"])
    pf = plan_fields(plan)
    out = dict(status=OK, passes=0, anchor_station=int(pf["side_anchor"][plan["home"]]), lateral=np.zeros(2), tilt=np.zeros(2), **{"pass": []})
    last = np.nan
    first = blocks(plan, state, rounded=not exact)
    for k in range(3):
        home = state if exact else {q: _f32(state[q]) for q in ("o", "a", "u", "v")}
        blk = blocks(plan, state, rounded=not exact)
        if fault == "side_unmoved":
            blk["side"] = np.array([blk["side"][i] if i == plan["home"] else first["side"][i] for i in range(len(blk["side"]))])
        gk = F(gate * 2.0 ** -k)
        r = one_pass(xyz, labels, home, s0, blk, gk, pf, grid, n_stations, raws if reference == MAP else None, min_count, exact=exact,
                     fault=fault)
        r["home"], r["blocks"], r["gate"] = home, blk, gk
        out["pass"].append(r)
        if r["status"] != OK:
            out["status"] = r["status"]
            break
        state = update(state, r["step"], s0)
        out["lateral"] += r["step"][:2]
        out["tilt"] += r["step"][2:]
        out["passes"] = k + 1
        last = float(np.linalg.norm(r["step"]))
    if out["status"] & FAILED_MASK:
        out["pose"] = np.full((3, 4), np.nan)
        out["lateral"], out["tilt"] = np.full(2, np.nan), np.full(2, np.nan)
    else:
        out["pose"] = compose(plan, state)
        if last > ln.STEP_BOUND:
            out["status"] |= NOT_CONVERGED
    return out


def as_info(t, plan):
    """A twin's locate() in the shape of WallAlignment.locate_points' info dict, for the shared assertions."""
    pf = plan_fields(plan)
    d = dict(status=t["status"], passes=t["passes"], n_points=len(t["pass"][0]["cls"]), anchor_station=t["anchor_station"], pose=t["pose"],
             lateral=t["lateral"], tilt=t["tilt"], n_sides=len(pf["side_element"]), element=pf["side_element"][plan["home"]], **pf)
    d["pass"] = []
    for r in t["pass"]:
        q = {k: r["home"][k].astype(F) for k in ("o", "a", "u", "v")}
        q.update(gate=r["gate"], rms=r["rms"], step=(np.full(4, np.nan) if r["step"] is None else r["step"]),
                 side=r["blocks"]["side"].astype(F), joint_o=r["blocks"]["joint_o"].astype(F), joint_a=r["blocks"]["joint_a"].astype(F), **r["classes"])
        d["pass"].append(q)
    return d


def survey_raws(frames, rule, grid, n_stations_of, bound, elements=None, gate=0.25):
    """The raw cells an alignment holds after adds of `frames` [(cloud, pose)]: per element index a RAW_CELL array, by the
    add's rule with the chains in fp64 (the add's gate; owner by the add's fp32 planes)."""
    import wall_np as wn
    out = {}
    for cloud, pose in frames:
        plan = rule.locate_plan(pose, bound)
        st = dict(o=plan["c"], a=plan["d"], u=plan["u"], v=plan["v"])
        blk = blocks(plan, st)
        pf = plan_fields(plan)
        side = al_np.owner32(cloud, dict(n_sides=len(pf["side_element"]), side_element=list(range(len(pf["side_element"]))),
                                         joint_o=plan["add"]["joint_o"], joint_a=plan["add"]["joint_a"]))
        for k, i in enumerate(pf["side_element"]):
            sel = side == k
            nst = n_stations_of(i)
            r = side_chain(cloud[sel], pf["side_kind"][k], blk["side"][k], pf["side_axis"][k], grid, int(pf["side_anchor"][k]), nst, exact=True)
            ok = r["guard"] & (np.abs(r["e"]) <= float(F(gate)))
            raw = wn.cells_from(np.asarray(r["e"], F)[ok], r["cell"][ok], nst * int(grid["n_sectors"]))
            out[i] = wn.merge_raw(out[i], raw) if i in out else raw
    return out


def assert_passes(info, xyz, labels, plan, grid, n_stations, s0, raws=None, min_count=8, res=None, cell=None, element=None, tol=1e-6,
                  fault=None, exact=False, start=None, log=print):
    """What the GPU test asserts of a locate's pass records, evaluated on the blocks the records REPORT: the owner is
    owner32 of pass 0's planes; the class counts are the twin's in every pass (exactly when the twin counts no ambiguous
    point, within their number otherwise); step and rms lie within tol of the twin's; lateral and tilt are the sums of the
    steps; with `start` (locate_plan()'s dict) the state and every block of a pass are the start's moved by the steps before it,
    to 1e-6; the per-point res of the last pass is bit-equal to the twin's on straight and arc sides and inside the twin's
    atan2f envelope on clothoid sides.  Returns the worst |step - twin|, |rms - twin| seen."""
    pf = plan_fields(plan) if "add" in plan else plan
    failed = bool(info["status"] & FAILED_MASK)
    ran = info["passes"] + (1 if failed else 0)
    worst = [0.0, 0.0]
    state = None if start is None else dict(o=start["c"], a=start["d"], u=start["u"], v=start["v"])
    for k in range(ran):
        rec = info["pass"][k]
        if state is not None:   # the state and every attached block of this pass follow from the start and the steps so far
            want = blocks(start, state)
            for q in ("o", "a", "u", "v"):
                assert np.abs(np.asarray(rec[q], np.float64) - state[q]).max() <= 1e-6, (k, q)
            for q in ("side", "joint_o", "joint_a"):
                assert np.abs(np.asarray(rec[q], np.float64) - want[q]).max(initial=0.0) <= 1e-6, (k, q)
            if k < info["passes"]:
                state = update(state, np.asarray(rec["step"], np.float64), s0)
        home = {q: np.asarray(rec[q], np.float64) for q in ("o", "a", "u", "v")}
        blk = dict(side=rec["side"], joint_o=rec["joint_o"], joint_a=rec["joint_a"])
        last = k == ran - 1
        t = one_pass(xyz, labels, home, s0, blk, rec["gate"], pf, grid, n_stations, raws, min_count,
                     cells=cell if (raws is not None and last) else None, fault=fault, exact=exact)
        amb = t["ambiguous"]
        got = {q: int(rec[q]) for q in CLASSES}
        log(f"pass {k}: {got} twin {t['classes']} ambiguous {amb} step {rec['step']} twin {t['step']}")
        assert sum(got.values()) == len(xyz)
        assert all(abs(got[q] - t["classes"][q]) <= amb for q in CLASSES), (k, got, t["classes"])
        if k == 0 and element is not None:
            assert np.array_equal(element, t["element"])
        if t["step"] is not None and not (failed and last):
            worst[0] = max(worst[0], float(np.abs(np.asarray(rec["step"]) - t["step"]).max()))
            worst[1] = max(worst[1], abs(float(rec["rms"]) - t["rms"]))
            assert worst[0] <= tol and worst[1] <= tol, (k, worst)
        if last and res is not None and len(xyz) and exact:
            both = ~np.isnan(res) & ~np.isnan(t["res"])
            assert np.abs(res[both].astype(np.float64) - t["res"][both]).max(initial=0.0) <= 2e-6
        elif last and res is not None and len(xyz):
            both = ~np.isnan(res) & ~np.isnan(t["res"])
            if amb == 0:
                assert np.array_equal(np.isnan(res), np.isnan(t["res"]))
            kinds = np.asarray(pf["side_kind"])[np.searchsorted(np.asarray(pf["side_element"]), t["element"])]
            plain = both & (kinds != CLOTHOID)
            assert np.array_equal(res[plain].view(np.uint32), t["res"][plain].astype(F).view(np.uint32))
            cl = both & (kinds == CLOTHOID)
            ulp = np.spacing(np.abs(res[cl]).astype(F)).astype(np.float64)
            assert np.all(res[cl] >= t["res_lo"][cl] - ulp) and np.all(res[cl] <= t["res_hi"][cl] + ulp)
    if not failed:
        assert np.allclose(info["lateral"], sum(np.asarray(info["pass"][k]["step"][:2]) for k in range(3)), rtol=0, atol=1e-15)
        assert np.allclose(info["tilt"], sum(np.asarray(info["pass"][k]["step"][2:]) for k in range(3)), rtol=0, atol=1e-15)
    return worst
