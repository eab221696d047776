"""fp64 numpy twin of the wall-map locate (gm_wall_map_locate_*, csrc/k_wall_locate.hip + gm_wall_slot.hip; include/gm_hip.h
states the rule).

one_pass() is one Gauss-Newton pass in fp64 on the fp32 frame a pass REPORTED (as wall_np.points does for the add): the
device runs the per-point chain in fp32 on those rounded vectors and sums in fp64, the twin does all of it in fp64 on the
same vectors, so the two agree to the rounding of a few fp32 operations per point.  A point whose |res| lies within 1e-5 m
of the gate is counted as ambiguous; in MAP mode so is one within wall_np's 1e-3 of a station or sector edge, unless the
device's own cell per point is passed in (cells=).

locate() is the whole chain restated: the start on the host in fp64, three passes, the update and the composed pose.
"""
import numpy as np

import wall_np as wn

DESIGN, MAP = 0, 1
OK, DEGENERATE, SINGULAR, FAILED_MASK, NOT_CONVERGED = 0, 2, 3, 0xFF, 1 << 8
STEP_BOUND = 1e-2
CLASSES = ("plane", "outside", "unsurveyed", "gated", "used")
DEFAULTS = dict(reference=DESIGN, min_count=8, gate=0.25)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def solve(A, g):
    """x = -A^-1 g by the device's Cholesky and pivot rule; None when a pivot fails it."""
    M = np.array(A, np.float64)
    for k in range(4):
        diag = M[k, k]
        piv = diag - float(M[k, :k] @ M[k, :k])
        if not (piv > 1e-12 * diag) or not np.isfinite(piv):
            return None
        M[k, k] = np.sqrt(piv)
        for i in range(k + 1, 4):
            M[i, k] = (M[i, k] - float(M[i, :k] @ M[k, :k])) / M[k, k]
    y = np.zeros(4)
    for i in range(4):
        y[i] = (-g[i] - float(M[i, :i] @ y[:i])) / M[i, i]
    x = np.zeros(4)
    for i in range(3, -1, -1):
        x[i] = (y[i] - float(M[i + 1:, i] @ x[i + 1:])) / M[i, i]
    return x


def mean_q(raw):
    """q = sum / (int64) count by C integer division (toward zero); 0 where count is 0."""
    s = raw["sum"].astype(np.int64).reshape(-1)
    c = np.maximum(raw["count"].astype(np.int64).reshape(-1), 1)
    return np.sign(s) * (np.abs(s) // c)


def one_pass(xyz, labels, frame, gate, raw, min_count, cells=None, p=None, anchor=0):
    """One pass on `frame` (o, a, u, v: the fp32 state the device reported, or any vectors) with the fp32 gate `gate`.
    raw None: DESIGN.  raw (RAW_CELL, any shape): MAP on the map with parameters `p` around the anchor station `anchor`;
    cells: the device's own cell per point (-1: none), which replaces the twin's binning.
    Returns dict(A (4, 4), g (4), used, res2, step (None: degenerate or singular), status, rms, classes (plane, outside,
    unsurveyed, gated, used), cls (per point index into CLASSES), res (per point, NaN unless used), ambiguous)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(x)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    o, a, u, v = (np.asarray(frame[k], np.float64) for k in ("o", "a", "u", "v"))
    R = float(np.float32((p or wn.DEFAULTS)["radius"]))
    g = float(np.float32(gate))
    q = x - o
    t = q @ a
    w = q - t[:, None] * a
    rho = np.sqrt((w * w).sum(1))
    e = rho - R
    plane = lab == 1
    bad = ~plane & ~np.isfinite(e)
    live = ~plane & ~bad
    m = np.zeros(n)
    outside = np.zeros(n, bool)
    unsurveyed = np.zeros(n, bool)
    cell = np.full(n, -1, np.int64)
    amb = np.zeros(n, bool)
    if raw is not None:
        ns, nst = int(p["n_sectors"]), int(p["n_stations"])
        if cells is None:
            ds = float(np.float32(p["station_length"]))
            dth = float(np.float32(2 * np.pi / ns))
            with np.errstate(invalid="ignore"):
                xs = t / ds
                ys = np.mod(np.arctan2(w @ v, w @ u), 2 * np.pi) / dth
                j = anchor + np.floor(np.where(live, xs, 0.0)).astype(np.int64)
                k = np.minimum(np.floor(np.where(live, ys, 0.0)), ns - 1).astype(np.int64)
                amb |= live & ((np.abs(xs - np.rint(xs)) < 1e-3) | (np.abs(ys - np.rint(ys)) < 1e-3))
            inside = live & (j >= 0) & (j < nst)
            cell[inside] = j[inside] * ns + k[inside]
        else:
            cell = np.where(live, np.asarray(cells, np.int64), -1)
        outside = live & (cell < 0)
        has = live & ~outside
        cnt = raw["count"].reshape(-1).astype(np.int64)
        unsurveyed[has] = cnt[cell[has]] < min_count
        ok = has & ~unsurveyed
        m[ok] = mean_q(raw)[cell[ok]].astype(np.float64) * 2.0 ** -20
    at_gate = live & ~outside & ~unsurveyed
    with np.errstate(invalid="ignore"):
        res = e - m
        used = at_gate & (np.abs(res) < g) & (rho > 0)
        amb |= at_gate & (np.abs(np.abs(res) - g) < 1e-5)
    gated = bad | (at_gate & ~used)
    cls = np.full(n, 3, np.int8)
    cls[plane], cls[outside], cls[unsurveyed], cls[used] = 0, 1, 2, 4
    nn = w[used] / rho[used, None]
    a1, a2 = -(nn @ u), -(nn @ v)
    tu, ru = t[used], res[used]
    J = np.stack([a1, a2, tu * a1, tu * a2], axis=1) if used.any() else np.zeros((0, 4))
    A, gv = J.T @ J, J.T @ ru
    nu = int(used.sum())
    res2 = float(ru @ ru)
    status, step = OK, None
    if nu < 4:
        status = DEGENERATE
    else:
        step = solve(A, gv)
        if step is None or not np.all(np.isfinite(step)):
            status, step = SINGULAR, None
    classes = dict(plane=int(plane.sum()), outside=int(outside.sum()), unsurveyed=int(unsurveyed.sum()), gated=int(gated.sum()),
                   used=nu)
    return dict(A=A, g=gv, used=nu, res2=res2, step=step, status=status, rms=(np.sqrt(res2 / nu) if nu else np.nan),
                classes=classes, cls=cls, res=np.where(used, res, np.nan), cell=cell, ambiguous=int(amb.sum()))


def update(state, x, s0):
    """The state (c, d, u, v fp64) moved by the step x."""
    c, d, u, v = (np.asarray(state[k], np.float64) for k in ("o", "a", "u", "v"))
    c = c + x[0] * u + x[1] * v
    d = d + x[2] * u + x[3] * v
    d = d / np.linalg.norm(d)
    u = u - (u @ d) * d
    u = u / np.linalg.norm(u)
    v = np.cross(d, u)
    c = c - (c @ d) * d - s0 * d
    return dict(o=c, a=d, u=u, v=v)


def start(design, p, pose):
    """The start of include/gm_hip.h: (state dict of fp64 o = c, a = d, u, v in sensor coordinates, s0, anchor, o_f)."""
    if not wn.pose_ok(pose):
        raise ValueError("pose refused")
    m = np.asarray(pose, np.float64)[:3]
    rm, tr = m[:, :3], m[:, 3]
    ds = float(p["station_length"])
    jf = np.floor(((tr - design["o"]) @ design["a"] - p["t_min"]) / ds)
    of = design["o"] + (p["t_min"] + jf * ds) * design["a"]
    st = dict(o=rm.T @ (of - tr), a=rm.T @ design["a"], u=rm.T @ design["u"], v=rm.T @ design["v"])
    return st, float(-(st["o"] @ st["a"])), int(jf), of


def compose(design, of, state):
    """Rm' = [a u v] [d u' v']^T, tr' = o_f - Rm' c: the (3, 4) pose."""
    rm = (np.outer(design["a"], state["a"]) + np.outer(design["u"], state["u"]) + np.outer(design["v"], state["v"]))
    return np.concatenate([rm, (of - rm @ state["o"]).reshape(3, 1)], axis=1)


def locate(xyz, labels, p, pose, raw=None, reference=DESIGN, min_count=8, gate=0.25):
    """The whole chain in fp64 (the per-pass state rounded to fp32 once, as the device does).  Returns dict(status, passes,
    pose (3, 4; NaN on failure), lateral, tilt, anchor_station, pass=[one_pass() dicts with frame and gate added])."""
    design = wn.design_frame(p)
    state, s0, anchor, of = start(design, p, pose)
    out = dict(status=OK, passes=0, anchor_station=anchor, lateral=np.zeros(2), tilt=np.zeros(2), **{"pass": []})
    last = np.nan
    for k in range(3):
        frame = {q: _f32(state[q]) for q in ("o", "a", "u", "v")}
        gk = np.float32(gate * 2.0 ** -k)
        r = one_pass(xyz, labels, frame, gk, raw if reference == MAP else None, min_count, p=p, anchor=anchor)
        r["frame"], r["gate"] = frame, gk
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
        out["pose"] = compose(design, of, state)
        if last > STEP_BOUND:
            out["status"] |= NOT_CONVERGED
    return out
