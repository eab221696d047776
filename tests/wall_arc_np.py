"""fp64 numpy twin of the wall map on a circular-arc design axis (gm_wall_map_create_arc; include/gm_hip.h states the rule).

design() is the arc design frame, add_frame() the per-add frame, frame() / project() / point() the host-only companions
(gm_wall_arc_*), all in the header's operation order on Python floats: the library's host code is plain fp64 C without
contraction, so these agree with it to the last bit or two (atan2, cos and sin come from the same libm through math.*).
points() is the per-point chain in fp64 on the frame the library REPORTED (gm_wall_arc_add_frame), with wall_np.points'
ambiguous mask; points_f32() is the same chain in float32, one rounding per operation as the device does it, up to the
class and the cell, with an `uncertain` mask around the one library call (atan2f) it cannot reproduce.
cloud() is gm_wall_map_cloud's records with the arc position rule, byte for byte.
"""
import math

import numpy as np

import fp32_np as fp
import wall_cloud_np as wc
import wall_np as wn

MAPPED, OUTSIDE, BEYOND, PLANE = wn.MAPPED, wn.OUTSIDE, wn.BEYOND, wn.PLANE


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _straight(p):
    """design_frame_of in its own operation order: a, u, v (lists of floats), status."""
    pt, d, up, fw = ([float(x) for x in p[k]] for k in ("point", "direction", "up", "forward"))
    dn = math.sqrt(_dot(d, d))
    s = _dot(d, fw)
    a = [(x if s >= 0.0 else -x) / dn for x in d]
    ua = _dot(up, a)
    u = [up[k] - ua * a[k] for k in range(3)]
    ul, upl = math.sqrt(_dot(u, u)), math.sqrt(_dot(up, up))
    status = wn.SURF_OK
    if ul < 0.1 * upl:
        u, status = [float(x) for x in wn.basis_e1(np.array(a))], wn.SURF_UP_FALLBACK
    else:
        u = [x / ul for x in u]
    return pt, a, u, _cross(a, u), status


def accepted(p, arc):
    """gm_wall_map_create_arc's refusals (the arc's own; p is taken as accepted by gm_wall_map_create)."""
    cv = [float(x) for x in arc["curvature"]]
    s0 = float(arc["point_chainage"])
    if not all(math.isfinite(x) for x in cv + [s0]):
        return False
    _, a, _, _, _ = _straight(p)
    ca = _dot(cv, a)
    c = [cv[k] - ca * a[k] for k in range(3)]
    kappa = math.sqrt(_dot(c, c))
    if not math.isfinite(kappa) or kappa < 1e-6 or (p["radius"] + p["gate"]) * kappa > 0.5:
        return False
    s_end = p["t_min"] + float(p["n_stations"]) * p["station_length"]
    return abs(kappa * (p["t_min"] - s0)) <= 3.0 and abs(kappa * (s_end - s0)) <= 3.0


def design(p, arc):
    """dict(a, u, v, n, b, C (float64 [3]), R, kappa, inv_kappa, s0, un, ub, vn, vb, status)."""
    if not accepted(p, arc):
        raise ValueError("arc refused")
    pt, a, u, v, status = _straight(p)
    cv = [float(x) for x in arc["curvature"]]
    ca = _dot(cv, a)
    c = [cv[k] - ca * a[k] for k in range(3)]
    kappa = math.sqrt(_dot(c, c))
    inv = 1.0 / kappa
    n = [x / kappa for x in c]
    b = _cross(a, n)
    C = [pt[k] + n[k] * inv for k in range(3)]
    d = dict(R=float(p["radius"]), kappa=kappa, inv_kappa=inv, s0=float(arc["point_chainage"]), un=_dot(u, n), ub=_dot(u, b),
             vn=_dot(v, n), vb=_dot(v, b), status=status)
    d.update({k: np.array(x, np.float64) for k, x in (("a", a), ("u", u), ("v", v), ("n", n), ("b", b), ("C", C))})
    return d


def section(D, s):
    """a(s), n(s), P(s) at one chainage."""
    psi = D["kappa"] * (float(s) - D["s0"])
    cp, sp = math.cos(psi), math.sin(psi)
    a_s = D["a"] * cp + D["n"] * sp
    n_s = D["n"] * cp - D["a"] * sp
    return a_s, n_s, D["C"] - n_s * D["inv_kappa"]


def frame(D, s):
    """gm_wall_arc_frame: o, a, u, v at chainage s."""
    a_s, n_s, P = section(D, s)
    return P, a_s, D["un"] * n_s + D["ub"] * D["b"], D["vn"] * n_s + D["vb"] * D["b"]


def project(D, xyz):
    """gm_wall_arc_project on map points [n, 3]: chainage, angle in [0, 2 pi), e."""
    r = np.asarray(xyz, np.float64).reshape(-1, 3) - D["C"]
    xa, xn, zb = (r[:, 0] * D[k][0] + r[:, 1] * D[k][1] + r[:, 2] * D[k][2] for k in ("a", "n", "b"))
    s = D["s0"] + np.arctan2(xa, -xn) / D["kappa"]
    yc = D["inv_kappa"] - np.sqrt(xa * xa + xn * xn)
    e = np.sqrt(yc * yc + zb * zb) - D["R"]
    th = np.arctan2(yc * D["vn"] + zb * D["vb"], yc * D["un"] + zb * D["ub"])
    return s, np.where(th < 0.0, th + 2 * np.pi, th), e


def point(D, s, phi, rho):
    """gm_wall_arc_point: the map points at (chainage, angle, rho), broadcast; [n, 3]."""
    s, phi, rho = (x.reshape(-1) for x in np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(phi, np.float64),
                                                               np.asarray(rho, np.float64)))
    psi = D["kappa"] * (s - D["s0"])
    cp, sp, c, sn = np.cos(psi), np.sin(psi), np.cos(phi), np.sin(phi)
    yc = rho * (c * D["un"] + sn * D["vn"])
    zb = rho * (c * D["ub"] + sn * D["vb"])
    r = yc - D["inv_kappa"]
    nr = D["n"][None, :] * cp[:, None] - D["a"][None, :] * sp[:, None]
    return (D["C"][None, :] + r[:, None] * nr) + zb[:, None] * D["b"][None, :]


def chainage(D, x):
    r = [float(x[k]) - D["C"][k] for k in range(3)]
    return D["s0"] + math.atan2(_dot(r, D["a"]), -_dot(r, D["n"])) / D["kappa"]


_f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)  # noqa: E731


def add_frame(D, p, pose, rounded=True):
    """The per-add frame: dict(anchor, sensor_chainage, anchor_chainage, o, a, n, b, u, v (fp64 values of the fp32
    vectors), kappa, un, ub, vn, vb, R, ds, gate, dtheta (fp64 values of the fp32 constants)).  ValueError on a pose the
    library refuses.  rounded False: the vectors and kappa, un, ub, vn, vb before their rounding."""
    if not wn.pose_ok(pose):
        raise ValueError("pose refused")
    m = np.asarray(pose, np.float64)[:3]
    rm, tr = m[:, :3], m[:, 3]
    ds = float(p["station_length"])
    s = chainage(D, tr)
    jf = math.floor((s - p["t_min"]) / ds)
    sf = p["t_min"] + jf * ds
    a_s, n_s, P = section(D, sf)
    rt = lambda x: np.array([rm[0, c] * x[0] + rm[1, c] * x[1] + rm[2, c] * x[2] for c in range(3)])  # noqa: E731  Rm^T x
    nn, bb = rt(n_s), rt(D["b"])
    _f32 = globals()["_f32"] if rounded else (lambda x: np.asarray(x, np.float64))
    f = dict(anchor=int(jf), sensor_chainage=s, anchor_chainage=sf, o=_f32(rt(P - tr)), a=_f32(rt(a_s)), n=_f32(nn), b=_f32(bb),
             u=_f32(D["un"] * nn + D["ub"] * bb), v=_f32(D["vn"] * nn + D["vb"] * bb))
    for k in ("kappa", "un", "ub", "vn", "vb", "R"):
        f[k] = float(np.float32(D[k])) if rounded or k == "R" else float(D[k])
    f.update(ds=float(np.float32(ds)), gate=float(np.float32(p["gate"])), dtheta=float(np.float32(2 * np.pi / p["n_sectors"])))
    return f


def _frame_fields(f):
    o, a, n, b = (np.asarray(f[k], np.float64) for k in ("o", "a", "n", "b"))
    k, un, ub, vn, vb, R = (float(f[x]) for x in ("kappa", "un", "ub", "vn", "vb", "R"))
    return o, a, n, b, k, un, ub, vn, vb, R, int(f["anchor"] if "anchor" in f else f["anchor_station"])


def points(xyz, labels, f, p, gate=None):
    """Per point in fp64 on the reported frame f (gm_wall_arc_add_frame's dict, or add_frame()'s): e (NaN for plane
    points), t, phi, class, cell (global j * n_sectors + k, -1 unless mapped), ambiguous mask (wall_np.points', plus
    |cy| < 1e-5).  gate: the check's own (None: the map's)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n_pts = len(x)
    lab = np.zeros(n_pts, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    o, a, n, b, k, un, ub, vn, vb, R, anchor = _frame_fields(f)
    ds = float(np.float32(p["station_length"]))
    gate = float(np.float32(p["gate"] if gate is None else gate))
    dth = float(np.float32(2 * np.pi / p["n_sectors"]))
    q = x - o
    xx, y, z = q @ a, q @ n, q @ b
    cx, cy = k * xx, 1.0 - k * y
    d = np.sqrt(cx * cx + cy * cy)
    t = np.arctan2(cx, cy) / k
    yc = (2.0 * y - k * (xx * xx + y * y)) / (1.0 + d)
    e = np.sqrt(yc * yc + z * z) - R
    phi = np.mod(np.arctan2(yc * vn + z * vb, yc * un + z * ub), 2 * np.pi)
    xs, ys = t / ds, phi / dth
    j = anchor + np.floor(xs).astype(np.int64)
    kk = np.minimum(np.floor(ys), p["n_sectors"] - 1).astype(np.int64)
    cls = np.full(n_pts, MAPPED, np.int8)
    plane = lab == 1
    beyond = ~plane & (~(np.abs(e) <= gate) | ~(cy > 0.0))
    outside = ~plane & ~beyond & ~((j >= 0) & (j < p["n_stations"]))
    cls[outside] = OUTSIDE
    cls[beyond] = BEYOND
    cls[plane] = PLANE
    mapped = cls == MAPPED
    cell = np.full(n_pts, -1, np.int64)
    cell[mapped] = j[mapped] * p["n_sectors"] + kk[mapped]
    amb = ~plane & ((np.abs(xs - np.rint(xs)) < 1e-3) | (np.abs(ys - np.rint(ys)) < 1e-3) |
                    (np.abs(np.abs(e) - gate) < 1e-5) | (np.abs(cy) < 1e-5))
    return dict(e=np.where(plane, np.nan, e), t=t, phi=phi, cls=cls, cell=cell, ambiguous=amb, yc=yc, z=z)


F = np.float32
ATAN2_ULPS = 6                       # OpenCL's bound for atan2 in single precision, which the device library's atan2f is built to
SHIFTS = tuple([0] + [d for d in range(-ATAN2_ULPS, ATAN2_ULPS + 1) if d])   # the nominal angle first
fma = fp.fma32                       # the twins' fused multiply-add (the sensitivity test swaps it for the old double rounding)
GUARD_CY = True                      # the cy > 0 test of both curved chains (the sensitivity test drops it)


def atan2_f32(y, x):
    """atan2 taken in fp64 and rounded to fp32 once: the one operation of the chains a twin cannot reproduce, because the
    device's atan2f is a library call."""
    with np.errstate(all="ignore"):
        return np.arctan2(np.asarray(y, F).astype(np.float64), np.asarray(x, F).astype(np.float64)).astype(F)


def _frame_consts(f, p, gate):
    """(anchor, ds, gate, dtheta, two_pi, n_stations, n_sectors) of a reported frame or of add_frame()'s; gate: the
    check's own (None: the frame's, which is the map's)."""
    anchor = int(f["anchor"] if "anchor" in f else f["anchor_station"])
    ds = F(f["ds"] if "ds" in f else f["station_length"])
    dth = F(f["dtheta"] if "dtheta" in f else f["sector_angle"])
    return anchor, ds, F(f["gate"] if gate is None else gate), dth, F(2 * np.pi), int(p["n_stations"]), int(p["n_sectors"])


def sector_f32(yc, z, f, dth, two_pi, nsec, shift=0):
    """arc_sector's operations, the angle moved by `shift` fp32 ulps: k as int64."""
    un, ub, vn, vb = (F(f[k]) for k in ("un", "ub", "vn", "vb"))
    with np.errstate(all="ignore"):
        th = fp.ulp_steps(atan2_f32(fma(yc, vn, z * vb), fma(yc, un, z * ub)), shift)
        phi = np.where(th < F(0.0), th + two_pi, th).astype(F)
        kf = np.floor(phi / dth)
    return np.minimum(np.where(np.isfinite(kf), kf, 0.0).astype(np.int64), nsec - 1)


def bin_f32(variants, f, p, labels, gate, shifts=None):
    """The rest of wall_chain after the residual, in float32: class (plane, gate-or-guard, range, then sector), jl by
    surf_station's operations (floor((t - 0) / ds)), the |jl| < 4e18 rule of wall_station, the sector by arc_sector's
    operations and the global cell.  variants: (e, ok, t, yc, z) float32 arrays per point, the nominal chain first and then
    the chains whose atan2f was moved by the other SHIFTS; every one is binned with the sector's own angle moved by every
    shift as well.  Returns dict(cls, cell, jl of the nominal variant, uncertain: a point that is not plane and whose
    class or cell differs from the nominal in any of those combinations)."""
    anchor, ds, gate, dth, two_pi, nst, nsec = _frame_consts(f, p, gate)
    n_pts = len(variants[0][0])
    plane = (np.zeros(n_pts, np.uint8) if labels is None else np.asarray(labels, np.uint8)) == 1
    first, uncertain = None, np.zeros(n_pts, bool)
    for e, ok, t, yc, z in variants:
        with np.errstate(all="ignore"):
            beyond = ~(np.abs(e) <= gate) | ~ok
            jl = np.floor(((t - F(0.0)) / ds).astype(F)).astype(F)
            fin = np.abs(jl) < F(4.0e18)
        j = anchor + np.where(fin, jl, F(0.0)).astype(np.int64)
        inr = fin & (j >= 0) & (j < nst)
        cls = np.where(plane, PLANE, np.where(beyond, BEYOND, np.where(inr, MAPPED, OUTSIDE))).astype(np.int8)
        for d in (SHIFTS if shifts is None else shifts):
            cell = np.where(cls == MAPPED, j * nsec + sector_f32(yc, z, f, dth, two_pi, nsec, d), -1)
            if first is None:
                first = dict(cls=cls, cell=cell, jl=jl)
            else:
                uncertain |= ~plane & ((cls != first["cls"]) | (cell != first["cell"]))
    first["uncertain"] = uncertain
    return first


def class_counts(r, keep=None):
    """(mapped, outside, beyond_gate, plane) of a twin's classes over the points of `keep` (all)."""
    c = r["cls"] if keep is None else r["cls"][keep]
    return tuple(int((c == k).sum()) for k in (MAPPED, OUTSIDE, BEYOND, PLANE))


def points_f32(xyz, f, labels=None, p=None, gate=None, shifts=None):
    """The device's chain in float32, operation by operation (numpy rounds each float32 operation to nearest; fma is
    fp32_np.fma32, rounded once): e, t, yc, z, cy as float32.  e, yc, z and cy do not depend on atan2f at all.

    With the map's parameters p it is the whole of wall_chain and returns what points() returns: e (NaN for plane
    points), cls, cell, jl, and `uncertain` in the place of `ambiguous`.  atan2f is taken in fp64 and rounded once, and
    whatever an angle decides is recomputed with that angle moved by -6 .. +6 fp32 ulps (bin_f32).  That the device's
    atan2f lies within 6 ulps of the true angle is an ASSUMPTION: it is OpenCL's bound for atan2, which the device
    library follows; nothing in this project measures it.  uncertain is built from the twin alone.  shifts: the ulps the
    angles are moved by, the nominal 0 first (SHIFTS; (0,) for the nominal chain alone, with an empty mask)."""
    x = np.asarray(xyz, F).reshape(-1, 3)
    o, a, n, b = (np.asarray(f[k], F) for k in ("o", "a", "n", "b"))
    k, R = F(f["kappa"]), F(f["R"])
    with np.errstate(all="ignore"):
        q = x - o
        dot3 = lambda w: fma(q[:, 0], w[0], fma(q[:, 1], w[1], q[:, 2] * w[2]))  # noqa: E731
        xx, y, z = dot3(a), dot3(n), dot3(b)
        cx = k * xx
        cy = fma(-k, y, F(1.0))
        d = np.sqrt(fma(cx, cx, cy * cy))
        th = atan2_f32(cx, cy)
        t = (th / k).astype(F)
        h = fma(xx, xx, y * y)
        yc = (fma(-k, h, y + y) / (F(1.0) + d)).astype(F)
        e = (np.sqrt(fma(yc, yc, z * z)) - R).astype(F)
        out = dict(e=e, t=t, yc=yc, z=z, cy=cy)
        if p is None:
            return out
        ok = (cy > F(0.0)) if GUARD_CY else np.ones(len(x), bool)
        shifts = SHIFTS if shifts is None else shifts
        out.update(bin_f32([(e, ok, (fp.ulp_steps(th, s) / k).astype(F), yc, z) for s in shifts], f, p, labels, gate, shifts))
    out["e"] = np.where(out["cls"] == PLANE, F(np.nan), e)
    return out


def row_angles(D, p, station0, n, bs):
    """(cos psi, sin psi) [NJ, 2] of the block rows' centre chainages, as the library's host computes them."""
    bs = min(int(bs), max(n, 1))
    out = np.empty((-(-n // bs), 2), np.float64)
    for J in range(len(out)):
        j0 = station0 + J * bs
        ns = min(bs, station0 + n - j0)
        tc = p["t_min"] + (float(2 * j0 + ns) * 0.5) * p["station_length"]
        psi = D["kappa"] * (tc - D["s0"])
        out[J] = (math.cos(psi), math.sin(psi))
    return out


def cloud(raw, p, arc, station0=0, n=None, directions=None, **params):
    """gm_wall_map_cloud on an arc map: wall_cloud_np.cloud's info and records with the arc position rule."""
    D = design(p, arc)
    info, out = wc.cloud(raw, p, station0=station0, n=n, directions=directions, **params)
    if not len(out):
        return info, out
    prm = dict(wc.DEFAULTS)
    prm.update(params)
    n = info["n_stations"]
    bs, _, _, NK = wc.grid(n, info["n_sectors"], prm["block_stations"], prm["block_sectors"])
    J, K = out["block"].astype(np.int64) // NK, out["block"].astype(np.int64) % NK
    # (the fp64 mean again: the record holds its rounding)
    m = wc.merge_blocks(raw[station0:station0 + n], bs, prm["block_sectors"]).reshape(-1)[out["block"]]
    mean = (m["sum"].astype(np.float64) * np.float64(2.0 ** -20)) / m["count"].astype(np.float64)
    rho = np.float64(D["R"]) + np.float64(prm["exaggeration"]) * mean
    tab = np.asarray(directions, np.float64)
    c, s = tab[K, 0], tab[K, 1]
    rows = row_angles(D, p, station0, n, bs)
    cp, sp = rows[J, 0], rows[J, 1]
    yc = rho * (c * D["un"] + s * D["vn"])
    zb = rho * (c * D["ub"] + s * D["vb"])
    r = yc - D["inv_kappa"]
    anchor = np.asarray(prm["anchor"], np.float64)
    for i, fld in enumerate("xyz"):
        nr = D["n"][i] * cp - D["a"][i] * sp
        q = ((D["C"][i] - anchor[i]) + r * nr) + zb * D["b"][i]
        out[fld] = q.astype(np.float32)
    return info, out
