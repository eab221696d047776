"""numpy twin of the wall map on a clothoid design axis (gm_wall_map_create_clothoid; include/gm_hip.h states the rule).

design() is the clothoid design frame with its table of station starts, xy() / section() / frame() / chainage() /
project() / point() the host-only companions (gm_wall_clothoid_*) in fp64, add_frame() the per-add frame.  points() is
the per-point chain in fp64 on the frame the library REPORTED (gm_wall_clothoid_add_frame): the foot of the
perpendicular converged by eight Newton steps on a 16-node quadrature, with wall_np.points' ambiguous mask;
points_f32() is the device's chain in float32, one rounding per operation, up to the class and the cell, with an
`uncertain` mask and an envelope of e around the one library call (atan2f) it cannot reproduce.  cloud() is
gm_wall_map_cloud's records with the clothoid position rule.
"""
import math

import numpy as np

import fp32_np as fp
import wall_arc_np as wa
import wall_cloud_np as wc
import wall_np as wn

MAPPED, OUTSIDE, BEYOND, PLANE = wn.MAPPED, wn.OUTSIDE, wn.BEYOND, wn.PLANE
HOST_NEWTON = 6          # GM_WALL_CLOTHOID_HOST_STEPS
DEVICE_NEWTON = 2        # GM_WALL_CLOTHOID_STEPS
G_BOUND = 2.0 ** -14     # GM_WALL_CLOTHOID_G_BOUND: the final |g| a mapped point may have (test_wall_clothoid_np measures it)
MIN_DEN = 0.25
GL8_X, GL8_W = np.polynomial.legendre.leggauss(8)
# the device's 4-node rule on [0, 1], as fp32 constants
GL4_C = np.array([0.06943184420297371, 0.33000947820757187, 0.6699905217924281, 0.9305681557970262], np.float32)
GL4_W = np.array([0.17392742256872692, 0.32607257743127305, 0.32607257743127305, 0.17392742256872692], np.float32)

_dot, _cross, _straight, _f32 = wa._dot, wa._cross, wa._straight, wa._f32


def _psi(D, tau):
    return tau * (D["k0"] + (0.5 * D["rate"]) * tau)


def _kap(D, tau):
    return D["k0"] + D["rate"] * tau


def _panels(D, ta, tb):
    return 1 + int(min(max(abs(_kap(D, ta)), abs(_kap(D, tb))) * abs(tb - ta) / 0.25, 4095.0))


def _integrate(D, ta, tb):
    """(X, Y) of the integral of (cos psi, sin psi) from ta to tb: the library's panels of the 8-node rule, scalar."""
    K = _panels(D, ta, tb)
    w = (tb - ta) / K
    h = 0.5 * w
    X = Y = 0.0
    for q in range(K):
        m = ta + (q + 0.5) * w
        sx = sy = 0.0
        for i in range(8):
            ps = _psi(D, m + h * GL8_X[i])
            sx += GL8_W[i] * math.cos(ps)
            sy += GL8_W[i] * math.sin(ps)
        X += h * sx
        Y += h * sy
    return X, Y


def accepted(p, cl):
    """gm_wall_map_create_clothoid's refusals (the clothoid's own; p is taken as accepted by gm_wall_map_create)."""
    nv = [float(x) for x in cl["normal"]]
    k0, c, s0 = float(cl["curvature"]), float(cl["rate"]), float(cl["point_chainage"])
    if not all(math.isfinite(x) for x in nv + [k0, c, s0]):
        return False
    _, a, _, _, _ = _straight(p)
    na = _dot(nv, a)
    n = [nv[k] - na * a[k] for k in range(3)]
    ln, l0 = math.sqrt(_dot(n, n)), math.sqrt(_dot(nv, nv))
    if not math.isfinite(ln) or not ln > 1e-6 * l0 or not ln > 0.0:
        return False
    L = float(p["n_stations"]) * p["station_length"]
    if abs(c) * L < 1e-6:
        return False
    t0 = p["t_min"] - s0
    t1 = t0 + L
    kmax = max(abs(k0 + c * t0), abs(k0 + c * t1))
    if not (p["radius"] + p["gate"]) * kmax <= 0.5:
        return False
    D = dict(k0=k0, rate=c)
    ends = [t0, t1]
    tz = -k0 / c
    if t0 < tz < t1:
        ends.append(tz)
    return all(abs(_psi(D, t)) <= 3.0 for t in ends)


def design(p, cl):
    """dict(pt, a, u, v, n, b (float64 [3]), R, k0, rate, s0, tau0, ds, nst, tab [nst + 1, 2], un, ub, vn, vb, status)."""
    if not accepted(p, cl):
        raise ValueError("clothoid refused")
    pt, a, u, v, status = _straight(p)
    nv = [float(x) for x in cl["normal"]]
    na = _dot(nv, a)
    n = [nv[k] - na * a[k] for k in range(3)]
    ln = math.sqrt(_dot(n, n))
    n = [x / ln for x in n]
    b = _cross(a, n)
    D = dict(R=float(p["radius"]), k0=float(cl["curvature"]), rate=float(cl["rate"]), s0=float(cl["point_chainage"]),
             un=_dot(u, n), ub=_dot(u, b), vn=_dot(v, n), vb=_dot(v, b), status=status, ds=float(p["station_length"]),
             nst=int(p["n_stations"]))
    D["tau0"] = float(p["t_min"]) - D["s0"]
    D.update({k: np.array(x, np.float64) for k, x in (("pt", pt), ("a", a), ("u", u), ("v", v), ("n", n), ("b", b))})
    tab = np.empty((D["nst"] + 1, 2), np.float64)
    tab[0] = _integrate(D, 0.0, D["tau0"])
    for j in range(D["nst"]):
        dx, dy = _integrate(D, D["tau0"] + j * D["ds"], D["tau0"] + (j + 1) * D["ds"])
        tab[j + 1] = (tab[j, 0] + dx, tab[j, 1] + dy)
    D["tab"] = tab
    return D


def xy(D, tau):
    """(X, Y) at one tau = s - s0: the table entry of the station start at or below it, plus the panels from there."""
    jd = min(max(math.floor((tau - D["tau0"]) / D["ds"]), 0), D["nst"])
    dx, dy = _integrate(D, D["tau0"] + jd * D["ds"], tau)
    return D["tab"][jd, 0] + dx, D["tab"][jd, 1] + dy


def section(D, s):
    """a(s), n(s), P(s) and the signed curvature at one chainage."""
    return _section_tau(D, float(s) - D["s0"])


def _section_tau(D, tau):
    ps = _psi(D, tau)
    cp, sp = math.cos(ps), math.sin(ps)
    X, Y = xy(D, tau)
    return D["a"] * cp + D["n"] * sp, D["n"] * cp - D["a"] * sp, (D["pt"] + X * D["a"]) + Y * D["n"], _kap(D, tau)


def frame(D, s):
    """gm_wall_clothoid_frame: o, a, u, v and the signed curvature at chainage s."""
    a_s, n_s, P, k = section(D, s)
    return P, a_s, D["un"] * n_s + D["ub"] * D["b"], D["vn"] * n_s + D["vb"] * D["b"], k


def _foot(D, xa, xn):
    """tau of the foot of the perpendicular of the planar point (xa, xn), and the final (g, yc)."""
    d2 = (xa - D["tab"][:, 0]) ** 2 + (xn - D["tab"][:, 1]) ** 2
    tau = D["tau0"] + int(np.argmin(d2)) * D["ds"]
    for it in range(HOST_NEWTON + 1):
        X, Y = xy(D, tau)
        ps = _psi(D, tau)
        c, s = math.cos(ps), math.sin(ps)
        dx, dy = xa - X, xn - Y
        g = dx * c + dy * s
        yc = dy * c - dx * s
        if it < HOST_NEWTON:
            tau = tau + g / (1.0 - _kap(D, tau) * yc)
    return tau, g, yc


def chainage(D, x):
    r = [float(x[k]) - D["pt"][k] for k in range(3)]
    return D["s0"] + _foot(D, _dot(r, D["a"]), _dot(r, D["n"]))[0]


def project(D, xyz):
    """gm_wall_clothoid_project on map points [n, 3]: chainage, angle in [0, 2 pi), e, and the final |g|."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    s, phi, e, gs = (np.empty(len(x)) for _ in range(4))
    for i, q in enumerate(x):
        r = q - D["pt"]
        tau, g, yc = _foot(D, _dot(r, D["a"]), _dot(r, D["n"]))
        zb = _dot(r, D["b"])
        th = math.atan2(yc * D["vn"] + zb * D["vb"], yc * D["un"] + zb * D["ub"])
        s[i], phi[i], e[i], gs[i] = D["s0"] + tau, th + 2 * math.pi if th < 0.0 else th, math.sqrt(yc * yc + zb * zb) - D["R"], abs(g)
    return s, phi, e, gs


def point(D, s, phi, rho):
    """gm_wall_clothoid_point: the map points at (chainage, angle, rho), broadcast; [n, 3]."""
    s, phi, rho = (x.reshape(-1) for x in np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(phi, np.float64),
                                                               np.asarray(rho, np.float64)))
    out = np.empty((len(s), 3), np.float64)
    for i in range(len(s)):
        _, n_s, P, _ = section(D, s[i])
        c, sn = math.cos(phi[i]), math.sin(phi[i])
        yc = rho[i] * (c * D["un"] + sn * D["vn"])
        zb = rho[i] * (c * D["ub"] + sn * D["vb"])
        out[i] = (P + yc * n_s) + zb * D["b"]
    return out


def add_frame(D, p, pose):
    """The per-add frame: dict(anchor, sensor_chainage, anchor_chainage, o, a, n, b, u, v (fp64 values of the fp32
    vectors), kappa, rate, un, ub, vn, vb, R, ds, gate, dtheta (fp64 values of the fp32 constants)).  ValueError on a pose
    the library refuses."""
    if not wn.pose_ok(pose):
        raise ValueError("pose refused")
    m = np.asarray(pose, np.float64)[:3]
    rm, tr = m[:, :3], m[:, 3]
    ds = float(p["station_length"])
    r = [float(tr[k]) - D["pt"][k] for k in range(3)]
    tau = _foot(D, _dot(r, D["a"]), _dot(r, D["n"]))[0]
    s = D["s0"] + tau
    jf = math.floor((tau - D["tau0"]) / ds)
    sf = p["t_min"] + jf * ds
    a_s, n_s, P, kf = _section_tau(D, D["tau0"] + jf * ds)
    rt = lambda x: np.array([rm[0, c] * x[0] + rm[1, c] * x[1] + rm[2, c] * x[2] for c in range(3)])  # noqa: E731  Rm^T x
    nn, bb = rt(n_s), rt(D["b"])
    f = dict(anchor=int(jf), sensor_chainage=s, anchor_chainage=sf, o=_f32(rt(P - tr)), a=_f32(rt(a_s)), n=_f32(nn), b=_f32(bb),
             u=_f32(D["un"] * nn + D["ub"] * bb), v=_f32(D["vn"] * nn + D["vb"] * bb), kappa=float(np.float32(kf)))
    for k in ("rate", "un", "ub", "vn", "vb", "R"):
        f[k] = float(np.float32(D[k]))
    f.update(ds=float(np.float32(ds)), gate=float(np.float32(p["gate"])), dtheta=float(np.float32(2 * np.pi / p["n_sectors"])))
    return f


def _frame_fields(f):
    o, a, n, b = (np.asarray(f[k], np.float64) for k in ("o", "a", "n", "b"))
    k, c, un, ub, vn, vb, R = (float(f[x]) for x in ("kappa", "rate", "un", "ub", "vn", "vb", "R"))
    return o, a, n, b, k, c, un, ub, vn, vb, R, int(f["anchor"] if "anchor" in f else f["anchor_station"])


_GL16 = np.polynomial.legendre.leggauss(16)


def _eval64(xx, y, k, c, t):
    """X, Y by a 16-node rule on [0, t] (the phase stays below a few radians within a frame's reach), then g, yc, psi."""
    sg = t[:, None] * (0.5 + 0.5 * _GL16[0][None, :])
    ps = (k + 0.5 * c * sg) * sg
    X, Y = 0.5 * t * (np.cos(ps) @ _GL16[1]), 0.5 * t * (np.sin(ps) @ _GL16[1])
    psi = (k + 0.5 * c * t) * t
    cs, sn = np.cos(psi), np.sin(psi)
    dx, dy = xx - X, y - Y
    return dx * cs + dy * sn, dy * cs - dx * sn


def _start(xx, y, k):
    """t0 and cy of the start: the arc chain's t with kappa_f, or x where |kappa_f| < 1e-6."""
    cy = 1.0 - k * y
    if abs(k) < 1e-6:
        return xx.copy(), cy
    return np.arctan2(k * xx, cy) / k, cy


def points(xyz, labels, f, p, gate=None):
    """Per point in fp64 on the reported frame f (gm_wall_clothoid_add_frame's dict, or add_frame()'s): e (NaN for plane
    points), t, phi, class, cell (global j * n_sectors + k, -1 unless mapped), ambiguous mask (wall_np.points', plus a
    start or a Newton denominator within 1e-3 of its limit), the final |g|."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n_pts = len(x)
    lab = np.zeros(n_pts, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    o, a, n, b, k, c, un, ub, vn, vb, R, anchor = _frame_fields(f)
    ds = float(np.float32(p["station_length"]))
    gate = float(np.float32(p["gate"] if gate is None else gate))
    dth = float(np.float32(2 * np.pi / p["n_sectors"]))
    q = x - o
    xx, y, z = q @ a, q @ n, q @ b
    t, cy = _start(xx, y, k)
    den_min = np.full(n_pts, np.inf)
    with np.errstate(all="ignore"):
        for it in range(8):
            g, yc = _eval64(xx, y, k, c, t)
            den = 1.0 - (k + c * t) * yc
            if it < DEVICE_NEWTON:
                den_min = np.minimum(den_min, den)
            t = t + g / den
        g, yc = _eval64(xx, y, k, c, t)
        e = np.sqrt(yc * yc + z * z) - R
        phi = np.mod(np.arctan2(yc * vn + z * vb, yc * un + z * ub), 2 * np.pi)
        xs, ys = t / ds, phi / dth
        fin = np.isfinite(xs) & (np.abs(xs) < 4.0e18)
        j = anchor + np.floor(np.where(fin, xs, 0.0)).astype(np.int64)
        kk = np.minimum(np.floor(np.where(np.isfinite(ys), ys, 0.0)), p["n_sectors"] - 1).astype(np.int64)
        cls = np.full(n_pts, MAPPED, np.int8)
        plane = lab == 1
        beyond = ~plane & (~(np.abs(e) <= gate) | ~(cy > 0.0) | ~(den_min > MIN_DEN) | ~np.isfinite(t) | ~(np.abs(g) <= G_BOUND))
        outside = ~plane & ~beyond & ~(fin & (j >= 0) & (j < p["n_stations"]))
        cls[outside] = OUTSIDE
        cls[beyond] = BEYOND
        cls[plane] = PLANE
        mapped = cls == MAPPED
        cell = np.full(n_pts, -1, np.int64)
        cell[mapped] = j[mapped] * p["n_sectors"] + kk[mapped]
        amb = ~plane & ((np.abs(xs - np.rint(xs)) < 1e-3) | (np.abs(ys - np.rint(ys)) < 1e-3) |
                        (np.abs(np.abs(e) - gate) < 1e-5) | (np.abs(cy) < 1e-5) | (np.abs(den_min - MIN_DEN) < 1e-3))
    return dict(e=np.where(plane, np.nan, e), t=t, phi=phi, cls=cls, cell=cell, ambiguous=amb, yc=yc, z=z, g=np.abs(g))


F = np.float32
# the header's sincos rule: pi / 2 in three terms, the sine's and the cosine's polynomial (highest power first)
PIO2 = np.array([1.5703125, 4.837512969970703125e-4, 7.54978995489188216e-8], F)
SIN_C = np.array([-1.9515295891e-4, 8.3321608736e-3, -1.6666654611e-1], F)
COS_C = np.array([2.443315711809948e-5, -1.388731625493765e-3, 4.166664568298827e-2], F)
GUARD_DEN = True                     # the den > 0.25 test (the sensitivity test drops it; the cy > 0 test is wall_arc_np.GUARD_CY)
GUARD_G = True                       # the closing tests: t finite and |g| <= G_BOUND (tests/test_wall_stray_np.py drops them)


def sincos_f32(ps):
    """The header's sincos rule, operation by operation: (sin, cos) as float32, NaN for |ps| >= 2^20 or a NaN."""
    fma = wa.fma
    ps = np.asarray(ps, F)
    with np.errstate(all="ignore"):
        fin = np.abs(ps) < F(1048576.0)
        k = np.where(fin, np.rint(ps * F(0.63661977236758134)), F(0.0)).astype(F)
        r = fma(-k, PIO2[0], ps)
        r = fma(-k, PIO2[1], r)
        r = fma(-k, PIO2[2], r)
        z = r * r
        sp = fma(fma(SIN_C[0], z, SIN_C[1]), z, SIN_C[2])
        sv = fma(sp * z, r, r)
        cp = fma(fma(COS_C[0], z, COS_C[1]), z, COS_C[2])
        cv = (fma(cp * z, z, F(-0.5) * z) + F(1.0)).astype(F)
        q = k.astype(np.int64) & 3
    s1, c1 = np.where(q & 1, cv, sv), np.where(q & 1, sv, cv)
    sn = np.where(fin, np.where(q & 2, -s1, s1), F(np.nan)).astype(F)
    cs = np.where(fin, np.where((q + 1) & 2, -c1, c1), F(np.nan)).astype(F)
    return sn, cs


def _eval_f32(xx, y, k, hr, t):
    """E(t) of the header: g and yc of the trial t."""
    fma = wa.fma
    sx = sy = None
    for i in range(4):
        sg = t * GL4_C[i]
        sn, cs = sincos_f32(fma(hr, sg, k) * sg)
        sx = GL4_W[i] * cs if sx is None else fma(cs, GL4_W[i], sx)
        sy = GL4_W[i] * sn if sy is None else fma(sn, GL4_W[i], sy)
    dx, dy = xx - t * sx, y - t * sy
    sn, cs = sincos_f32(fma(hr, t, k) * t)
    return fma(dx, cs, dy * sn), fma(dy, cs, -(dx * sn))


def _newton_f32(xx, y, z, k, c, R, t):
    """The DEVICE_NEWTON steps from the start t and the closing evaluation: e, t, yc, g, the two denominators [2, n]."""
    fma = wa.fma
    hr = F(0.5) * c
    dens = []
    for _ in range(DEVICE_NEWTON):
        g, yc = _eval_f32(xx, y, k, hr, t)
        den = fma(-fma(t, c, k), yc, F(1.0))
        dens.append(den)
        t = (t + (g / den).astype(F)).astype(F)
    g, yc = _eval_f32(xx, y, k, hr, t)
    e = (np.sqrt(fma(yc, yc, z * z)) - R).astype(F)
    return e, t, yc, g, np.array(dens, F).reshape(DEVICE_NEWTON, -1)


def points_f32(xyz, f, labels=None, p=None, gate=None, shifts=None):
    """The device's chain in float32, operation by operation (numpy rounds each float32 operation to nearest; fma is
    fp32_np.fma32, rounded once; sin and cos follow the header's own rule): e, t, yc, z, the final g, the smaller of the
    Newton denominators (den) and each of them (dens [steps, n]), cy, and tangent: whether the frame takes the tangent start
    (|kappa_f| < 1e-6).  On such a frame nothing up to the station depends on atan2f; on the others the osculating-arc
    start does, through t0 = atan2f(kappa_f x, cy) / kappa_f, which is taken in fp64 and rounded once.

    With the map's parameters p it is the whole of wall_chain and returns what points() returns: e (NaN for plane
    points), cls, cell, jl, `uncertain` in the place of `ambiguous` (wall_arc_np.bin_f32: the class or the cell changes
    when the start's or the sector's angle is moved by -6 .. +6 fp32 ulps -- an ASSUMPTION about the device's atan2f, see
    wall_arc_np.points_f32, also for `shifts`), e_lo / e_hi: per point the lowest and the highest e over the thirteen starts
    (both e on a tangent-start frame), and e_mixed: some of the starts give a NaN e and some do not."""
    fma = wa.fma
    x = np.asarray(xyz, F).reshape(-1, 3)
    o, a, n, b = (np.asarray(f[k], F) for k in ("o", "a", "n", "b"))
    k, c, R = F(f["kappa"]), F(f["rate"]), F(f["R"])
    tangent = bool(abs(k) < F(1.0e-6))
    with np.errstate(all="ignore"):
        q = x - o
        dot3 = lambda w: fma(q[:, 0], w[0], fma(q[:, 1], w[1], q[:, 2] * w[2]))  # noqa: E731
        xx, y, z = dot3(a), dot3(n), dot3(b)
        cy = fma(-k, y, F(1.0))
        th = None if tangent else wa.atan2_f32(k * xx, cy)
        t0 = xx.copy() if tangent else (th / k).astype(F)
        e, t, yc, g, dens = _newton_f32(xx, y, z, k, c, R, t0)
        den_min = np.minimum.reduce(dens, axis=0) if DEVICE_NEWTON else np.full(len(x), np.inf, F)
        out = dict(e=e, t=t, yc=yc, z=z, g=g, den=den_min, dens=dens, cy=cy, tangent=tangent)
        if p is None:
            return out

        def ok_of(t, g, dens):
            good = (cy > F(0.0)) if wa.GUARD_CY else np.ones(len(x), bool)
            if GUARD_DEN:
                good = good & np.all(dens > F(MIN_DEN), axis=0)
            return good & (np.abs(t) < F(np.inf)) & (np.abs(g) <= F(G_BOUND)) if GUARD_G else good

        variants = [(e, ok_of(t, g, dens), t, yc, z)]
        shifts = wa.SHIFTS if shifts is None else shifts
        for s in (() if tangent else shifts[1:]):
            ev, tv, ycv, gv, dv = _newton_f32(xx, y, z, k, c, R, (fp.ulp_steps(th, s) / k).astype(F))
            variants.append((ev, ok_of(tv, gv, dv), tv, ycv, z))
        out.update(wa.bin_f32(variants, f, p, labels, gate, shifts))
        es = np.array([v[0] for v in variants], F)
        nan = np.isnan(es)
        out["e_mixed"] = nan.any(axis=0) & ~nan.all(axis=0)
        out["e_lo"] = np.where(nan.any(axis=0), F(np.nan), np.min(np.where(nan, F(np.inf), es), axis=0))
        out["e_hi"] = np.where(nan.any(axis=0), F(np.nan), np.max(np.where(nan, F(-np.inf), es), axis=0))
    out["e"] = np.where(out["cls"] == PLANE, F(np.nan), e)
    return out


def row_table(D, p, station0, n, bs, anchor):
    """(P(tc) - anchor, cos psi, sin psi) [NJ, 5] of the block rows' centre chainages, as the library's host computes them."""
    bs = min(int(bs), max(n, 1))
    out = np.empty((-(-n // bs), 5), np.float64)
    for J in range(len(out)):
        j0 = station0 + J * bs
        ns = min(bs, station0 + n - j0)
        tc = p["t_min"] + (float(2 * j0 + ns) * 0.5) * p["station_length"]
        tau = tc - D["s0"]
        X, Y = xy(D, tau)
        ps = _psi(D, tau)
        out[J, :3] = ((D["pt"] + X * D["a"]) + Y * D["n"]) - np.asarray(anchor, np.float64)
        out[J, 3:] = (math.cos(ps), math.sin(ps))
    return out


def cloud(raw, p, cl, station0=0, n=None, directions=None, **params):
    """gm_wall_map_cloud on a clothoid map: wall_cloud_np.cloud's info and records with the clothoid position rule."""
    D = design(p, cl)
    info, out = wc.cloud(raw, p, station0=station0, n=n, directions=directions, **params)
    if not len(out):
        return info, out
    prm = dict(wc.DEFAULTS)
    prm.update(params)
    n = info["n_stations"]
    bs, _, _, NK = wc.grid(n, info["n_sectors"], prm["block_stations"], prm["block_sectors"])
    J, K = out["block"].astype(np.int64) // NK, out["block"].astype(np.int64) % NK
    m = wc.merge_blocks(raw[station0:station0 + n], bs, prm["block_sectors"]).reshape(-1)[out["block"]]
    mean = (m["sum"].astype(np.float64) * np.float64(2.0 ** -20)) / m["count"].astype(np.float64)
    rho = np.float64(D["R"]) + np.float64(prm["exaggeration"]) * mean
    tab = np.asarray(directions, np.float64)
    c, s = tab[K, 0], tab[K, 1]
    rows = row_table(D, p, station0, n, bs, prm["anchor"])
    cp, sp = rows[J, 3], rows[J, 4]
    yc = rho * (c * D["un"] + s * D["vn"])
    zb = rho * (c * D["ub"] + s * D["vb"])
    for i, fld in enumerate("xyz"):
        nr = D["n"][i] * cp - D["a"][i] * sp
        q = (rows[J, i] + yc * nr) + zb * D["b"][i]
        out[fld] = q.astype(np.float32)
    return info, out
