"""fp64 numpy twin of the cylinder regression (GM_CFG_CYLINDER_FIT, csrc/k_cylfit.hip; include/gm_hip.h states it).

Same passes, same gates, same re-centring and the same fp32 rounding of the model at the start of every pass (the device
evaluates its per-point geometry in fp32 on the rounded model; here it is fp64 on the same rounded model).  The sums and
the 5x5 solve are fp64 on both sides, so the twin and the device agree to the rounding of per-point fp32 arithmetic.
The twin's label pass decides in fp64; the device's labels are checked against the oracle's fp32 predicate instead.
"""
import numpy as np

FIT_OK, FIT_NO_MODEL, FIT_DEGENERATE, FIT_SINGULAR = 0, 1, 2, 3
FIT_NOT_CONVERGED = 1 << 8
STEP_BOUND = 1e-2


def basis(d):
    """e1, e2 perpendicular to the unit d: e1 = (h x d) / |h x d|, h = z unless |d_z| >= 0.9 (then y); e2 = d x e1."""
    h = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(h, d)
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(d, e1)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _failed(status, passes):
    nan = float("nan")
    return dict(status=status, passes=passes, point=np.full(3, nan), axis=np.full(3, nan), radius=nan, rms=nan,
                last_step=nan, model=np.full(7, np.nan, np.float32), inliers=None, n_inliers=0)


def fit_cylinder(xyz, init7, tau, eligible=None):
    """xyz [n,3]; init7 = (point, direction, radius); eligible: boolean mask (None: every point).
    Returns dict(status, passes, point, axis, radius, rms, last_step, model (fp32 row), inliers (mask), n_inliers)."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    el = np.ones(len(p), bool) if eligible is None else np.asarray(eligible, bool)
    init = np.asarray(init7, np.float64)
    c, d, r = init[:3].copy(), init[3:6].copy(), float(init[6])
    dn = np.linalg.norm(d)
    if not (np.all(np.isfinite(init)) and dn > 0):
        return _failed(FIT_NO_MODEL, 0)
    d /= dn
    dh = d.copy()
    step = float("nan")
    for k in range(3):
        e1, e2 = basis(d)
        cf, df, rf, e1f, e2f = _f32(c), _f32(d), float(np.float32(r)), _f32(e1), _f32(e2)
        gate = float(np.float32((4 >> k) * tau))
        v = p - cf
        t = v @ df
        w = v - t[:, None] * df
        rho = np.linalg.norm(w, axis=1)
        res = rho - rf
        with np.errstate(invalid="ignore"):
            m = el & (np.abs(res) < gate) & (rho > 0)
        cnt = int(m.sum())
        if cnt < 5:
            return _failed(FIT_DEGENERATE, k)
        t, res, nh = t[m], res[m], w[m] / rho[m][:, None]
        tb = t.mean()
        a1, a2 = -(nh @ e1f), -(nh @ e2f)
        J = np.stack([a1, a2, (t - tb) * a1, (t - tb) * a2, -np.ones(cnt)], axis=1)
        M, g = J.T @ J, J.T @ res
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return _failed(FIT_SINGULAR, k)
        if not np.all(np.diag(L) ** 2 > 1e-12 * np.diag(M)):
            return _failed(FIT_SINGULAR, k)
        x = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        c = c + tb * d + x[0] * e1 + x[1] * e2
        d = d + x[2] * e1 + x[3] * e2
        d /= np.linalg.norm(d)
        r = r + x[4]
        step = float(np.linalg.norm(x))
    if d @ dh < 0:
        d = -d
    row = np.concatenate([c, d, [r]]).astype(np.float32)
    rw = row.astype(np.float64)
    v = p - rw[:3]
    t = v @ rw[3:6]
    q = np.einsum("ij,ij->i", v, v) - t * t
    lo, hi = r - tau, r + tau
    lo2 = float(np.float32(lo * lo)) if lo > 0 else -1.0
    with np.errstate(invalid="ignore"):
        inl = el & (q > lo2) & (q < float(np.float32(hi * hi)))
    n_in = int(inl.sum())
    tb = t[inl].mean() if n_in else 0.0
    rms = float(np.sqrt(((np.sqrt(q[inl]) - rw[6]) ** 2).mean())) if n_in else float("nan")
    status = FIT_OK | (FIT_NOT_CONVERGED if step > STEP_BOUND else 0)
    return dict(status=status, passes=3, point=c + tb * d, axis=d, radius=float(r), rms=rms, last_step=step, model=row,
                inliers=inl, n_inliers=n_in)


def axis_angle(a, b):
    """Angle between two lines (sign-free), radians."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.arcsin(min(1.0, s)))


def line_distance(point, origin, direction):
    """Distance of `point` from the line through `origin` along `direction`."""
    v = np.asarray(point, np.float64) - np.asarray(origin, np.float64)
    u = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    return float(np.linalg.norm(v - (v @ u) * u))


def perturbed_init(origin, direction, radius, dr=0.05, tilt=0.04, shift=0.05):
    """A starting row off the truth by dr in radius, `tilt` rad in axis and `shift` m in axis point (perpendicular)."""
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    e1, e2 = basis(d)
    dt = np.cos(tilt) * d + np.sin(tilt) * (e1 + e2) / np.sqrt(2.0)
    c = np.asarray(origin, np.float64) + shift * (e1 - e2) / np.sqrt(2.0)
    return np.concatenate([c, dt, [radius + dr]]).astype(np.float32)
