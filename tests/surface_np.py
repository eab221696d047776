"""fp64 numpy twin of the wall deviation map (GM_CFG_SURFACE_MAP, csrc/k_surface.hip; include/gm_hip.h states it).

The map frame is built here from the fp32 model row exactly as stated (fp64, then rounded to fp32), but the per-point
part takes the frame vectors the device REPORTED (o, a, u, v as fp64 inputs): the device bins in fp32 on those rounded
vectors, the twin in fp64 on the same vectors, so the two agree to the rounding of a few fp32 operations.  Points whose
bin coordinate lies within 1e-3 of a station or sector edge, or whose |e| lies within 1e-5 m of the gate, are flagged
ambiguous: fp32 and fp64 may put them on different sides.

cells_from() is the integer rule of the device, bit for bit: sum of rint(e 2^20) in int64, mean = sum 2^-20 / count in
fp64 rounded to fp32 once, min / max of the fp32 residuals.
"""
import numpy as np

SURF_OK, SURF_NO_MODEL, SURF_UP_FALLBACK = 0, 1, 1 << 8
MAPPED, OUTSIDE, BEYOND, PLANE = 0, 1, 2, 3
DEFAULTS = dict(n_stations=40, n_sectors=90, station_length=0.25, t_min=-5.0, gate=0.25, up=(0.0, 0.0, 1.0),
                forward=(1.0, 0.0, 0.0))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def basis_e1(a):
    """The fit basis' e1 of the unit a (k_cylfit.hip fit_basis, cylfit_np.basis)."""
    h = np.array([0.0, 0.0, 1.0]) if abs(a[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(h, a)
    return e1 / np.linalg.norm(e1)


def map_frame(model7, up=(0.0, 0.0, 1.0), forward=(1.0, 0.0, 0.0)):
    """dict(o, a, u, v (fp64 values of the fp32 vectors), R, status) or None when the row is not finite."""
    m = np.asarray(model7, np.float32).astype(np.float64)
    c, d, R = m[:3], m[3:6], m[6]
    dn = np.linalg.norm(d)
    if not (np.all(np.isfinite(m)) and dn > 0):
        return None
    a = (d if d @ np.asarray(forward, np.float64) >= 0 else -d) / dn
    o = c - (c @ a) * a
    up = np.asarray(up, np.float64)
    w = up - (up @ a) * a
    status = SURF_OK
    if np.linalg.norm(w) < 0.1 * np.linalg.norm(up):
        u, status = basis_e1(a), SURF_UP_FALLBACK
    else:
        u = w / np.linalg.norm(w)
    v = np.cross(a, u)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    return dict(o=f32(o), a=f32(a), u=f32(u), v=f32(v), R=float(np.float32(R)), status=status)


def points(xyz, labels, o, a, u, v, R, p):
    """Per point: e (NaN for plane points), t, phi, class, cell (-1 unless mapped), ambiguous mask.  o, a, u, v, R:
    the device's reported frame; p: params() dict (the fp32 binning constants are taken as the device rounds them)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(x)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    o, a, u, v = (np.asarray(q, np.float64) for q in (o, a, u, v))
    t_min = float(np.float32(p["t_min"]))
    ds = float(np.float32(p["station_length"]))
    gate = float(np.float32(p["gate"]))
    dth = float(np.float32(2 * np.pi / p["n_sectors"]))
    q = x - o
    t = q @ a
    w = q - t[:, None] * a
    e = np.sqrt((w * w).sum(1)) - R
    phi = np.mod(np.arctan2(w @ v, w @ u), 2 * np.pi)
    xs = (t - t_min) / ds
    ys = phi / dth
    j = np.floor(xs)
    k = np.minimum(np.floor(ys), p["n_sectors"] - 1)
    cls = np.full(n, MAPPED, np.int8)
    plane = lab == 1
    beyond = ~plane & ~(np.abs(e) <= gate)
    outside = ~plane & ~beyond & ~((j >= 0) & (j < p["n_stations"]))
    cls[outside] = OUTSIDE
    cls[beyond] = BEYOND
    cls[plane] = PLANE
    mapped = cls == MAPPED
    cell = np.full(n, -1, np.int64)
    cell[mapped] = (j[mapped] * p["n_sectors"] + k[mapped]).astype(np.int64)
    amb = ~plane & ((np.abs(xs - np.rint(xs)) < 1e-3) | (np.abs(ys - np.rint(ys)) < 1e-3) |
                    (np.abs(np.abs(e) - gate) < 1e-5))
    e = np.where(plane, np.nan, e)
    return dict(e=e, t=t, phi=phi, cls=cls, cell=cell, ambiguous=amb)


def cells_from(e, cell, n_cells):
    """The device's integer rule on per-point (e fp32, cell): count, mean, min, max (fp32, NaN when empty)."""
    e = np.asarray(e, np.float32)
    cell = np.asarray(cell, np.int64)
    m = cell >= 0
    c, ee = cell[m], e[m]
    key = np.rint(ee * np.float32(2.0 ** 20)).astype(np.int64)
    count = np.bincount(c, minlength=n_cells).astype(np.uint32)
    s = np.zeros(n_cells, np.int64)
    np.add.at(s, c, key)
    mn = np.full(n_cells, np.inf, np.float32)
    mx = np.full(n_cells, -np.inf, np.float32)
    np.minimum.at(mn, c, ee)
    np.maximum.at(mx, c, ee)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = ((s.astype(np.float64) * 2.0 ** -20) / count.astype(np.float64)).astype(np.float32)
    empty = count == 0
    mean[empty] = np.nan
    mn[empty] = np.nan
    mx[empty] = np.nan
    return count, mean, mn, mx
