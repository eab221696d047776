"""Synthetic tunnel frames (build-defined; the reference ships no data).

The reference's only data hint is a commented-out Velodyne rosbag path
(/root/reference launch/mapping.launch:29-32), so every test and benchmark
frame is produced here: a noisy cylinder of radius R around an axis through
the sensor origin, optionally with a floor plane and uniform outliers.
Seeded with numpy's PCG64 so the same (n, seed) gives the same float32 cloud
on every machine.
"""
from __future__ import annotations

import numpy as np

__all__ = ["tunnel_frame", "cylinder_frame", "plane_patch", "fixed_k_radius", "to_pointcloud2", "velodyne_tunnel", "drop_row_padding"]


def _basis(axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = np.array([0.0, 0.0, 1.0]) if abs(a[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(h, a)
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    return a, u, v


def cylinder_frame(n, seed=0, radius=2.0, length=12.0, sigma=0.01, axis=(1.0, 0.0, 0.0)):
    """n points on a noisy cylinder; float32 (n,3), generation order (unsorted)."""
    rng = np.random.default_rng(seed)
    a, u, v = _basis(axis)
    t = rng.uniform(-length / 2, length / 2, n)
    th = rng.uniform(0.0, 2 * np.pi, n)
    rr = radius + rng.normal(0.0, sigma, n)
    p = t[:, None] * a + (rr * np.cos(th))[:, None] * u + (rr * np.sin(th))[:, None] * v
    return np.ascontiguousarray(p, dtype=np.float32)


def tunnel_frame(n, seed=0, radius=2.0, length=12.0, sigma=0.01, axis=(1.0, 0.0, 0.0),
                 floor_z=None, outlier_frac=0.0, outlier_cube=6.0):
    """Cylinder, optionally with a floor (points below floor_z are projected
    onto the plane z=floor_z with N(0,sigma) noise) and a fraction of uniform
    outliers in a +-outlier_cube box (config 3 uses
    floor_z=-1.2, outlier_frac=0.01)."""
    rng = np.random.default_rng(seed)
    a, u, v = _basis(axis)
    t = rng.uniform(-length / 2, length / 2, n)
    th = rng.uniform(0.0, 2 * np.pi, n)
    rr = radius + rng.normal(0.0, sigma, n)
    p = t[:, None] * a + (rr * np.cos(th))[:, None] * u + (rr * np.sin(th))[:, None] * v
    if floor_z is not None:
        below = p[:, 2] < floor_z
        p[below, 2] = floor_z + rng.normal(0.0, sigma, int(below.sum()))
    if outlier_frac > 0.0:
        m = int(round(n * outlier_frac))
        idx = rng.choice(n, size=m, replace=False)
        p[idx] = rng.uniform(-outlier_cube, outlier_cube, (m, 3))
    return np.ascontiguousarray(p, dtype=np.float32)


def plane_patch(n, seed=0, normal=(0.0, 0.0, 1.0), offset=1.5, half=3.0, sigma=0.0):
    """n points on the plane normal.p = offset (|in-plane coords| <= half)."""
    rng = np.random.default_rng(seed)
    a, u, v = _basis(normal)
    s = rng.uniform(-half, half, n)
    t = rng.uniform(-half, half, n)
    e = rng.normal(0.0, sigma, n) if sigma > 0 else np.zeros(n)
    p = (offset + e)[:, None] * a + s[:, None] * u + t[:, None] * v
    return np.ascontiguousarray(p, dtype=np.float32)


def fixed_k_radius(n, r50k=0.5):
    """Neighbour radius that keeps k~256 as the frame grows (SURVEY.md §8d:
    r = 0.5*sqrt(50000/N); surface density scales with N, disc area with r^2)."""
    return float(r50k * np.sqrt(50000.0 / float(n)))


def to_pointcloud2(xyz, point_step=16, offsets=(0, 4, 8), fill=0):
    """Pack (n,3) float32 into sensor_msgs/PointCloud2 `data` rows: the byte
    layout pcl::fromROSMsg reads at /root/reference src/geometric_mapping.cpp:55."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = xyz.shape[0]
    buf = np.full((n, point_step), fill, dtype=np.uint8)
    raw = xyz.view(np.uint8).reshape(n, 12)
    for k, off in enumerate(offsets):
        buf[:, off:off + 4] = raw[:, 4 * k:4 * k + 4]
    return buf.reshape(-1)


def velodyne_tunnel(rings=16, az=1800, seed=0, radius=2.0, axis_offset=(0.3, 0.5), floor_z=-1.2, sigma=0.01,
                    max_range=30.0, nan_frac=0.02, point_step=32, row_pad=0):
    """A spinning multi-beam lidar inside the tunnel: what /velodyne_points carries
    (/root/reference launch/mapping.launch:22; the reference's only data hint is a Velodyne rosbag, :29-32).

    The sensor sits at the origin; the tunnel is a cylinder of `radius` around an x-parallel axis through
    (0, axis_offset), cut by a floor plane z = floor_z.  `rings` beams at evenly spaced elevations (+-15 deg for 16 rings,
    -25..+15 deg otherwise, like the VLP-16 / HDL-32 / HDL-64) sweep `az` azimuth steps; every ray returns its nearest hit
    with N(0, sigma) range noise, or NaN when it hits nothing within max_range (rays along the tunnel) or drops out
    (nan_frac).  The cloud is ORGANISED: height = rings, width = az, one row of the message per ring, each row
    row_pad bytes longer than width * point_step -- row_step padding, which pcl::fromROSMsg honours
    (src/geometric_mapping.cpp:55).  Density falls off with range: a few centimetres between returns on the wall beside
    the sensor, decimetres at the far ends of the crop box -- the frame the uniform-density generator above is not.

    Returns dict(data=uint8 message bytes, height, width, point_step, row_step, offsets=(x, y, z),
                 xyz=float32 [height * width, 3] in message order, NaN rows included).
    point_step 32: x, y, z at 0 / 4 / 8, intensity float at 16, ring uint16 at 20 (velodyne_pointcloud's XYZIR);
    point_step 22: x, y, z at 0 / 4 / 8, intensity at 12, ring at 16, time float at 18 (XYZIRT, unaligned rows)."""
    if point_step not in (22, 32):
        raise ValueError("point_step must be 22 or 32")
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(-15.0, 15.0, rings) if rings <= 16 else np.linspace(-25.0, 15.0, rings))
    th = np.linspace(0.0, 2.0 * np.pi, az, endpoint=False) + rng.uniform(0, 2 * np.pi / az)
    E, T = np.meshgrid(el, th, indexing="ij")                  # [rings, az]
    d = np.stack([np.cos(E) * np.cos(T), np.cos(E) * np.sin(T), np.sin(E)], axis=-1).reshape(-1, 3)
    oy, oz = float(axis_offset[0]), float(axis_offset[1])
    # cylinder around the x-parallel axis through (0, oy, oz): |(t d)_yz - (oy, oz)|^2 = R^2, sensor inside
    a = d[:, 1] ** 2 + d[:, 2] ** 2
    b = -2.0 * (d[:, 1] * oy + d[:, 2] * oz)
    c = oy * oy + oz * oz - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(divide="ignore", invalid="ignore"):
        t_cyl = np.where(a > 1e-12, (-b + np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
        t_floor = np.where(d[:, 2] < -1e-9, floor_z / d[:, 2], np.inf) if floor_z is not None else np.full(len(d), np.inf)
    t = np.minimum(t_cyl, t_floor)
    t = t + rng.normal(0.0, sigma, len(t))
    hit = np.isfinite(t) & (t > 0.3) & (t < max_range) & (rng.random(len(t)) >= nan_frac)
    xyz = np.where(hit[:, None], d * t[:, None], np.nan).astype(np.float32)
    row_step = az * point_step + int(row_pad)
    buf = np.full((rings, row_step), 0xC3, dtype=np.uint8)
    pts = buf[:, : az * point_step].reshape(rings, az, point_step)
    raw = xyz.view(np.uint8).reshape(rings, az, 12)
    pts[:, :, 0:12] = raw
    inten = rng.uniform(0, 255, rings * az).astype(np.float32).view(np.uint8).reshape(rings, az, 4)
    ring = np.repeat(np.arange(rings, dtype=np.uint16), az).view(np.uint8).reshape(rings, az, 2)
    if point_step == 32:
        pts[:, :, 16:20] = inten; pts[:, :, 20:22] = ring
    else:
        pts[:, :, 12:16] = inten; pts[:, :, 16:18] = ring
    return dict(data=np.ascontiguousarray(buf).reshape(-1), height=rings, width=az, point_step=point_step, row_step=row_step,
                offsets=(0, 4, 8), xyz=xyz)


SURFACE_PATCHES = ((-2.0, -1.0, 20.0, 44.0, 0.15), (1.0, 2.0, 316.0, 340.0, -0.15))


def tunnel_patches(n, seed=0, radius=2.0, length=12.0, sigma=0.01, floor_z=-1.2, patches=SURFACE_PATCHES):
    """A tunnel along +x (like tunnel_frame, no outliers) whose wall is pushed radially by dr inside known patches.
    A patch is (t0, t1, phi0_deg, phi1_deg, dr) in the coordinates of the wall deviation map (GM_CFG_SURFACE_MAP) with
    its default up = +z: t along x, phi from +z turning toward a x u = -y.  Points below floor_z are projected onto the
    floor as in tunnel_frame.  The defaults lie on the upper half of the wall, aligned with the default map cells
    (0.25 m x 4 degrees from t = -5): 4 stations x 6 sectors each, +0.15 m and -0.15 m.  float32 (n, 3)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-length / 2, length / 2, n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    rr = radius + rng.normal(0.0, sigma, n)
    deg = np.rad2deg(phi)
    for t0, t1, p0, p1, dr in patches:
        rr = np.where((t >= t0) & (t < t1) & (deg >= p0) & (deg < p1), rr + dr, rr)
    # u = +z, v = a x u = -y
    p = np.stack([t, -rr * np.sin(phi), rr * np.cos(phi)], axis=1)
    if floor_z is not None:
        below = p[:, 2] < floor_z
        p[below, 2] = floor_z + rng.normal(0.0, sigma, int(below.sum()))
    return np.ascontiguousarray(p, dtype=np.float32)


DRIVE_PATCHES = ((10.0, 12.0, 20.0, 44.0, 0.15), (25.0, 27.0, 316.0, 340.0, -0.15), (33.0, 34.0, 100.0, 140.0, 0.15))


def pose_matrix(position, yaw_deg=0.0, roll_deg=0.0, pitch_deg=0.0):
    """Row-major 3x4 [Rm | tr], sensor -> world: Rm = Rz(yaw) Ry(pitch) Rx(roll), tr = position.  float64."""
    y, p, r = np.deg2rad([yaw_deg, pitch_deg, roll_deg])
    rz = np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[np.cos(p), 0.0, np.sin(p)], [0.0, 1.0, 0.0], [-np.sin(p), 0.0, np.cos(p)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(r), -np.sin(r)], [0.0, np.sin(r), np.cos(r)]])
    return np.concatenate([rz @ ry @ rx, np.asarray(position, np.float64).reshape(3, 1)], axis=1)


def wall_texture(t, phi, seed=0, amplitude=0.04, length=48.0, bumps_per_metre=4.0, sigma_t=(0.15, 0.6), sigma_phi=(0.08, 0.4)):
    """A deterministic, world-fixed radial texture of a tunnel wall (metres, same shape as t): a sum of Gaussian bumps of
    heights up to +-amplitude at centres drawn by `seed` over chainage [0, length) and the whole ring, with widths drawn
    from sigma_t (metres) and sigma_phi (radians); the angular distance wraps.  The value at (t, phi) depends on the seed
    and the position alone, not on the other points of the call: joints, bolts, niches and rough rock for the align
    (gm_wall_map_align_*), which a smooth lining cannot serve."""
    t = np.asarray(t, np.float64)
    phi = np.asarray(phi, np.float64)
    rng = np.random.default_rng([int(seed), 0x7E87])
    nb = max(1, int(round(bumps_per_metre * length)))
    ct, cp = rng.uniform(0.0, length, nb), rng.uniform(0.0, 2 * np.pi, nb)
    st, sp = rng.uniform(*sigma_t, nb), rng.uniform(*sigma_phi, nb)
    h = rng.uniform(-amplitude, amplitude, nb)
    out = np.zeros(t.shape, np.float64)
    order = np.argsort(t.reshape(-1), kind="stable")
    ts, ps = t.reshape(-1)[order], phi.reshape(-1)[order]
    acc = np.zeros(len(ts), np.float64)
    for i in range(nb):   # a bump reaches 4 sigma along the axis: only the points in that span see it
        lo, hi = np.searchsorted(ts, (ct[i] - 4 * st[i], ct[i] + 4 * st[i]))
        if lo == hi:
            continue
        dp = np.mod(ps[lo:hi] - cp[i] + np.pi, 2 * np.pi) - np.pi
        acc[lo:hi] += h[i] * np.exp(-0.5 * (((ts[lo:hi] - ct[i]) / st[i]) ** 2 + (dp / sp[i]) ** 2))
    out.reshape(-1)[order] = acc
    return out


def tunnel_drive(n_frames, n_points, seed=0, radius=2.0, length=48.0, start=6.0, step=3.5, reach=7.0, sigma=0.01,
                 patches=DRIVE_PATCHES, yaw_deg=4.0, roll_deg=3.0, lateral=0.25, texture=None):
    """A drive through a straight tunnel for the persistent wall map (gm_wall_*).  The WORLD frame is the map frame: the
    design cylinder has its axis along +x through the origin, `radius`, up = +z, and runs from chainage 0 to `length`.
    The wall carries world-fixed patches (t0, t1, phi0_deg, phi1_deg, dr) in design-map coordinates (the SURFACE_PATCHES
    form: phi from +z turning toward -y); the defaults are aligned with 0.25 m x 4 degree cells from t_min = 0.
    Frame i sees the wall within `reach` metres of chainage start + i step from a sensor with a yaw / roll of up to
    +-yaw_deg / +-roll_deg and a lateral offset of up to `lateral` metres in y and z (step < the crop length, so
    neighbouring frames overlap).  Radial noise N(0, sigma).  texture: None (a smooth wall) or the keywords of wall_texture
    (seed, amplitude, ...), whose world-fixed bumps are added to the radius; the draws of the frame do not change.  Returns dict(frames=[(cloud float32 (n_points, 3) in SENSOR
    coordinates, pose float64 (3, 4) sensor -> world), ...], design=dict(point, direction, radius, up, forward),
    patches, sigma, length)."""
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n_frames):
        s = start + i * step
        pose = pose_matrix((s, rng.uniform(-lateral, lateral), rng.uniform(-lateral, lateral)),
                           yaw_deg=rng.uniform(-yaw_deg, yaw_deg), roll_deg=rng.uniform(-roll_deg, roll_deg))
        t = rng.uniform(max(0.0, s - reach), min(length, s + reach), n_points)
        phi = rng.uniform(0.0, 2 * np.pi, n_points)
        rr = radius + rng.normal(0.0, sigma, n_points)
        deg = np.rad2deg(phi)
        for t0, t1, p0, p1, dr in patches:
            rr = np.where((t >= t0) & (t < t1) & (deg >= p0) & (deg < p1), rr + dr, rr)
        if texture is not None:
            rr = rr + wall_texture(t, phi, **texture)
        world = np.stack([t, -rr * np.sin(phi), rr * np.cos(phi)], axis=1)
        sensor = (world - pose[:, 3]) @ pose[:, :3]   # Rm^T (p - tr)
        frames.append((np.ascontiguousarray(sensor, dtype=np.float32), pose))
    design = dict(point=(0.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), radius=float(radius), up=(0.0, 0.0, 1.0),
                  forward=(1.0, 0.0, 0.0))
    return dict(frames=frames, design=design, patches=tuple(patches), sigma=sigma, length=length)


def arc_sections(t, arc_radius, toward):
    """The sections of the arc design axis of arc_drive at chainages t [n]: (P, a, u, v), float64 [n, 3] each.  The axis
    starts at the origin along +x with up = +z and turns toward `toward` (made perpendicular to x) at 1 / arc_radius:
    a(s) = a cos psi + n sin psi, n(s) = n cos psi - a sin psi, P(s) = C - arc_radius n(s), psi = s / arc_radius; u and v
    turn with the section about b = a x n."""
    t = np.asarray(t, np.float64).reshape(-1)
    a = np.array([1.0, 0.0, 0.0])
    n = np.asarray(toward, np.float64) - np.dot(toward, a) * a
    n = n / np.linalg.norm(n)
    b = np.cross(a, n)
    u0, v0 = np.array([0.0, 0.0, 1.0]), np.array([0.0, -1.0, 0.0])
    psi = t / float(arc_radius)
    c, s = np.cos(psi)[:, None], np.sin(psi)[:, None]
    a_s = a * c + n * s
    n_s = n * c - a * s
    P = arc_radius * n - arc_radius * n_s
    u = (u0 @ n) * n_s + (u0 @ b) * b
    v = (v0 @ n) * n_s + (v0 @ b) * b
    return P, a_s, u, v


def arc_drive(n_frames, n_points, arc_radius=80.0, toward=(0.0, 1.0, 0.0), seed=0, radius=2.0, length=48.0, start=6.0,
              step=3.5, reach=7.0, sigma=0.01, patches=DRIVE_PATCHES, yaw_deg=4.0, roll_deg=3.0, lateral=0.25, texture=None):
    """tunnel_drive on a curved tube, for a wall map on a circular-arc design axis (gm_wall_map_create_arc).  The design
    axis starts at the world origin along +x (chainage 0, up = +z) and is a circle of `arc_radius` whose centre lies
    toward `toward` from the origin: (0, 1, 0) a horizontal curve to the left, (0, 0, +-1) a vertical curve, anything
    else perpendicular to x an oblique plane of curvature.  Patches and texture stay in (chainage, phi), phi in the
    section's own (u(s), v(s)); the sensor rides the axis: its pose is the section's frame at chainage start + i step
    times tunnel_drive's yaw / roll, offset laterally in the section.  The draws are tunnel_drive's, in its order.  Returns
    tunnel_drive's dict plus arc=dict(curvature, point_chainage) for GeometricMapping.wall_map(arc=...)."""
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n_frames):
        s = start + i * step
        ly, lz = rng.uniform(-lateral, lateral), rng.uniform(-lateral, lateral)
        local = pose_matrix((0.0, 0.0, 0.0), yaw_deg=rng.uniform(-yaw_deg, yaw_deg), roll_deg=rng.uniform(-roll_deg, roll_deg))
        P, a_s, u_s, v_s = (x[0] for x in arc_sections([s], arc_radius, toward))
        F = np.stack([a_s, -v_s, u_s], axis=1)   # the section as a sensor frame: x forward, y left, z up
        pose = np.concatenate([F @ local[:, :3], (P - ly * v_s + lz * u_s).reshape(3, 1)], axis=1)
        t = rng.uniform(max(0.0, s - reach), min(length, s + reach), n_points)
        phi = rng.uniform(0.0, 2 * np.pi, n_points)
        rr = radius + rng.normal(0.0, sigma, n_points)
        deg = np.rad2deg(phi)
        for t0, t1, p0, p1, dr in patches:
            rr = np.where((t >= t0) & (t < t1) & (deg >= p0) & (deg < p1), rr + dr, rr)
        if texture is not None:
            rr = rr + wall_texture(t, phi, **texture)
        Pt, _, ut, vt = arc_sections(t, arc_radius, toward)
        world = Pt + (rr * np.cos(phi))[:, None] * ut + (rr * np.sin(phi))[:, None] * vt
        sensor = (world - pose[:, 3]) @ pose[:, :3]   # Rm^T (p - tr)
        frames.append((np.ascontiguousarray(sensor, dtype=np.float32), pose))
    design = dict(point=(0.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), radius=float(radius), up=(0.0, 0.0, 1.0),
                  forward=(1.0, 0.0, 0.0))
    n = np.asarray(toward, np.float64) - np.array([float(toward[0]), 0.0, 0.0])
    arc = dict(curvature=tuple(n / np.linalg.norm(n) / float(arc_radius)), point_chainage=0.0)
    return dict(frames=frames, design=design, arc=arc, patches=tuple(patches), sigma=sigma, length=length)


def clothoid_sections(t, curvature, rate, toward):
    """The sections of the clothoid design axis of clothoid_drive at chainages t [n]: (P, a, u, v), float64 [n, 3] each,
    and the signed curvature there [n].  The axis starts at the origin along +x with up = +z; its curvature toward
    `toward` (made perpendicular to x) is curvature + rate s, so psi = curvature s + rate s^2 / 2,
    a(s) = a cos psi + n sin psi, n(s) = n cos psi - a sin psi and P(s) = the integral of a from 0 to s: four panels of a
    20-node Gauss-Legendre rule per point (a quadrature of its own: the library's and the test twin's are others)."""
    t = np.asarray(t, np.float64).reshape(-1)
    a = np.array([1.0, 0.0, 0.0])
    n = np.asarray(toward, np.float64) - np.dot(toward, a) * a
    n = n / np.linalg.norm(n)
    b = np.cross(a, n)
    u0, v0 = np.array([0.0, 0.0, 1.0]), np.array([0.0, -1.0, 0.0])
    k0, c = float(curvature), float(rate)
    x, w = np.polynomial.legendre.leggauss(20)
    X, Y = np.zeros(len(t)), np.zeros(len(t))
    for q in range(4):
        sg = (t[:, None] / 4.0) * (q + 0.5 + 0.5 * x[None, :])
        ps = k0 * sg + 0.5 * c * sg * sg
        X += (t / 8.0) * (np.cos(ps) @ w)
        Y += (t / 8.0) * (np.sin(ps) @ w)
    psi = k0 * t + 0.5 * c * t * t
    cs, sn = np.cos(psi)[:, None], np.sin(psi)[:, None]
    a_s = a * cs + n * sn
    n_s = n * cs - a * sn
    P = X[:, None] * a + Y[:, None] * n
    u = (u0 @ n) * n_s + (u0 @ b) * b
    v = (v0 @ n) * n_s + (v0 @ b) * b
    return P, a_s, u, v, k0 + c * t


def clothoid_drive(n_frames, n_points, curvature=0.0, rate=1.0 / (80.0 * 48.0), toward=(0.0, 1.0, 0.0), seed=0, radius=2.0,
                   length=48.0, start=6.0, step=3.5, reach=7.0, sigma=0.01, patches=DRIVE_PATCHES, yaw_deg=4.0, roll_deg=3.0,
                   lateral=0.25, texture=None):
    """arc_drive on a tube whose axis is a clothoid, for a wall map on a transition curve (gm_wall_map_create_clothoid).
    The design axis starts at the world origin along +x (chainage 0, up = +z) with the signed curvature `curvature` toward
    `toward`, which grows by `rate` per metre (the default: from straight to an 80 m radius over `length`).  Everything
    else, the draws and their order included, is arc_drive's.  Returns tunnel_drive's dict plus
    clothoid=dict(normal, curvature, rate, point_chainage) for GeometricMapping.wall_map(clothoid=...)."""
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n_frames):
        s = start + i * step
        ly, lz = rng.uniform(-lateral, lateral), rng.uniform(-lateral, lateral)
        local = pose_matrix((0.0, 0.0, 0.0), yaw_deg=rng.uniform(-yaw_deg, yaw_deg), roll_deg=rng.uniform(-roll_deg, roll_deg))
        P, a_s, u_s, v_s = (x[0] for x in clothoid_sections([s], curvature, rate, toward)[:4])
        F = np.stack([a_s, -v_s, u_s], axis=1)   # the section as a sensor frame: x forward, y left, z up
        pose = np.concatenate([F @ local[:, :3], (P - ly * v_s + lz * u_s).reshape(3, 1)], axis=1)
        t = rng.uniform(max(0.0, s - reach), min(length, s + reach), n_points)
        phi = rng.uniform(0.0, 2 * np.pi, n_points)
        rr = radius + rng.normal(0.0, sigma, n_points)
        deg = np.rad2deg(phi)
        for t0, t1, p0, p1, dr in patches:
            rr = np.where((t >= t0) & (t < t1) & (deg >= p0) & (deg < p1), rr + dr, rr)
        if texture is not None:
            rr = rr + wall_texture(t, phi, **texture)
        Pt, _, ut, vt, _ = clothoid_sections(t, curvature, rate, toward)
        world = Pt + (rr * np.cos(phi))[:, None] * ut + (rr * np.sin(phi))[:, None] * vt
        sensor = (world - pose[:, 3]) @ pose[:, :3]   # Rm^T (p - tr)
        frames.append((np.ascontiguousarray(sensor, dtype=np.float32), pose))
    design = dict(point=(0.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), radius=float(radius), up=(0.0, 0.0, 1.0),
                  forward=(1.0, 0.0, 0.0))
    n = np.asarray(toward, np.float64) - np.array([float(toward[0]), 0.0, 0.0])
    clothoid = dict(normal=tuple(n / np.linalg.norm(n)), curvature=float(curvature), rate=float(rate), point_chainage=0.0)
    return dict(frames=frames, design=design, clothoid=clothoid, patches=tuple(patches), sigma=sigma, length=length)


def drop_row_padding(msg):
    """What the node does with an organised cloud whose rows are padded (ros/geometric_mapping_node.cpp): the C ABI takes
    point_step-strided rows, so the row_step padding is dropped once on the host.  Returns the packed uint8 rows."""
    h, w, ps, rs = msg["height"], msg["width"], msg["point_step"], msg["row_step"]
    return np.ascontiguousarray(msg["data"].reshape(h, rs)[:, : w * ps]).reshape(-1)
