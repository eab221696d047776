"""numpy twin of the wall alignment (include/gm_hip.h: gm_wall_alignment_create): the chaining of the spans, the chainage
window, the fp32 ownership rule of the joint kernel with its forward-error bound, and the synthetic frames the alignment
tests share.  The element maps' own rules stay with their twins (wall_np, wall_arc_np, wall_clothoid_np)."""
import numpy as np

import fp32_np as f32
from geometric_mapping_amd import synth

F = np.float32
U = 2.0 ** -24   # unit roundoff of fp32

# the issue's alignment: straight - transition - curve - transition - straight at ds = 0.25, R = 2, arc radius 80
DS, RADIUS, ARC_R = 0.25, 2.0, 80.0
LEFT = (0.0, -1.0)   # +y with the default up = +z: v = a x u = -y


def elements5(n_straight=40, n_clothoid=48, n_arc=40, arc_r=ARC_R, ds=DS, turn=LEFT):
    lc = n_clothoid * ds
    return [dict(kind="straight", n_stations=n_straight),
            dict(kind="clothoid", n_stations=n_clothoid, turn=turn, curvature=0.0, rate=1.0 / (arc_r * lc)),
            dict(kind="arc", n_stations=n_arc, turn=turn, curvature=1.0 / arc_r),
            dict(kind="clothoid", n_stations=n_clothoid, turn=turn, curvature=1.0 / arc_r, rate=-1.0 / (arc_r * lc)),
            dict(kind="straight", n_stations=n_straight)]


def spans(elements, t_min=0.0, ds=DS):
    """(s_start, s_end) per element: s_start_0 = t_min, s_end = s_start + n_stations ds (the header's order)."""
    out, s = [], float(t_min)
    for e in elements:
        out.append((s, s + float(e["n_stations"]) * ds))
        s = out[-1][1]
    return out


def window(elements, s_from, s_to, t_min=0.0, ds=DS):
    """The header's window rule: [(element, station0, n_stations)]."""
    out = []
    for i, ((s0, s1), e) in enumerate(zip(spans(elements, t_min, ds), elements)):
        lo, hi = max(s_from, s0), min(s_to, s1)
        if not lo < hi:
            continue
        j0 = min(max(np.floor((lo - s0) / ds), 0.0), e["n_stations"])
        j1 = min(max(np.ceil((hi - s0) / ds), 0.0), e["n_stations"])
        if j0 < j1:
            out.append((i, int(j0), int(j1 - j0)))
    return out


def design_uv(point, direction, up, forward):
    """(a, u, v) of the straight rule's design frame (gm_wall_params -> the frame), fp64."""
    d, up, fw = (np.asarray(x, np.float64) for x in (direction, up, forward))
    a = (d if d @ fw >= 0.0 else -d) / np.sqrt(d @ d)
    u = up - (up @ a) * a
    u = u / np.sqrt(u @ u)
    return a, u, np.cross(a, u)


def axes(A, s):
    """(P, a, u, v) of the alignment's section at chainage s, from the library's point rule."""
    P, pu, pv = A.point([s, s, s], [0.0, 0.0, 0.5 * np.pi], [0.0, 1.0, 1.0])
    u, v = pu - P, pv - P
    return P, np.cross(u, v), u, v


def frame(A, s, n, seed, half=4.5, lateral=(0.2, -0.1), yaw_deg=3.0, sigma=0.005, radius=RADIUS, length=200.0):
    """A frame of n wall points seen from chainage s: (cloud float32 [n, 3] in sensor coordinates, pose float64 [3, 4]).
    The wall is the design tube plus synth.wall_texture and noise, over chainages s +- half."""
    rng = np.random.default_rng([int(seed), 0xA11])
    P, a, u, v = axes(A, s)
    y = np.deg2rad(yaw_deg)
    ax = np.cos(y) * a - np.sin(y) * v
    ay = np.cross(u, ax)
    Rm = np.stack([ax, ay, u], axis=1)
    tr = P - lateral[0] * v + lateral[1] * u
    sp = s + rng.uniform(-half, half, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rho = radius + synth.wall_texture(sp, phi, seed=seed, length=length) + rng.normal(0.0, sigma, n)
    x = A.point(sp, phi, rho)
    cloud = ((x - tr) @ Rm).astype(F)
    return cloud, np.concatenate([Rm, tr.reshape(3, 1)], axis=1)


def joint_d32(xyz, jo, ja):
    """d of one joint for float32 points [n, 3]: q = p - Jo', d = fma(qx, ax, fma(qy, ay, qz az)), surf_dot3's order."""
    p = np.asarray(xyz, F)
    jo, ja = np.asarray(jo, F), np.asarray(ja, F)
    qx, qy, qz = p[:, 0] - jo[0], p[:, 1] - jo[1], p[:, 2] - jo[2]
    return f32.fma32(qx, ja[0], f32.fma32(qy, ja[1], qz * ja[2]))


def owner32(xyz, plan):
    """The device's owner of every point under the plan of gm_wall_alignment_add_plan: the element index, int32 [n]."""
    n = len(xyz)
    side = np.full(n, plan["n_sides"] - 1, np.int64)
    for k in range(plan["n_sides"] - 2, -1, -1):   # descending: the lowest joint with d < 0 stays
        side[joint_d32(xyz, plan["joint_o"][k], plan["joint_a"][k]) < 0.0] = k
    return np.asarray(plan["side_element"], np.int64)[side].astype(np.int32)


def joint_d64(xyz, pose, J, aJ):
    """The same d in fp64 from the unrounded plane, and the forward-error bound of the fp32 chain per point:
    the roundings of Jo' (sum |Jo_k a_k| u) and of aJ' (sum |q_k a_k| u), the three subtractions (sum |q_k a_k| u) and the
    three-term fma chain (at most 3 sum |q_k a_k| u), times 1.01 for the second-order terms."""
    pose = np.asarray(pose, np.float64)
    Rm, tr = pose[:, :3], pose[:, 3]
    jo = Rm.T @ (np.asarray(J, np.float64) - tr)
    a = Rm.T @ np.asarray(aJ, np.float64)
    q = np.asarray(xyz, F).astype(np.float64) - jo
    d = q @ a
    bound = 1.01 * U * (np.abs(jo) @ np.abs(a) + 5.0 * (np.abs(q) @ np.abs(a)))
    return d, bound
