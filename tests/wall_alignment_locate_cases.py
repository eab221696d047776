"""What the CPU and the GPU tests of the alignment's locate share: the alignments and frames of the alignment tests (4 000
points, 90 sectors, ds 0.25, the elements5 / COMPOUND alignments and their five joints), the perturbation of
test_truth_of_a_perturbed_drive, the error measures of a located pose on a curved axis, and the truth test's bounds."""
import numpy as np

import wall_alignment_np as al_np
from geometric_mapping_amd import synth

N = 4000
K80 = 1.0 / 80.0
T = al_np.LEFT
SURVEY_OFFSETS = (-2.5, -1.0, 1.0, 2.5)   # a MAP test's survey: frames of the same wall around the located one
TRUTH_SEED = 9
DESIGN, MAP = 0, 1


def prm(**kw):
    return dict(dict(n_sectors=90, station_length=al_np.DS, radius=al_np.RADIUS), **kw)


def long5(n=80, ds=al_np.DS):
    """straight - clothoid - arc - clothoid - straight with elements longer than the reach."""
    return al_np.elements5(n_straight=n, n_clothoid=n, n_arc=n, ds=ds)


COMPOUND = [dict(kind="arc", n_stations=80, turn=T, curvature=K80), dict(kind="arc", n_stations=80, turn=T, curvature=1.0 / 50.0)]
JOINTS = {
    "straight_clothoid": (long5(), 0), "clothoid_arc": (long5(), 1), "arc_clothoid": (long5(), 2),
    "clothoid_straight": (long5(), 3), "arc_arc": (COMPOUND, 0),
}
SHORT = [dict(kind="arc", n_stations=8, turn=T, curvature=K80), dict(kind="clothoid", n_stations=8, turn=T, curvature=K80, rate=-K80 / 2.0)]
ENDS = [dict(kind="straight", n_stations=80)]
LONE = al_np.elements5(n_straight=160, n_clothoid=160, n_arc=160)[:3]   # 40 m each: mid-element frames see one side

RECORD_CASES = ("arc", "clothoid") + tuple(f"{k}:{w}" for k in sorted(JOINTS) for w in ("before", "after")) + ("three_sides", "four_sides")
MAP_RECORD_CASES = ("arc", "clothoid_arc:before", "straight_clothoid:after")


def record_case(case):
    """(elements, the sensor's chainage, the sides the plan must have)."""
    if case == "arc":
        return LONE, 100.0, 1
    if case == "clothoid":
        return LONE, 60.0, 1
    if case == "three_sides":
        return ENDS + SHORT[:1] + ENDS, 21.0 - 1.5, 3
    if case == "four_sides":
        return ENDS + SHORT + ENDS, 22.0 + 1.5, 4
    name, where = case.split(":")
    els, j = JOINTS[name]
    return els, al_np.spans(els)[j][1] + (-1.0 if where == "before" else 1.0), 2


def truth_frames():
    """(name, elements, chainage): every joint frame, and one frame in mid-arc and in mid-clothoid."""
    out = [(c, *record_case(c)[:2]) for c in RECORD_CASES if ":" in c]
    return out + [("arc", LONE, 100.0), ("clothoid", LONE, 60.0)]


def perturbed(pose, rng, lateral=0.05, angle_deg=0.5):
    """test_gpu_wall_locate.py's: tr moved by up to +-lateral in y and z, Rm right-multiplied by a yaw and a pitch of up
    to +-angle_deg."""
    dy, dz = rng.uniform(-lateral, lateral, 2)
    yaw, pitch = rng.uniform(-angle_deg, angle_deg, 2)
    out = np.array(pose, np.float64)
    out[:, :3] = out[:, :3] @ synth.pose_matrix((0, 0, 0), yaw_deg=yaw, pitch_deg=pitch)[:, :3]
    out[1, 3] += dy
    out[2, 3] += dz
    return out


def truth_input(rule, name, s):
    """(cloud, the true pose, the perturbed pose) of a truth frame."""
    cloud, true = al_np.frame(rule, s, N, seed=TRUTH_SEED)
    k = [t[0] for t in truth_frames()].index(name)
    return cloud, true, perturbed(true, np.random.default_rng([TRUTH_SEED, k]))


def pose_errors(rule, got, true, pin):
    """(lateral: |tr' - tr_true| perpendicular to the axis at the true sensor position; angle between Rm'^T a and
    Rm_true^T a for that axis direction a; |chainage of tr' - chainage of the caller's tr|, by WallAlignmentRule.project)."""
    s_true = rule.project(true[:, 3])[1][0]
    _, a, _, _ = al_np.axes(rule, s_true)
    a = a / np.linalg.norm(a)
    dt = got[:, 3] - true[:, 3]
    d1, d2 = got[:, :3].T @ a, true[:, :3].T @ a
    ch = abs(rule.project(got[:, 3])[1][0] - rule.project(pin[:, 3])[1][0])
    return float(np.linalg.norm(dt - (dt @ a) * a)), float(np.arctan2(np.linalg.norm(np.cross(d1, d2)), d1 @ d2)), float(ch)


# (lateral m, angle rad, chainage m) per reference: the fp64 twin's worst over truth_frames(), rounded up in the third digit;
# tests/test_wall_alignment_locate_np.py computes them and asserts these constants against what it finds (DESIGN: 5.924e-3,
# 1.418e-3, 1.110e-4; MAP: 1.901e-4, 2.641e-4, 1.114e-4).  In DESIGN mode the floor is the wall's own texture, which a frame
# of 9 m does not average out; in MAP mode it is the 5 mm noise of 4 000 points.  The GPU test's bounds are five times these.
TWIN_WORST = {DESIGN: (5.93e-3, 1.42e-3, 1.12e-4), MAP: (1.91e-4, 2.65e-4, 1.12e-4)}
TRUTH_BOUNDS = {k: tuple(5.0 * x for x in v) for k, v in TWIN_WORST.items()}
