"""What the CPU and the GPU tests of the alignment's align share: the grids and cases of wall_alignment_locate_cases, a
textured wall seen from a chainage (the texture of test_gpu_wall_align.py, drawn over the whole alignment), the pose a
caller holds that is a stations and b sectors short, a twin-made survey, and the truth tests' constants."""
import numpy as np

import wall_align_np as an
import wall_alignment_align_np as aan
import wall_alignment_locate_cases as lc
import wall_alignment_locate_np as aln
import wall_alignment_np as al_np
from geometric_mapping_amd import synth

F = np.float32
N = lc.N
BOUND = 5.0                                # boxFilterBound of the alignment tests
TEX = dict(seed=5, amplitude=0.04)         # test_gpu_wall_align.py's TEX; its length becomes the alignment's
SIGMA = 0.005
# a frame's 4.5 m of reach is 18 stations; 4 000 points on 36 x 90 patch cells are about one per cell
AP = dict(half_patch_stations=18, max_station_shift=6, max_sector_shift=4, min_count=2, min_frame_count=1, min_overlap=64)
JOINT_CASES = tuple(f"{k}:{w}" for k in sorted(lc.JOINTS) for w in ("before", "after"))
PARITY_CASES = JOINT_CASES + ("three_sides", "four_sides", "arc", "clothoid")
TRUTH_CASES = ("clothoid_arc:before", "straight_clothoid:after")
WHOLE = ((3, 2), (-2, -1), (0, 0), (5, 0))            # test_gpu_wall_align.py's
FRACTIONAL = ((1.3, -0.4), (-2.25, 1.7), (0.4, 0.3))  # test_gpu_wall_align.py's
SURVEY_OFFSETS = (-3.0, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0)
# The truth tests name their counts: a survey of nine frames of 16 000 points and a frame of 32 000, about ten points per
# patch cell.  On 90 sectors a sector is 0.14 m of arc, well inside the texture's widths: with one point per cell the shifts
# two cells apart are told apart by less than min_distinction (the twin: 1.2 .. 1.7 at 4 000 points, 1.5 .. 6 here).
TRUTH_N, SURVEY_N, TRUTH_SEED = 32000, 16000, 7
# The fp64 twin's worst errors over TRUTH_CASES x FRACTIONAL (align() of the twin on a twin-made survey;
# tests/test_wall_alignment_align_np.py computes them and asserts these constants against what it finds: 0.0273 cell of
# chainage, 0.0568 cell of roll), rounded up in the third digit.  The GPU test's bounds are five times these, never more
# than half a cell.
TWIN_WORST_STATION, TWIN_WORST_SECTOR = 0.028, 0.057
BOUND_STATION, BOUND_SECTOR = min(5 * TWIN_WORST_STATION, 0.5), min(5 * TWIN_WORST_SECTOR, 0.5)
# Closing the loop (clothoid_arc:before, the truth frame, the caller two stations and one sector off; the check with
# LOOP_CHECK: a threshold of three noise sigmas, under the texture's 0.04 m): the twin's changed points under the twin's
# aligned pose, under the true pose and under the caller's pose (tests/test_wall_alignment_align_np.py computes them and
# asserts these constants).
LOOP_SHIFT = (2, 1)
LOOP_CHECK = dict(min_count=2, threshold=0.015, gate=0.25)
LOOP_TWIN_ALIGNED, LOOP_TWIN_TRUE, LOOP_TWIN_OFF = 168, 176, 3705


def rule_of(api, case):
    """(WallAlignmentRule, grid, the sensor's chainage, the sides the plan must have)."""
    els, s, sides = lc.record_case(case)
    p = lc.prm()
    return api.WallAlignmentRule(els, **p), dict(p), s, sides


def length_of(rule):
    return float(sum(rule.element_params(i)[0].n_stations for i in range(rule.n_elements))) * al_np.DS


def textured_frame(A, s, n, seed, tex=TEX, half=4.5, sigma=SIGMA):
    """wall_alignment_np.frame on the textured wall TEX: (cloud float32 [n, 3] in sensor coordinates, the true pose).  The
    wall is fixed by `tex`; `seed` draws the points and the noise.  tex None: a smooth lining."""
    rng = np.random.default_rng([int(seed), 0xA116])
    _, pose = al_np.frame(A, s, 1, seed=0)
    sp = s + rng.uniform(-half, half, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rho = al_np.RADIUS + rng.normal(0.0, sigma, n)
    if tex is not None:
        rho = rho + synth.wall_texture(sp, phi, length=length_of(A), **tex)
    x = A.point(sp, phi, rho)
    return ((x - pose[:, 3]) @ pose[:, :3]).astype(F), pose


def moved(A, s, sa, sb, grid):
    """The pose a caller holds whose chainage is sa stations short and whose roll is sb sectors short of the frame seen
    from s: frame(A, s - sa ds)'s pose, rolled by -sb sectors about the axis there."""
    x = s - sa * float(grid["station_length"])
    _, pose = al_np.frame(A, x, 1, seed=0)
    return aan.pose(A, pose, x, 0.0, -sb * 2.0 * np.pi / int(grid["n_sectors"]))


def twin_survey(rule, grid, s, n=SURVEY_N, offsets=SURVEY_OFFSETS, tex=TEX):
    """Twin-made raw cells per element (None: never surveyed) of the textured wall around s."""
    nst_of = lambda i: rule.element_params(i)[0].n_stations   # noqa: E731
    raws = aln.survey_raws(survey_frames(rule, s, n, offsets, tex), rule, grid, nst_of, BOUND)
    return [raws.get(i) for i in range(rule.n_elements)]


def survey_frames(rule, s, n=SURVEY_N, offsets=SURVEY_OFFSETS, tex=TEX):
    """The survey's frames [(cloud, pose)]: what twin_survey bins, for a device to add."""
    return [textured_frame(rule, s + d, n, seed=100 + k, tex=tex) for k, d in enumerate(offsets)]


def twin_changed(rule, grid, raws, cloud, pose, **kw):
    """The check twin's changed points of `cloud` under `pose` against per-element raws (None: never surveyed)."""
    import wall_alignment_check_np as acn
    import wall_np as wn
    lp = rule.locate_plan(pose, BOUND)
    se = lp["add"]["side_element"]
    nst = [rule.element_params(i)[0].n_stations for i in se]
    rs = [raws[i] if raws[i] is not None else np.zeros(nst[k] * int(grid["n_sectors"]), wn.RAW_CELL) for k, i in enumerate(se)]
    info = acn.check(cloud, None, lp, grid, nst, rs, **kw)["info"]
    return info["changed_pos"] + info["changed_neg"]


def shift_error(info, sa, sb):
    """(|chainage error| in stations, |roll error| in sectors) of an align's info against the true shift."""
    return abs(info["best_station"] + info["frac_station"] - sa), abs(info["best_sector"] + info["frac_sector"] - sb)


def prm(**kw):
    return an.prm(**dict(AP, **kw))
