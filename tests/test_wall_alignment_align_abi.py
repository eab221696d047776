"""ABI of the align on a wall alignment (gm_wall_alignment_align_*): the symbols, the structs' sizes and offsets as
include/gm_hip.h states them, against a C compiler and against the ctypes mirror, and the shared head; the device-free
plan against the twin's integers; the device-free selection and pose against the twin; a whole-station shift along an arc;
every refusal that needs no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_align_np as an  # noqa: E402
import wall_alignment_align_cases as ac  # noqa: E402
import wall_alignment_align_np as aan  # noqa: E402
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_locate_np as aln  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402
import wall_clothoid_np as wl  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gm_wall_alignment_align_plan", "gm_wall_alignment_align_select", "gm_wall_alignment_align_frame",
           "gm_wall_alignment_get_align", "gm_wall_alignment_align_points")
# |pose' - frame(A, s + a ds)'s pose| after a whole-station shift along an arc of radius 80 at chainages near 100: both
# sides compose the same frames in fp64, and the twin's frame is a difference of two points of the library (1e-14 of
# cancellation at coordinates of 100).  Measured on the twin here: 1.6e-14 over a in -6 .. 6; five times that.
WHOLE_SHIFT_BOUND = 5 * 1.6e-14


def _kinds(rule):
    eps = [rule.element_params(i) for i in range(rule.n_elements)]
    return ([int(e[0].n_stations) for e in eps],
            [aln.CLOTHOID if e[2] is not None else (aln.ARC if e[1] is not None else aln.STRAIGHT) for e in eps])


def test_symbols_exist():
    L = _lib.load()
    for name in SYMBOLS:
        assert getattr(L, name) is not None, name
    for name in ("align_frame", "align_result", "align_points", "align_plan", "align_select"):
        assert callable(getattr(api.WallAlignment, name)), name


def test_struct_sizes_and_offsets(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gm_hip.h")).read()
    assert "typedef struct gm_wall_alignment_align_info {   /* 472 bytes; the first 224 are gm_wall_align_info's" in hdr
    assert "typedef struct gm_wall_alignment_align_plan_info {   /* 336 bytes" in hdr
    assert "align (chainage and roll) and check objects through the alignment" not in hdr   # no longer out of scope
    I, Pl, Pc = _lib.WallAlignmentAlignInfo, _lib.WallAlignmentAlignPlan, _lib.WallAlignmentAlignPiece
    assert (C.sizeof(I), C.sizeof(Pl), C.sizeof(Pc), C.sizeof(_lib.WallAlignInfo)) == (472, 336, 16, 224)
    for name, _ in _lib.WallAlignInfo._fields_:   # the shared head is gm_wall_align_info, field for field
        assert getattr(I, name).offset == getattr(_lib.WallAlignInfo, name).offset, name
    assert (I.element.offset, I.n_sides.offset, I.chainage.offset, I.anchor_global.offset, I.side_class.offset, I.plan.offset) == (
        224, 228, 232, 240, 248, 312)
    assert (Pl.n_pieces.offset, Pl.add.offset, Pl.anchor_global.offset, Pl.total.offset, Pl.row0.offset, Pl.own.offset, Pl.home.offset,
            Pl.piece.offset) == (4, 8, 168, 176, 184, 200, 204, 208)
    src = tmp_path / "sizes.c"
    src.write_text('#include "gm_hip.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(gm_wall_alignment_align_info) == 472, \"size\");\n"
                   "_Static_assert(sizeof(gm_wall_alignment_align_plan_info) == 336, \"plan\");\n"
                   "_Static_assert(sizeof(gm_wall_alignment_align_piece) == 16, \"piece\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_info, element) == sizeof(gm_wall_align_info), \"head\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_info, pose) == offsetof(gm_wall_align_info, pose), \"pose\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_info, best_sector) == offsetof(gm_wall_align_info, best_sector), \"best\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_info, side_class) == 248, \"side_class\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_info, plan) == 312, \"plan\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_align_plan_info, piece) == 208, \"pieces\");\n"
                   "_Static_assert(GM_WALL_ALIGN_MAX_PIECES == 8, \"pieces\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True)


@pytest.mark.parametrize("case", ac.PARITY_CASES)
@pytest.mark.parametrize("shift", ((0, 0), (3, -2)))
def test_plan_against_the_twin(case, shift):
    """G_f, row0 per side, the pieces, total, home and the one-straight-side rule: exactly the twin's integers."""
    rule, grid, s, sides = ac.rule_of(api, case)
    nst, kinds = _kinds(rule)
    for kw in (ac.AP, dict(half_patch_stations=45, max_station_shift=64, max_sector_shift=1), dict(half_patch_stations=1, max_station_shift=0)):
        pose = ac.moved(rule, s, *shift, grid)
        got = rule.align_plan(pose, ac.BOUND, **kw)
        add = rule.add_plan(pose, ac.BOUND)
        assert all(np.array_equal(got["add"][q], add[q]) for q in add) and add["n_sides"] == sides
        tp = aan.plan(add, nst, kinds, an.prm(**kw))
        assert (got["anchor_global"], got["total"], got["home"], got["own"]) == (tp["anchor_global"], tp["total"], tp["home"], tp["own"])
        assert got["row0"].tolist() == tp["row0"].tolist() and got["pieces"] == tp["pieces"] and got["n_pieces"] == len(tp["pieces"])


def _table(ap, best, n=500, ssd=10 ** 9, neighbours=()):
    """A table whose only valid shifts are `best` (a, b) and `neighbours` [(a, b, ssd)]."""
    A, B = ap["max_station_shift"], ap["max_sector_shift"]
    t = np.zeros((2 * A + 1, 2 * B + 1), an.SCORE)
    t[best[0] + A, best[1] + B] = (ssd, -12345, n, 0)
    for a, b, q in neighbours:
        t[a + A, b + B] = (q, 777, n, 0)
    return t


@pytest.mark.parametrize("case", ac.PARITY_CASES)
def test_select_against_the_twin(case):
    """The selection's scalars to rtol 1e-14 and the pose to atol 1e-12 (test_gpu_wall_align.py's tolerances for select):
    both sides evaluate the library's frames."""
    rule, grid, s, _ = ac.rule_of(api, case)
    nst, kinds = _kinds(rule)
    ap = ac.prm()
    pose = ac.moved(rule, s, 1, 1, grid)
    add = rule.add_plan(pose, ac.BOUND)
    tp = aan.plan(add, nst, kinds, ap)
    for tab in (_table(ap, (3, -2), neighbours=((2, -2, 3 * 10 ** 9), (4, -2, 2 * 10 ** 9), (3, -1, 4 * 10 ** 9), (3, -3, 2 * 10 ** 9), (-5, 3, 10 ** 10))),
                _table(ap, (-6, 4)), _table(ap, (0, 0), n=10)):
        got = rule.align_select(pose, ac.BOUND, tab, **ac.AP)
        want = aan.select(tab, rule, pose, add, tp, grid, ap)
        for k in ("status", "anchor_station", "overlap", "best_station", "best_sector"):
            assert got[k] == want[k], (k, got[k], want[k])
        for k in ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction"):
            assert np.isclose(got[k], want[k], rtol=1e-14, atol=0.0, equal_nan=True), (k, got[k], want[k])
        assert np.allclose(got["pose"], want["pose"], rtol=0.0, atol=1e-12, equal_nan=True)
        assert (got["element"], got["n_sides"], got["chainage"], got["anchor_global"]) == (add["element"], add["n_sides"], add["chainage"],
                                                                                          tp["anchor_global"])
        assert got["n_points"] == 0 and not got["side_class"].any()
        if got["status"] & _lib.GM_ALIGN_FAILED_MASK:
            assert np.all(np.isnan(got["pose"]))
        else:
            assert wn.pose_ok(got["pose"])   # the library's own pose check


def test_pose_on_a_clothoid_against_the_clothoid_twin():
    """F(s), F(s') from wall_clothoid_np.frame on the element's derived structs: test_wall_clothoid_np.py's tolerance for the
    frame (1e-12 relative)."""
    rule, grid, s, _ = ac.rule_of(api, "clothoid")   # mid-clothoid, one side
    ep, _, cl = rule.element_params(1)
    p = wn.params(n_stations=ep.n_stations, n_sectors=ep.n_sectors, station_length=ep.station_length, radius=ep.radius, t_min=ep.t_min,
                  point=list(ep.point), direction=list(ep.direction), up=list(ep.up), forward=list(ep.forward))
    D = wl.design(p, dict(normal=list(cl.normal), curvature=cl.curvature, rate=cl.rate, point_chainage=cl.point_chainage))
    ap = ac.prm()
    pose = ac.moved(rule, s, 0, 0, grid)
    add = rule.add_plan(pose, ac.BOUND)
    assert add["element"] == 1 and add["n_sides"] == 1
    got = rule.align_select(pose, ac.BOUND, _table(ap, (5, -3)), **ac.AP)
    P1, a1, u1, v1, _ = wl.frame(D, add["chainage"])
    P2, a2, u2, v2, _ = wl.frame(D, add["chainage"] + got["shift_m"])
    c, sn = np.cos(got["roll"]), np.sin(got["roll"])
    M = np.stack([a2, u2, v2], axis=1) @ np.array([[1.0, 0, 0], [0, c, -sn], [0, sn, c]]) @ np.stack([a1, u1, v1], axis=1).T
    want = np.concatenate([M @ pose[:, :3], (P2 + M @ (pose[:, 3] - P1)).reshape(3, 1)], axis=1)
    assert (got["shift_m"], got["roll"]) == (5 * 0.25, -3 * (2 * np.pi / 90))
    assert np.abs(got["pose"] - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def test_a_whole_station_shift_along_an_arc():
    """pose' is the pose wall_alignment_np.frame gives at s + a ds, with the same lateral offset and yaw."""
    rule, grid, s, _ = ac.rule_of(api, "arc")   # mid-arc of radius 80, chainage 100
    ap = ac.prm()
    _, pose = al_np.frame(rule, s, 1, seed=0)
    worst = 0.0
    for a in range(-6, 7):
        got = rule.align_select(pose, ac.BOUND, _table(ap, (a, 0)), **ac.AP)
        assert got["status"] & ~_lib.GM_ALIGN_AT_BORDER == _lib.GM_ALIGN_OK and got["shift_m"] == a * 0.25
        _, want = al_np.frame(rule, s + a * 0.25, 1, seed=0)
        worst = max(worst, float(np.abs(got["pose"] - want).max()))
    print("worst |pose' - frame(s + a ds)|:", worst)
    assert worst <= WHOLE_SHIFT_BOUND


def test_refusals_without_a_device():
    L = _lib.load()
    I, U = _lib.GM_ERR_INVALID_ARG, _lib.GM_ERR_UNSUPPORTED
    rule, grid, s, _ = ac.rule_of(api, "clothoid_arc:before")
    pose = ac.moved(rule, s, 0, 0, grid)
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    plan, info = _lib.WallAlignmentAlignPlan(), _lib.WallAlignmentAlignInfo()
    prm = api.WallMap.align_params(**ac.AP)
    tab = _table(ac.prm(), (0, 0))
    tp = tab.ctypes.data_as(C.POINTER(_lib.WallAlignScore))
    head = rule._head()
    # NULLs
    assert L.gm_wall_alignment_align_plan(*head, dp, ac.BOUND, C.byref(prm), None) == I
    assert L.gm_wall_alignment_align_plan(*head, None, ac.BOUND, C.byref(prm), C.byref(plan)) == I
    assert L.gm_wall_alignment_align_plan(None, head[1], head[2], dp, ac.BOUND, C.byref(prm), C.byref(plan)) == I
    assert L.gm_wall_alignment_align_plan(head[0], None, head[2], dp, ac.BOUND, C.byref(prm), C.byref(plan)) == I
    assert L.gm_wall_alignment_align_plan(*head, dp, ac.BOUND, None, C.byref(plan)) == _lib.GM_OK   # NULL parameters: the defaults
    assert plan.struct_size == 336 and plan.add.n_sides == 2
    assert L.gm_wall_alignment_align_select(*head, dp, ac.BOUND, C.byref(prm), None, tab.size, C.byref(info)) == I
    assert L.gm_wall_alignment_align_select(*head, dp, ac.BOUND, C.byref(prm), tp, tab.size, None) == I
    assert L.gm_wall_alignment_align_select(*head, None, ac.BOUND, C.byref(prm), tp, tab.size, C.byref(info)) == I
    assert L.gm_wall_alignment_align_select(*head, dp, ac.BOUND, C.byref(prm), tp, tab.size - 1, C.byref(info)) == I   # a wrong n_scores
    assert L.gm_wall_alignment_align_select(*head, dp, ac.BOUND, C.byref(prm), tp, tab.size, C.byref(info)) == _lib.GM_OK
    assert info.struct_size == 472
    assert L.gm_wall_alignment_align_frame(None, None, 0, dp, None, None) == I
    assert L.gm_wall_alignment_get_align(None, 0, C.byref(info), None, 0, None) == I
    assert L.gm_wall_alignment_align_points(None, None, 0, None, dp, None, None, C.byref(info), None, 0, None, None, None, None) == I
    # bad parameters (gm_wall_align_check_params' on the alignment's 90 sectors), a bad bound, a bad pose
    for bad in (dict(half_patch_stations=0), dict(half_patch_stations=46), dict(max_station_shift=65), dict(max_sector_shift=45),
                dict(max_station_shift=64, max_sector_shift=16), dict(min_count=0), dict(min_frame_count=0), dict(min_overlap=0),
                dict(gate=0.0), dict(gate=9.0), dict(gate=float("nan")), dict(clip=0.0), dict(clip=1e-9), dict(min_distinction=0.5),
                dict(min_distinction=float("inf"))):
        with pytest.raises(_lib.GmError) as ex:
            rule.align_plan(pose, ac.BOUND, **bad)
        assert ex.value.status == I, bad
        with pytest.raises(_lib.GmError) as ex:
            rule.align_select(pose, ac.BOUND, tab, **bad)
        assert ex.value.status == I, bad
    wrong = api.WallMap.align_params(**ac.AP)
    wrong.struct_size = 48
    assert L.gm_wall_alignment_align_plan(*head, dp, ac.BOUND, C.byref(wrong), C.byref(plan)) == I
    for bound in (0.0, -1.0, float("nan"), float("inf")):
        assert L.gm_wall_alignment_align_plan(*head, dp, bound, C.byref(prm), C.byref(plan)) == I
    skew = pose.copy()
    skew[0, 0] = np.nan
    with pytest.raises(_lib.GmError) as ex:
        rule.align_plan(skew, ac.BOUND, **ac.AP)
    assert ex.value.status == I
    # too many sides: six 1 m elements in a row
    many = api.WallAlignmentRule(lc.ENDS + [dict(kind="arc", n_stations=4, turn=lc.T, curvature=lc.K80)] * 6 + lc.ENDS, **lc.prm())
    _, pose6 = al_np.frame(many, 23.0, 1, seed=0)
    with pytest.raises(_lib.GmError) as ex:
        many.align_plan(pose6, ac.BOUND, **ac.AP)
    assert ex.value.status == U
    with pytest.raises(_lib.GmError) as ex:
        many.align_select(pose6, ac.BOUND, tab, **ac.AP)
    assert ex.value.status == U
    # nine pieces, built from one-station elements, under a bound whose reach (2 sqrt(3) 0.01 + 0.25 = 0.28 m) meets three
    # of them: eight pieces are accepted, nine are not
    one = dict(kind="arc", n_stations=1, turn=lc.T, curvature=lc.K80)
    for n_el, want in ((8, _lib.GM_OK), (9, U)):
        tiny = api.WallAlignmentRule([one] * n_el, **lc.prm())
        _, pose9 = al_np.frame(tiny, 1.1, 1, seed=0, lateral=(0.0, 0.0), yaw_deg=0.0)
        p9 = _lib.WallAlignmentAlignPlan()
        pd = np.ascontiguousarray(pose9).ctypes.data_as(C.POINTER(C.c_double))
        st = L.gm_wall_alignment_align_plan(*tiny._head(), pd, 0.01, C.byref(prm), C.byref(p9))
        assert st == want, (n_el, st)
        assert p9.add.n_sides == 3 and p9.n_pieces == (8 if want == _lib.GM_OK else 0)
