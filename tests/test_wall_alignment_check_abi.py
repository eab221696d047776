"""ABI of the check and the checked add on a wall alignment (gm_wall_alignment_check_*, gm_wall_alignment_add_*_checked):
the symbols, the struct's size and offsets as include/gm_hip.h states them, against a C compiler and against the ctypes
mirror; the refusals that need no device; and, on a device, the refusals that need an alignment."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gm_wall_alignment_check_frame", "gm_wall_alignment_get_check", "gm_wall_alignment_check_points",
           "gm_wall_alignment_add_frame_checked", "gm_wall_alignment_get_add_checked", "gm_wall_alignment_add_points_checked")


def test_symbols_exist():
    L = _lib.load()
    for name in SYMBOLS:
        assert getattr(L, name) is not None, name
    for name in ("check_frame", "check_result", "check_points", "add_frame_checked", "add_checked_result", "add_points_checked",
                 "split_cell"):
        assert callable(getattr(api.WallAlignment, name)), name


def test_struct_size_and_offsets(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gm_hip.h")).read()
    assert "typedef struct gm_wall_alignment_check_info {   /* 184 bytes" in hdr
    I = _lib.WallAlignmentCheckInfo
    assert C.sizeof(I) == 184 and C.sizeof(_lib.WallCheckInfo) == 64 and C.sizeof(_lib.WallCheckPoint) == 32
    # the shared head is gm_wall_check_info, field for field
    for name, _ in _lib.WallCheckInfo._fields_:
        assert getattr(I, name).offset == getattr(_lib.WallCheckInfo, name).offset, name
    assert (I.n_sides.offset, I.reserved.offset, I.side_class.offset) == (64, 68, 72)
    src = tmp_path / "sizes.c"
    src.write_text('#include "gm_hip.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(gm_wall_alignment_check_info) == 184, \"size\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_check_info, n_sides) == sizeof(gm_wall_check_info), \"head\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_check_info, peak_neg) == offsetof(gm_wall_check_info, peak_neg), \"peaks\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_check_info, side_class) == 72, \"side_class\");\n"
                   "_Static_assert(sizeof(((gm_wall_alignment_check_info *)0)->side_class) == 4 * GM_WALL_JOINT_MAX_SIDES * GM_WALL_CHECK_N_CLS, \"classes\");\n"
                   "_Static_assert(GM_WALL_ROW_SIDE(3 << 24 | 77) == 3 && GM_WALL_ROW_CELL(3 << 24 | 77) == 77, \"row\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True)


def test_split_cell():
    rows = np.zeros(3, api.WALL_CHECK_POINT)
    rows["cell"] = np.array([5, (1 << 24) | 7, (3 << 24) | 0xFFFFFF], np.uint32).view(np.int32)
    side, cell = api.WallAlignment.split_cell(rows)
    assert list(side) == [0, 1, 3] and list(cell) == [5, 7, 0xFFFFFF]


def test_null_refusals_without_a_device():
    L = _lib.load()
    I = _lib.GM_ERR_INVALID_ARG
    pose = np.ascontiguousarray(np.eye(4)[:3])
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    ci, ai = _lib.WallAlignmentCheckInfo(), _lib.WallAddCheckedInfo()
    assert L.gm_wall_alignment_check_frame(None, None, 0, dp, None, None) == I
    assert L.gm_wall_alignment_get_check(None, 0, C.byref(ci), None, 0, None) == I
    assert L.gm_wall_alignment_check_points(None, None, 0, None, dp, None, None, C.byref(ci), None, 0, None, None, None, None, None, None) == I
    assert L.gm_wall_alignment_add_frame_checked(None, None, 0, dp, None, None) == I
    assert L.gm_wall_alignment_get_add_checked(None, 0, C.byref(ai)) == I
    assert L.gm_wall_alignment_add_points_checked(None, None, 0, None, dp, None, None, 0, None, C.byref(ai), None, None, None) == I


@pytest.mark.gpu
def test_refusals_on_an_alignment(gm):
    els, j = lc.JOINTS["clothoid_arc"]
    p = lc.prm()
    I, NR = _lib.GM_ERR_INVALID_ARG, _lib.GM_ERR_NOT_READY
    sj = al_np.spans(els)[j][1]
    with gm.GeometricMapping() as c, gm.GeometricMapping() as other:
        al = c.wall_alignment(els, **p)
        cloud, pose = al_np.frame(al, sj - 1.0, 200, seed=1)
        L = c._L
        dp = pose.ctypes.data_as(C.POINTER(C.c_double))
        ci, ai = _lib.WallAlignmentCheckInfo(), _lib.WallAddCheckedInfo()
        # no frame in the slot, no check, no checked add
        assert L.gm_wall_alignment_check_frame(al._al, c._ctx, 0, dp, None, None) == NR
        assert L.gm_wall_alignment_add_frame_checked(al._al, c._ctx, 0, dp, None, None) == NR
        assert L.gm_wall_alignment_get_check(al._al, 0, C.byref(ci), None, 0, None) == NR
        assert L.gm_wall_alignment_get_add_checked(al._al, 0, C.byref(ai)) == NR
        # NULLs, a foreign context, a slot out of range
        assert L.gm_wall_alignment_check_frame(al._al, None, 0, dp, None, None) == I
        assert L.gm_wall_alignment_check_frame(al._al, other._ctx, 0, dp, None, None) == I
        assert L.gm_wall_alignment_check_frame(al._al, c._ctx, 7, dp, None, None) == I
        assert L.gm_wall_alignment_add_frame_checked(al._al, other._ctx, 0, dp, None, None) == I
        assert L.gm_wall_alignment_add_frame_checked(al._al, c._ctx, 7, dp, None, None) == I
        assert L.gm_wall_alignment_get_check(al._al, 7, C.byref(ci), None, 0, None) == I
        assert L.gm_wall_alignment_get_add_checked(al._al, 7, C.byref(ai)) == I
        assert L.gm_wall_alignment_get_add_checked(al._al, 0, None) == I
        assert L.gm_wall_alignment_check_points(al._al, None, 5, None, dp, None, None, C.byref(ci), None, 0, None, None, None, None, None, None) == I
        assert L.gm_wall_alignment_add_points_checked(al._al, None, 5, None, dp, None, None, 0, None, None, None, None, None) == I
        c.process_frame(cloud)
        assert L.gm_wall_alignment_check_frame(al._al, c._ctx, 0, None, None, None) == I   # NULL pose
        assert L.gm_wall_alignment_add_frame_checked(al._al, c._ctx, 0, dp, None, None) == NR   # a frame, but no check of it
        # gm_wall_check_params' and gm_wall_add_checked_params' refusals, unchanged
        for bad in (dict(threshold=0.0), dict(threshold=9.0), dict(gate=float("nan")), dict(min_count=0), dict(reference=2)):
            with pytest.raises(_lib.GmError) as ex:
                al.check_frame(0, pose, **bad)
            assert ex.value.status == I, bad
            with pytest.raises(_lib.GmError) as ex:
                al.check_points(cloud, pose, **bad)
            assert ex.value.status == I, bad
        al.check_frame(0, pose)
        for bad in (dict(skip=0), dict(skip=4), dict(min_delta=-1.0), dict(min_delta=9.0)):
            with pytest.raises(_lib.GmError) as ex:
                al.add_frame_checked(0, pose, **bad)
            assert ex.value.status == I, bad
            with pytest.raises(_lib.GmError) as ex:
                al.add_points_checked(cloud, pose, np.zeros(0, api.WALL_CHECK_POINT), **bad)
            assert ex.value.status == I, bad
        skew = pose.copy()
        skew[0, 0] = np.nan
        with pytest.raises(_lib.GmError) as ex:
            al.check_points(cloud, skew)
        assert ex.value.status == I
        assert al.info()["frames"] == 0
        # six 1 m elements in a row: more sides than a launch takes; nothing is enqueued
        many = lc.ENDS + [dict(kind="arc", n_stations=4, turn=lc.T, curvature=lc.K80)] * 6 + lc.ENDS
        a6 = c.wall_alignment(many, **p)
        cloud6, pose6 = al_np.frame(a6, 23.0, 200, seed=23)
        for call in (lambda: a6.check_points(cloud6, pose6), lambda: a6.check_frame(0, pose6), lambda: a6.add_frame_checked(0, pose6),
                     lambda: a6.add_points_checked(cloud6, pose6, np.zeros(0, api.WALL_CHECK_POINT))):
            with pytest.raises(_lib.GmError) as ex:
                call()
            assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
        assert L.gm_wall_alignment_get_check(a6._al, 0, C.byref(ci), None, 0, None) == NR
        assert a6.info()["frames"] == 0
