"""gm_wall_alignment_* without a GPU: the symbols, the struct layouts from plain C99, and the refusals of the device-free
calls (include/gm_hip.h: a wall alignment)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_np as al_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_alignment_check", "gm_wall_alignment_element_params", "gm_wall_alignment_project", "gm_wall_alignment_point",
         "gm_wall_alignment_add_plan", "gm_wall_alignment_window", "gm_wall_alignment_create", "gm_wall_alignment_destroy",
         "gm_wall_alignment_map", "gm_wall_alignment_add_frame", "gm_wall_alignment_add_points", "gm_wall_alignment_sync",
         "gm_wall_alignment_info")
I, OK = _lib.GM_ERR_INVALID_ARG, _lib.GM_OK


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_element": _lib.WallElement,
        "gm_wall_alignment_piece": _lib.WallAlignmentPiece,
        "gm_wall_alignment_add_info": _lib.WallAlignmentAddInfo,
        "gm_wall_alignment_totals": _lib.WallAlignmentTotals,
    }
    lines = ['printf("%d %d %d %d %d\\n", GM_WALL_ALIGNMENT_MAX_ELEMENTS, GM_WALL_JOINT_MAX_SIDES, GM_WALL_ELEMENT_STRAIGHT, '
             'GM_WALL_ELEMENT_ARC, GM_WALL_ELEMENT_CLOTHOID);']
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gm_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    assert out[:5] == [256, 4, 0, 1, 2]
    want = []
    for _, ct in sorted(fields.items()):
        want.append(C.sizeof(ct))
        want += [getattr(ct, f).offset for f, _t in ct._fields_]
    assert out[5:] == want
    assert [C.sizeof(fields[k]) for k in sorted(fields)] == [160, 16, 72, 48]
    assert api.WALL_ELEMENT_KINDS == dict(straight=0, arc=1, clothoid=2)


def _check(elements, n=None, **prm):
    p = api.WallMap.params(**dict(dict(n_sectors=90, station_length=0.25, radius=2.0), **prm))
    arr, cnt = api._wall_elements(elements)
    return int(_lib.load().gm_wall_alignment_check(C.byref(p), arr, cnt if n is None else n))


def test_refusals():
    L = _lib.load()
    good = al_np.elements5()
    assert _check(good) == OK
    assert _check(good, n=0) == I and _check([good[0]] * 256) == OK
    big, _ = api._wall_elements([good[0]] * 257)
    p = api.WallMap.params(n_sectors=90)
    assert L.gm_wall_alignment_check(C.byref(p), big, 257) == I
    assert L.gm_wall_alignment_check(None, big, 1) == I and L.gm_wall_alignment_check(C.byref(p), None, 1) == I
    assert _check(good, n_stations=0) == OK                       # the template's n_stations is not read
    assert _check(good, gate=9.0) == I                            # ... the rest of it is
    for field, value in (("struct_size", 40), ("reserved", 1), ("kind", 3), ("n_stations", 0)):
        e = api.wall_element(**good[2])
        setattr(e, field, value)
        assert _check(good[:2] + [e]) == I, field
    arc = good[2]
    for bad in (dict(arc, turn=(0.0, 0.0)), dict(arc, turn=(float("nan"), 1.0)), dict(arc, curvature=-1 / 80.0),
                dict(arc, curvature=0.0), dict(arc, curvature=0.3),           # (R + gate) kappa > 0.5: gm_wall_map_create_arc's
                dict(arc, n_stations=1000),                                  # |kappa (s_end - s0)| > 3
                dict(good[1], rate=0.0), dict(good[1], turn=(0.0, 0.0)),     # gm_wall_map_create_clothoid's: an arc or a straight
                dict(good[1], curvature=float("inf"))):
        assert _check(good[:1] + [bad]) == I, bad
    assert _check([dict(kind="straight", n_stations=5, turn=(0.0, 0.0), curvature=float("nan"))]) == OK   # not read on a straight
    # the calls that take the alignment refuse what the check refuses, and their own arguments
    rule = api.WallAlignmentRule(good, n_sectors=90, station_length=0.25, radius=2.0)
    head = rule._head()
    out, el = np.zeros(3), C.c_uint32()
    d = [C.c_double() for _ in range(3)]
    dp = C.POINTER(C.c_double)
    assert L.gm_wall_alignment_point(*head, float("nan"), 0.0, 2.0, out.ctypes.data_as(dp)) == I
    assert L.gm_wall_alignment_point(*head, 1.0, 0.0, 2.0, None) == I
    x = np.array([0.0, np.inf, 0.0])
    assert L.gm_wall_alignment_project(*head, x.ctypes.data_as(dp), C.byref(el), *(C.byref(v) for v in d)) == I
    assert L.gm_wall_alignment_project(*head, out.ctypes.data_as(dp), None, *(C.byref(v) for v in d)) == I
    ep = _lib.WallParams()
    assert L.gm_wall_alignment_element_params(*head, 5, C.byref(ep), None, None) == I
    assert L.gm_wall_alignment_element_params(*head, 4, C.byref(ep), None, None) == OK and ep.n_stations == 40
    got = C.c_uint32()
    assert L.gm_wall_alignment_window(*head, 3.0, 2.0, None, 0, C.byref(got)) == I
    assert L.gm_wall_alignment_window(*head, 3.0, float("nan"), None, 0, C.byref(got)) == I
    assert L.gm_wall_alignment_window(*head, 3.0, 30.0, None, 0, C.byref(got)) == _lib.GM_ERR_CAPACITY and got.value == 3
    assert L.gm_wall_alignment_window(*head, -9.0, -3.0, None, 0, C.byref(got)) == OK and got.value == 0
    info = _lib.WallAlignmentAddInfo()
    pose = np.ascontiguousarray(np.eye(4)[:3])
    pp = pose.ctypes.data_as(dp)
    assert L.gm_wall_alignment_add_plan(*head, pp, 5.0, C.byref(info)) == OK and info.struct_size == 160
    assert L.gm_wall_alignment_add_plan(*head, pp, 0.0, C.byref(info)) == I
    assert L.gm_wall_alignment_add_plan(*head, pp, 5.0, None) == I and L.gm_wall_alignment_add_plan(*head, None, 5.0, C.byref(info)) == I
    pose[0, 0] = 2.0   # not a rotation
    assert L.gm_wall_alignment_add_plan(*head, pp, 5.0, C.byref(info)) == I
    # six 1 m elements within the reach: more sides than a launch takes
    short = [dict(kind="straight", n_stations=80)] + [dict(kind="arc", n_stations=4, turn=(0, -1), curvature=1 / 80.0)] * 6
    r2 = api.WallAlignmentRule(short, n_sectors=90, station_length=0.25, radius=2.0)
    pose = np.ascontiguousarray(np.eye(4)[:3])
    pose[0, 3] = 19.5
    with pytest.raises(_lib.GmError) as ex:
        r2.add_plan(pose, 5.0)
    assert ex.value.status == _lib.GM_ERR_UNSUPPORTED
    assert r2.add_plan(pose, 0.2)["n_sides"] == 2               # a reach of 0.94 m: 20 m, the first joint, lies within it


def test_context_calls_refuse_null():
    L = _lib.load()
    h = C.c_void_p()
    assert L.gm_wall_alignment_create(None, None, None, 0, C.byref(h)) == I
    assert L.gm_wall_alignment_map(None, 0, C.byref(h)) == I and L.gm_wall_alignment_sync(None) == I
    assert L.gm_wall_alignment_info(None, None) == I
    assert L.gm_wall_alignment_add_points(None, None, 0, None, None, None, None, None, None) == I
    L.gm_wall_alignment_destroy(None)
