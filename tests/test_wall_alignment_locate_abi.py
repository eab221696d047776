"""ABI and host-only calls of the locate on a wall alignment (gm_wall_alignment_locate_*): the structs' sizes as
include/gm_hip.h states them, against a C compiler and against the ctypes mirror; the refusals that need no device; the
device-free plan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_alignment_locate_cases as lc  # noqa: E402
import wall_alignment_np as al_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(gm_wall_alignment_locate_pass=376, gm_wall_alignment_locate_info=1448, gm_wall_alignment_locate_start=1008)


def test_struct_sizes(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "gm_hip.h")).read()
    for name, size in SIZES.items():
        assert f"typedef struct {name} {{   /* {size} bytes" in hdr, name
    assert C.sizeof(_lib.WallAlignmentLocatePass) == 376 and C.sizeof(_lib.WallAlignmentLocateInfo) == 1448
    assert C.sizeof(_lib.WallAlignmentLocateStart) == 1008
    # the shared heads: gm_wall_locate_info's first 152 bytes, gm_wall_locate_pass's 112
    assert _lib.WallAlignmentLocateInfo.element.offset == _lib.WallLocateInfo.pass_.offset == 152
    assert _lib.WallAlignmentLocatePass.side.offset == C.sizeof(_lib.WallLocatePass) == 112
    assert _lib.WallAlignmentLocateInfo.pass_.offset == 320
    src = tmp_path / "sizes.c"
    src.write_text('#include "gm_hip.h"\n#include <stddef.h>\n' +
                   "".join(f"_Static_assert(sizeof({n}) == {s}, \"{n}\");\n" for n, s in SIZES.items()) +
                   "_Static_assert(offsetof(gm_wall_alignment_locate_info, element) == offsetof(gm_wall_locate_info, pass), \"head\");\n"
                   "_Static_assert(offsetof(gm_wall_alignment_locate_pass, side) == sizeof(gm_wall_locate_pass), \"pass head\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True)


def test_refusals_without_a_device():
    L = _lib.load()
    I = _lib.GM_ERR_INVALID_ARG
    pose = np.ascontiguousarray(np.eye(4)[:3])
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    info = _lib.WallAlignmentLocateInfo()
    assert L.gm_wall_alignment_locate_frame(None, None, 0, dp, None) == I
    assert L.gm_wall_alignment_get_locate(None, 0, C.byref(info)) == I
    assert L.gm_wall_alignment_locate_points(None, None, 0, None, dp, None, C.byref(info), None, None, None) == I
    p = api.WallMap.locate_params()
    assert L.gm_wall_locate_check_params(C.byref(p)) == _lib.GM_OK
    for bad in (dict(gate=9.0), dict(gate=float("nan")), dict(min_count=0), dict(reference=2)):
        assert L.gm_wall_locate_check_params(C.byref(api.WallMap.locate_params(**bad))) == I, bad
    rule = api.WallAlignmentRule(lc.JOINTS["clothoid_arc"][0], **lc.prm())
    start = _lib.WallAlignmentLocateStart()
    assert L.gm_wall_alignment_locate_plan(*rule._head(), dp, 5.0, None) == I
    assert L.gm_wall_alignment_locate_plan(*rule._head(), None, 5.0, C.byref(start)) == I
    assert L.gm_wall_alignment_locate_plan(*rule._head(), dp, 0.0, C.byref(start)) == I
    assert L.gm_wall_alignment_locate_plan(None, rule._els, rule.n_elements, dp, 5.0, C.byref(start)) == I
    skew = pose.copy()
    skew[0, 0] = 1.1
    with pytest.raises(_lib.GmError) as ex:
        rule.locate_plan(skew, 5.0)
    assert ex.value.status == I
    # six 1 m elements in a row: more sides than a launch takes
    many = lc.ENDS + [dict(kind="arc", n_stations=4, turn=lc.T, curvature=lc.K80)] * 6 + lc.ENDS
    r6 = api.WallAlignmentRule(many, **lc.prm())
    _, pose6 = al_np.frame(r6, 23.0, 8, seed=23)
    with pytest.raises(_lib.GmError) as ex:
        r6.locate_plan(pose6, 5.0)
    assert ex.value.status == _lib.GM_ERR_UNSUPPORTED


def test_plan():
    els, j = lc.JOINTS["clothoid_arc"]
    rule = api.WallAlignmentRule(els, **lc.prm())
    sj = al_np.spans(els)[j][1]
    for s, home in ((sj - 1.0, 0), (sj + 1.0, 1)):
        _, pose = al_np.frame(rule, s, 8, seed=2)
        plan = rule.locate_plan(pose, 5.0)
        add = rule.add_plan(pose, 5.0)
        assert plan["home"] == home and plan["add"]["side_element"] == [j, j + 1] and plan["side_kind"] == [2, 1]
        assert all(np.array_equal(plan["add"][q], add[q]) for q in add)
        assert plan["side"].shape == (2, 4, 3) and plan["joint"].shape == (1, 2, 3) and plan["side_axis"].shape == (2, 6)
        # the home section is the alignment's own at the anchor chainage, and orthonormal
        sf = 0.25 * plan["add"]["side_anchor"][home] + al_np.spans(els)[j + home][0]
        P, a, u, v = al_np.axes(rule, sf)
        assert np.abs(plan["o_f"] - P).max() <= 1e-9 and np.abs(plan["a"] - a).max() <= 1e-9
        assert np.abs(plan["fu"] - u).max() <= 1e-9 and np.abs(plan["fv"] - v).max() <= 1e-9
        # the attached vectors: unit directions, the other side's origin within the reach, the joint on the axis
        assert np.abs(np.linalg.norm(plan["side"][:, 1:], axis=2) - 1.0).max() <= 1e-12
        assert np.abs(np.linalg.norm(plan["joint"][:, 1], axis=1) - 1.0).max() <= 1e-12
        assert np.linalg.norm(plan["side"][1 - home, 0]) < plan["add"]["reach"]
        assert abs(plan["joint"][0, 0, 0] - (sj - sf)) < 1e-2 and np.linalg.norm(plan["joint"][0, 0, 1:]) < 2e-2
        assert plan["side_axis"][1][0] == np.float32(1.0 / 80.0) and plan["side_axis"][1][1] == 0.0


def test_locate_plan_runs_cleanly_under_sanitizers(tmp_path):
    """host/gm_wall_alignment_locate_host_test.cpp with gm_wall_host.hip and gm_wall_alignment_host.hip alone, under
    AddressSanitizer and UBSan: a stand-alone program, no device, no Python."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "gm_wall_alignment_locate_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    csrc = os.path.join(ROOT, "geometric_mapping_amd", "csrc")
    subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(csrc, "gm_wall_host.hip"), os.path.join(csrc, "gm_wall_alignment_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_alignment_locate_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_alignment_locate_host_test ok"), r.stdout + r.stderr
