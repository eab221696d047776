"""gm_group_fit_cylinder (cylinder regression over a sharded frame) checks that need no GPU: the three entry points are
exported, declared and prototyped, their C signatures compile from C99 as documented, a NULL group is refused, the
ABI version did not move, and the Python group exposes fit_cylinder / labels."""
import ctypes as C
import os
import subprocess
import tempfile

from geometric_mapping_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_group_fit_cylinder", "gm_group_get_cylinder_fit", "gm_group_get_labels")


def test_group_fit_entry_points_are_exported_declared_and_prototyped():
    L = _lib.load()
    names = _lib.declared_symbols()
    for n in NAMES:
        assert n in names and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_group_fit_signatures_compile_from_c99():
    src = r'''
#include <stdint.h>
#include "gm_hip.h"
static gm_status (*fit)(gm_group *, const float[7], gm_cylinder_fit *) = gm_group_fit_cylinder;
static gm_status (*get)(const gm_group *, gm_cylinder_fit *) = gm_group_get_cylinder_fit;
static gm_status (*lab)(gm_group *, uint8_t *, uint32_t, uint32_t *) = gm_group_get_labels;
int main(void) { return (fit && get && lab) ? 0 : 1; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c],
                       check=True)


def test_group_fit_entry_points_refuse_a_null_group():
    L = _lib.load()
    f = _lib.CylinderFit()
    n = C.c_uint32(7)
    init = (C.c_float * 7)(0, 0, 0, 1, 0, 0, 2)
    assert L.gm_group_fit_cylinder(None, init, C.byref(f)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_group_fit_cylinder(None, None, C.byref(f)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_group_get_cylinder_fit(None, C.byref(f)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_group_get_labels(None, None, 0, C.byref(n)) == _lib.GM_ERR_INVALID_ARG


def test_python_group_exposes_fit_and_labels():
    from geometric_mapping_amd.api import GeometricMappingGroup
    for m in ("fit_cylinder", "last_cylinder_fit", "labels"):
        assert callable(getattr(GeometricMappingGroup, m, None)), m
