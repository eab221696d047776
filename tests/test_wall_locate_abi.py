"""gm_wall_map_locate_* without a GPU: the symbols, the struct layouts from plain C99, the defaults, and the refusals that
need no device (a NULL, a struct_size mismatch, a parameter outside its limits)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_locate_np as ln  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_locate_default_params", "gm_wall_locate_check_params", "gm_wall_map_locate_frame", "gm_wall_map_get_locate",
         "gm_wall_map_locate_points")
C_NAME = {"pass_": "pass"}   # (a Python keyword)


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_locate_params": _lib.WallLocateParams,
        "gm_wall_locate_pass": _lib.WallLocatePass,
        "gm_wall_locate_info": _lib.WallLocateInfo,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {C_NAME.get(f, f)}));')
    enums = ("GM_WALL_LOCATE_DESIGN", "GM_WALL_LOCATE_MAP", "GM_LOCATE_OK", "GM_LOCATE_DEGENERATE", "GM_LOCATE_SINGULAR",
             "GM_LOCATE_FAILED_MASK", "GM_LOCATE_NOT_CONVERGED", "GM_LOCATE_PASSES")
    for e in enums:
        lines.append(f'printf("%d\\n", (int){e});')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gm_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = []
    for _, ct in sorted(fields.items()):
        want.append(C.sizeof(ct))
        want += [getattr(ct, f).offset for f, _t in ct._fields_]
    want += [getattr(_lib, e) for e in enums]
    assert out == want
    assert C.sizeof(_lib.WallLocateParams) == 24 and C.sizeof(_lib.WallLocatePass) == 112 and C.sizeof(_lib.WallLocateInfo) == 488
    # the twin speaks the same constants
    assert (ln.DESIGN, ln.MAP, ln.OK, ln.DEGENERATE, ln.SINGULAR, ln.FAILED_MASK, ln.NOT_CONVERGED) == tuple(
        getattr(_lib, e) for e in enums[:7])
    assert ln.STEP_BOUND == _lib.GM_FIT_STEP_BOUND


def test_defaults():
    L = _lib.load()
    p = _lib.WallLocateParams()
    L.gm_wall_locate_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallLocateParams) and p.reserved == 0
    assert (p.reference, p.min_count, p.gate) == (_lib.GM_WALL_LOCATE_DESIGN, 8, 0.25)
    assert (p.reference, p.min_count, p.gate) == tuple(ln.DEFAULTS[k] for k in ("reference", "min_count", "gate"))
    L.gm_wall_locate_default_params(None)   # a NULL is ignored
    q = api.WallMap.locate_params(reference=_lib.GM_WALL_LOCATE_MAP, gate=0.5)
    assert (q.reference, q.min_count, q.gate) == (1, 8, 0.5)
    try:
        api.WallMap.locate_params(threshold=1.0)
        raise AssertionError("an unknown keyword was accepted")
    except TypeError:
        pass


def test_null_struct_size_and_parameter_refusals():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    ok = api.WallMap.locate_params()
    assert L.gm_wall_locate_check_params(C.byref(ok)) == _lib.GM_OK
    assert L.gm_wall_locate_check_params(None) == bad
    for k, v in (("struct_size", 0), ("struct_size", 20), ("struct_size", 32), ("reference", 2), ("reference", 0xFFFFFFFF),
                 ("min_count", 0), ("gate", 0.0), ("gate", -0.25), ("gate", 8.000001), ("gate", float("nan")),
                 ("gate", float("inf"))):
        p = api.WallMap.locate_params()
        setattr(p, k, v)
        assert L.gm_wall_locate_check_params(C.byref(p)) == bad, (k, v)
    for k, v in (("reference", _lib.GM_WALL_LOCATE_MAP), ("min_count", 1), ("min_count", 0xFFFFFFFF), ("gate", 8.0), ("gate", 1e-6)):
        p = api.WallMap.locate_params()
        setattr(p, k, v)
        assert L.gm_wall_locate_check_params(C.byref(p)) == _lib.GM_OK, (k, v)
    pose = np.ascontiguousarray(np.eye(4)[:3]).ctypes.data_as(C.POINTER(C.c_double))
    info = _lib.WallLocateInfo()
    assert L.gm_wall_map_locate_frame(None, None, 0, pose, C.byref(ok)) == bad
    assert L.gm_wall_map_get_locate(None, 0, C.byref(info)) == bad
    assert L.gm_wall_map_locate_points(None, None, 0, None, pose, C.byref(ok), C.byref(info), None, None) == bad
