"""gm_wall_map_add_*_checked without a GPU: the symbols, the struct layouts from plain C99, the defaults, and
gm_wall_add_checked_check_params at and beyond the limits, against the twin's rule (tests/wall_add_checked_np.py)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_add_checked_np as an  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_add_checked_default_params", "gm_wall_add_checked_check_params", "gm_wall_map_add_frame_checked",
         "gm_wall_map_get_add_checked", "gm_wall_map_add_points_checked")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {"gm_wall_add_checked_params": _lib.WallAddCheckedParams, "gm_wall_add_checked_info": _lib.WallAddCheckedInfo}
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    for e in ("GM_WALL_SKIP_NEG", "GM_WALL_SKIP_POS"):
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
    want += [_lib.GM_WALL_SKIP_NEG, _lib.GM_WALL_SKIP_POS]
    assert out == want
    assert C.sizeof(_lib.WallAddCheckedParams) == 16 and C.sizeof(_lib.WallAddCheckedInfo) == 64
    assert (_lib.GM_WALL_SKIP_NEG, _lib.GM_WALL_SKIP_POS) == (an.SKIP_NEG, an.SKIP_POS) == (1, 2)
    assert [f for f, _t in _lib.WallAddCheckedInfo._fields_][1:] == list(api._ADD_CHECKED_INFO)


def test_defaults():
    L = _lib.load()
    p = _lib.WallAddCheckedParams()
    L.gm_wall_add_checked_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallAddCheckedParams)
    assert (p.skip, p.min_delta) == (3, 0.0) == (an.DEFAULTS["skip"], an.DEFAULTS["min_delta"])
    L.gm_wall_add_checked_default_params(None)   # a NULL is ignored
    q = api.WallMap.add_checked_params(skip=1, min_delta=0.25)
    assert (q.skip, q.min_delta, q.struct_size) == (1, 0.25, 16)
    with pytest.raises(TypeError):
        api.WallMap.add_checked_params(struct_size=8)


@pytest.mark.parametrize("skip,min_delta,ok", [
    (1, 0.0, True), (2, 0.0, True), (3, 0.0, True), (3, 8.0, True), (1, 8.0, True), (3, 2.0 ** -20, True),
    (0, 0.0, False), (4, 0.0, False), (7, 0.0, False), (3, -2.0 ** -30, False), (3, 8.000001, False), (3, float("nan"), False),
    (3, float("inf"), False), (3, -0.0, True)])
def test_check_params_at_the_limits(skip, min_delta, ok):
    L = _lib.load()
    p = api.WallMap.add_checked_params(skip=skip, min_delta=min_delta)
    assert (L.gm_wall_add_checked_check_params(C.byref(p)) == _lib.GM_OK) == ok
    assert an.params_ok(skip, min_delta) == ok


def test_check_params_refuses_a_wrong_size_and_null():
    L = _lib.load()
    p = api.WallMap.add_checked_params()
    assert L.gm_wall_add_checked_check_params(C.byref(p)) == _lib.GM_OK
    for size in (0, 8, 15, 17, 24):
        p.struct_size = size
        assert L.gm_wall_add_checked_check_params(C.byref(p)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_add_checked_check_params(None) == _lib.GM_ERR_INVALID_ARG
