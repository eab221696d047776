"""gm_wall_map_align_* without a GPU: the symbols, the struct layouts from plain C99, the defaults, every parameter refusal,
the host-only selection (gm_wall_align_select) on hand-made tables against the twin (tests/wall_align_np.py), and the
composed pose."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_align_np as an  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_align_default_params", "gm_wall_align_check_params", "gm_wall_align_select", "gm_wall_map_align_frame",
         "gm_wall_map_get_align", "gm_wall_map_align_points")
F64 = ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction")
INT = ("status", "anchor_station", "overlap", "best_station", "best_sector")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_align_params": _lib.WallAlignParams,
        "gm_wall_align_score": _lib.WallAlignScore,
        "gm_wall_align_info": _lib.WallAlignInfo,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    enums = ("GM_WALL_ALIGN_MAX_PATCH_CELLS", "GM_WALL_ALIGN_MAX_SHIFT", "GM_WALL_ALIGN_MAX_SHIFTS", "GM_ALIGN_OK",
             "GM_ALIGN_NO_OVERLAP", "GM_ALIGN_FAILED_MASK", "GM_ALIGN_AMBIGUOUS", "GM_ALIGN_AT_BORDER")
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
    assert C.sizeof(_lib.WallAlignParams) == 56 and C.sizeof(_lib.WallAlignScore) == 24 and C.sizeof(_lib.WallAlignInfo) == 224
    assert api.WALL_ALIGN_SCORE.itemsize == 24 and an.SCORE == api.WALL_ALIGN_SCORE
    # the twin speaks the same constants
    assert (an.MAX_PATCH_CELLS, an.MAX_SHIFT, an.MAX_SHIFTS, an.OK, an.NO_OVERLAP, an.FAILED_MASK, an.AMBIGUOUS,
            an.AT_BORDER) == tuple(getattr(_lib, e) for e in enums)
    assert _lib.GM_ALIGN_AMBIGUOUS == 1 << 8 and _lib.GM_ALIGN_AT_BORDER == 1 << 9


def test_defaults():
    L = _lib.load()
    p = _lib.WallAlignParams()
    L.gm_wall_align_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallAlignParams) and p.reserved == 0
    assert {k: getattr(p, k) for k in an.DEFAULTS} == an.DEFAULTS
    assert an.DEFAULTS == dict(half_patch_stations=20, max_station_shift=8, max_sector_shift=4, min_count=8, min_frame_count=4,
                               min_overlap=64, gate=0.25, clip=0.05, min_distinction=1.5)
    L.gm_wall_align_default_params(None)   # a NULL is ignored
    q = api.WallMap.align_params(max_sector_shift=2, clip=0.1)
    assert (q.max_sector_shift, q.clip, q.half_patch_stations) == (2, 0.1, 20)
    with pytest.raises(TypeError):
        api.WallMap.align_params(threshold=1.0)


def _check(n_sectors=90, **kw):
    p = api.WallMap.align_params()
    for k, v in kw.items():
        setattr(p, k, v)
    st = _lib.load().gm_wall_align_check_params(C.byref(p), n_sectors)
    if "struct_size" not in kw:
        assert (st == _lib.GM_OK) == an.params_ok({k: getattr(p, k) for k in an.DEFAULTS}, n_sectors), (n_sectors, kw)
    return st


def test_every_parameter_refusal():
    L = _lib.load()
    ok, bad = _lib.GM_OK, _lib.GM_ERR_INVALID_ARG
    nan, inf = float("nan"), float("inf")
    assert _check() == ok
    assert L.gm_wall_align_check_params(None, 90) == bad
    refused = (dict(struct_size=0), dict(struct_size=48), dict(struct_size=64), dict(half_patch_stations=0),
               dict(half_patch_stations=46),                          # 2 * 46 * 90 = 8280
               dict(max_station_shift=65), dict(max_sector_shift=65), dict(max_sector_shift=45),   # 2 * 45 + 1 = 91 > 90
               dict(max_station_shift=64, max_sector_shift=16),       # 129 * 33 = 4257
               dict(min_count=0), dict(min_frame_count=0), dict(min_overlap=0),
               dict(gate=0.0), dict(gate=-0.25), dict(gate=8.000001), dict(gate=nan), dict(gate=inf),
               dict(clip=0.0), dict(clip=-0.05), dict(clip=8.000001), dict(clip=nan), dict(clip=inf), dict(clip=4e-7),   # C = 0
               dict(min_distinction=0.999), dict(min_distinction=nan), dict(min_distinction=inf), dict(min_distinction=-2.0))
    for kw in refused:
        assert _check(**kw) == bad, kw
    accepted = (dict(half_patch_stations=1), dict(half_patch_stations=45),   # 2 * 45 * 90 = 8100
                dict(max_station_shift=0), dict(max_sector_shift=0), dict(max_station_shift=0, max_sector_shift=0),
                dict(max_station_shift=64), dict(max_sector_shift=44),       # 2 * 44 + 1 = 89
                dict(max_station_shift=64, max_sector_shift=15),             # 129 * 31 = 3999
                dict(min_count=1), dict(min_count=0xFFFFFFFF), dict(min_frame_count=1), dict(min_overlap=1),
                dict(min_overlap=0xFFFFFFFF), dict(gate=8.0), dict(gate=1e-6), dict(clip=8.0), dict(clip=5e-7),   # C = 1
                dict(min_distinction=1.0), dict(min_distinction=1e9))
    for kw in accepted:
        assert _check(**kw) == ok, kw
    # 2P n_sectors = 8192 accepted, 8193 and beyond refused; 2B + 1 = n_sectors accepted
    assert _check(64, half_patch_stations=64) == ok and _check(64, half_patch_stations=65) == bad
    assert _check(4096, half_patch_stations=1) == ok and _check(4097, half_patch_stations=1) == bad
    assert _check(8193, half_patch_stations=1, max_sector_shift=0) == bad
    assert _check(1, half_patch_stations=4096, max_sector_shift=0) == ok
    assert _check(1, half_patch_stations=4097, max_sector_shift=0) == bad
    assert _check(1) == bad and _check(0, max_sector_shift=0) == bad          # the default B = 4 needs 9 sectors
    assert _check(33, max_sector_shift=16) == ok and _check(32, max_sector_shift=16) == bad
    assert _check(9) == ok and _check(8) == bad
    pose = np.ascontiguousarray(np.eye(4)[:3]).ctypes.data_as(C.POINTER(C.c_double))
    info, p = _lib.WallAlignInfo(), api.WallMap.align_params()
    assert L.gm_wall_map_align_frame(None, None, 0, pose, C.byref(p), None) == bad
    assert L.gm_wall_map_get_align(None, 0, C.byref(info), None, 0, None) == bad
    assert L.gm_wall_map_align_points(None, None, 0, None, pose, C.byref(p), None, C.byref(info), None, 0, None, None, None) == bad


# ---- gm_wall_align_select against the twin ----

P32 = wn.params(n_stations=96, n_sectors=32)
POSE = synth.pose_matrix((10.3, 0.1, -0.05), yaw_deg=2.0, roll_deg=1.0)


def _table(ap, fill=(4 << 40, 0, 100)):
    t = np.zeros((2 * ap["max_station_shift"] + 1, 2 * ap["max_sector_shift"] + 1), an.SCORE)
    t["ssd"], t["sum_d"], t["n"] = fill
    return t


def _both(t, p=P32, pose=POSE, **kw):
    ap = an.prm(**kw)
    got = api.align_select(api.WallMap.params(**p), pose, t, **kw)
    want = an.select(t, p, pose, ap)
    for k in INT:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in F64:
        assert np.isclose(got[k], want[k], rtol=1e-14, atol=0.0, equal_nan=True), (k, got[k], want[k])
    assert np.allclose(got["pose"], want["pose"], rtol=0.0, atol=1e-12, equal_nan=True)
    assert (got["half_patch_stations"], got["max_station_shift"], got["max_sector_shift"]) == (
        ap["half_patch_stations"], ap["max_station_shift"], ap["max_sector_shift"])
    assert got["n_points"] == got["plane"] == got["binned"] == got["patch_cells_usable"] == 0
    return got


def test_select_plain_minimum_and_fraction():
    ap = an.prm()
    t = _table(ap)
    A, B = 8, 4
    for da, db, c in ((0, 0, 1 << 40), (-1, 0, 2 << 40), (1, 0, 3 << 40), (0, -1, 3 << 40), (0, 1, 2 << 40)):
        t["ssd"][A + 3 + da, B - 2 + db] = c
    t["sum_d"][A + 3, B - 2] = -(37 << 20)
    g = _both(t)
    assert (g["status"], g["best_station"], g["best_sector"], g["overlap"]) == (_lib.GM_ALIGN_OK, 3, -2, 100)
    assert g["frac_station"] == pytest.approx(0.5 * (2 - 3) / (2 - 2 + 3)) and g["frac_sector"] == pytest.approx(0.5 * (3 - 2) / 3)
    assert g["shift_m"] == pytest.approx((3 - 1 / 6) * 0.25) and g["roll"] == pytest.approx((-2 + 1 / 6) * 2 * np.pi / 32)
    assert g["bias_m"] == pytest.approx(-0.37) and g["distinction"] == pytest.approx(4.0)
    assert g["rms_best"] == pytest.approx(np.sqrt((1 << 40) / 100) * 2.0 ** -20)
    assert g["rms_runner"] == pytest.approx(np.sqrt((4 << 40) / 100) * 2.0 ** -20)
    assert wn.pose_ok(g["pose"])


def test_select_ties():
    ap = an.prm()
    A, B = 8, 4
    # every shift the same cost: the smaller max(|a|, |b|) wins, so (0, 0); the wall tells nothing apart
    g = _both(_table(ap))
    assert (g["best_station"], g["best_sector"]) == (0, 0) and g["distinction"] == 1.0
    assert g["status"] == _lib.GM_ALIGN_AMBIGUOUS and g["frac_station"] == 0.0 and g["frac_sector"] == 0.0   # den = 0
    assert wn.pose_ok(g["pose"]) and np.allclose(g["pose"], POSE, atol=1e-15)
    # two equal minima at the same distance: the smaller index
    t = _table(ap)
    t["ssd"][A + 2, B + 1] = t["ssd"][A - 2, B + 1] = 1 << 40
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (-2, 1)
    # two equal minima at different distances, the nearer at the larger index
    t = _table(ap)
    t["ssd"][A - 3, B] = t["ssd"][A + 1, B + 1] = 1 << 40
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (1, 1)
    # equal costs from different (ssd, n)
    t = _table(ap)
    t["ssd"][A - 1, B], t["n"][A - 1, B] = 3 << 30, 300
    t["ssd"][A + 1, B], t["n"][A + 1, B] = 2 << 30, 200
    g = _both(t)
    assert (g["best_station"], g["best_sector"], g["overlap"]) == (-1, 0, 300)


def test_select_128_bit_comparison():
    """Costs of 2^46 + 1/8191 and 2^46: equal in fp64 (an ulp there is 2^-6), and their cross products (about 2^72) do
    not fit 64 bits.  The exact comparison picks the smaller whatever the tie rules would say."""
    ap = an.prm()
    A, B = 8, 4
    t = _table(ap, fill=(1 << 59, 0, 4096))                      # cost 2^47 everywhere else
    t["ssd"][A, B], t["n"][A, B] = (8191 << 46) + 1, 8191        # the centre: favoured by every tie rule, and worse
    t["ssd"][A + 5, B + 3], t["n"][A + 5, B + 3] = 1 << 59, 8192
    assert float((8191 << 46) + 1) / 8191.0 == float(1 << 59) / 8192.0
    g = _both(t)
    assert (g["best_station"], g["best_sector"], g["overlap"]) == (5, 3, 8192)
    t["ssd"][A, B] = (8191 << 46) - 1                            # now the centre is better
    g = _both(t)
    assert (g["best_station"], g["best_sector"], g["overlap"]) == (0, 0, 8191)
    t["ssd"][A, B], t["n"][A, B] = 1 << 59, 8192                 # and with the roles swapped
    t["ssd"][A + 5, B + 3], t["n"][A + 5, B + 3] = (8191 << 46) - 1, 8191
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (5, 3)


def test_select_border_missing_neighbour_and_zero_cost():
    ap = an.prm()
    A, B = 8, 4
    # the best shift on the border of both axes: flagged, no fraction (a neighbour is outside the table)
    t = _table(ap)
    t["ssd"][2 * A, 0] = 1 << 40
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (A, -B) and g["status"] == _lib.GM_ALIGN_AT_BORDER
    assert g["frac_station"] == 0.0 and g["frac_sector"] == 0.0 and wn.pose_ok(g["pose"])
    # on the station border only; the sector axis keeps its fraction
    t = _table(ap)
    t["ssd"][0, B] = 1 << 40
    t["ssd"][0, B + 1] = 2 << 40
    g = _both(t)
    assert g["status"] == _lib.GM_ALIGN_AT_BORDER and g["frac_station"] == 0.0 and g["frac_sector"] > 0.0
    # A = B = 0: one shift, never at the border, no runner
    g = _both(_table(an.prm(max_station_shift=0, max_sector_shift=0)), max_station_shift=0, max_sector_shift=0)
    assert g["status"] == _lib.GM_ALIGN_OK and g["distinction"] == np.inf and np.isnan(g["rms_runner"])
    # an invalid neighbour: fraction 0 on that axis only
    t = _table(ap)
    t["ssd"][A + 1, B + 1] = 1 << 40
    t["ssd"][A, B + 1] = 2 << 40
    t["n"][A + 2, B + 1] = 63
    t["ssd"][A + 1, B] = 3 << 40
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (1, 1) and g["frac_station"] == 0.0 and g["frac_sector"] == pytest.approx(-0.1)
    # an invalid shift is never the best nor the runner, however small its cost
    t = _table(ap)
    t["ssd"][A, B] = 1 << 40
    t["ssd"][A + 4, B], t["n"][A + 4, B] = 0, 63
    g = _both(t)
    assert (g["best_station"], g["distinction"]) == (0, 4.0)
    # c_best = 0
    t = _table(ap)
    t["ssd"][A - 1, B + 2] = 0
    g = _both(t)
    assert (g["best_station"], g["best_sector"]) == (-1, 2) and g["distinction"] == np.inf and g["rms_best"] == 0.0
    assert g["status"] == _lib.GM_ALIGN_OK
    # the runner is taken outside the 3 x 3 block around the best: here it is the only valid shift left
    t = _table(ap, fill=(4 << 40, 0, 10))
    t["n"][A, B], t["ssd"][A, B] = 100, 1 << 40
    t["n"][A + 1, B + 1], t["ssd"][A + 1, B + 1] = 100, (1 << 40) + 5
    g = _both(t)
    assert g["distinction"] == np.inf and np.isnan(g["rms_runner"])
    t["n"][A + 2, B] = 100
    g = _both(t)
    assert g["distinction"] == 4.0


def test_select_no_valid_shift():
    ap = an.prm()
    t = _table(ap, fill=(1 << 30, 5, 63))
    g = _both(t)
    assert g["status"] == _lib.GM_ALIGN_NO_OVERLAP and g["status"] & _lib.GM_ALIGN_FAILED_MASK
    assert np.all(np.isnan(g["pose"])) and all(np.isnan(g[k]) for k in F64)
    assert (g["best_station"], g["best_sector"], g["overlap"]) == (0, 0, 0)
    g = _both(t, min_overlap=63)
    assert g["status"] == _lib.GM_ALIGN_AMBIGUOUS


def test_select_refusals():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    ap = an.prm()
    t = np.ascontiguousarray(_table(ap).reshape(-1))
    tp = t.ctypes.data_as(C.POINTER(_lib.WallAlignScore))
    wp, prm, info = api.WallMap.params(**P32), api.WallMap.align_params(), _lib.WallAlignInfo()
    dp = lambda m: np.ascontiguousarray(m).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(POSE), tp, len(t), C.byref(info)) == _lib.GM_OK
    assert L.gm_wall_align_select(C.byref(wp), None, dp(POSE), tp, len(t), C.byref(info)) == _lib.GM_OK     # the defaults
    assert L.gm_wall_align_select(None, C.byref(prm), dp(POSE), tp, len(t), C.byref(info)) == bad
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), None, tp, len(t), C.byref(info)) == bad
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(POSE), None, len(t), C.byref(info)) == bad
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(POSE), tp, len(t), None) == bad
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(POSE), tp, len(t) - 1, C.byref(info)) == bad
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(POSE * 1.01), tp, len(t), C.byref(info)) == bad
    nan = POSE.copy()
    nan[0, 3] = np.nan
    assert L.gm_wall_align_select(C.byref(wp), C.byref(prm), dp(nan), tp, len(t), C.byref(info)) == bad
    few = api.WallMap.params(**dict(P32, n_sectors=8))          # 2B + 1 = 9 > 8
    assert L.gm_wall_align_select(C.byref(few), C.byref(prm), dp(POSE), tp, len(t), C.byref(info)) == bad


# ---- the composed pose ----

@pytest.mark.parametrize("shift", ((3, 2), (-2, -1), (0, 0), (5, 0), (-8, 4), (0, -4)))
def test_whole_cell_shift_moves_every_point_by_whole_cells(shift):
    """Dyadic inputs (axis along x, ds = 0.25, dyadic t_min and translation, as wall_np.chainage_pair's): a point binned
    under the composed pose lands exactly a* stations and b* sectors from where the caller's pose put it."""
    sa, sb = shift
    ns = 32
    p = wn.params(n_stations=400, n_sectors=ns, t_min=-8.0)
    rot = synth.pose_matrix((0, 0, 0), yaw_deg=5.0, roll_deg=3.0)[:, :3]
    pose = np.concatenate([rot, np.array([21.375, 0.1875, -0.125]).reshape(3, 1)], axis=1)
    ap = an.prm(min_overlap=1)
    t = _table(ap, fill=(0, 0, 0))
    t["ssd"][8 + sa, 4 + sb], t["n"][8 + sa, 4 + sb] = 1 << 30, 50          # the one valid shift: no fraction
    g = _both(t, p=p, pose=pose, min_overlap=1)
    assert (g["best_station"], g["best_sector"], g["frac_station"], g["frac_sector"]) == (sa, sb, 0.0, 0.0)
    assert g["shift_m"] == sa * 0.25 and wn.pose_ok(g["pose"])
    # points at cell centres of the design cylinder, in sensor coordinates under the caller's pose
    rng = np.random.default_rng(3)
    j = rng.integers(100, 140, 500)
    k = rng.integers(0, ns, 500)
    tt, phi = p["t_min"] + (j + 0.5) * 0.25, (k + 0.5) * 2 * np.pi / ns
    world = np.stack([tt, -2.0 * np.sin(phi), 2.0 * np.cos(phi)], axis=1)   # u = +z, v = a x u = -y
    sensor = ((world - pose[:, 3]) @ pose[:, :3]).astype(np.float32)
    design = wn.design_frame(p)
    old = wn.points(sensor, None, wn.add_frame(design, p, pose), p)
    new = wn.points(sensor, None, wn.add_frame(design, p, g["pose"]), p)
    assert np.array_equal(old["cell"], j * ns + k)
    assert np.array_equal(new["cell"] // ns, j + sa) and np.array_equal(new["cell"] % ns, (k + sb) % ns)
    assert np.abs(new["e"] - old["e"]).max() < 1e-6
    # the chainage moved by whole stations exactly, the lateral position not at all
    a = design["a"]
    dt = g["pose"][:, 3] - pose[:, 3]
    assert dt @ a == sa * 0.25
    if sb == 0:
        assert np.array_equal(g["pose"][:, :3], pose[:, :3]) and np.array_equal(dt, sa * 0.25 * a)
