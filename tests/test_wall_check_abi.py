"""gm_wall_map_check_* without a GPU: the symbols, the struct layouts from plain C99, the defaults, the host-only
gm_wall_check_classify against the twin (tests/wall_check_np.py) over random and edge cells, envelope-changed implies
mean-changed, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_check_np as kn  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_check_default_params", "gm_wall_check_classify", "gm_wall_map_check_frame", "gm_wall_map_get_check",
         "gm_wall_map_check_points")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_check_params": _lib.WallCheckParams,
        "gm_wall_check_point": _lib.WallCheckPoint,
        "gm_wall_check_info": _lib.WallCheckInfo,
    }
    lines = []
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    enums = ("GM_WALL_CHECK_MEAN", "GM_WALL_CHECK_ENVELOPE", "GM_WALL_CHECK_CLS_PLANE", "GM_WALL_CHECK_CLS_BEYOND_GATE",
             "GM_WALL_CHECK_CLS_OUTSIDE", "GM_WALL_CHECK_CLS_UNSURVEYED", "GM_WALL_CHECK_CLS_UNCHANGED",
             "GM_WALL_CHECK_CLS_CHANGED_POS", "GM_WALL_CHECK_CLS_CHANGED_NEG")
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
    assert [getattr(_lib, e) for e in enums[2:]] == [kn.PLANE, kn.BEYOND, kn.OUTSIDE, kn.UNSURVEYED, kn.UNCHANGED, kn.CHANGED_POS,
                                                    kn.CHANGED_NEG]
    assert C.sizeof(_lib.WallCheckPoint) == 32 == api.WALL_CHECK_POINT.itemsize and kn.POINT == api.WALL_CHECK_POINT
    assert [api.WALL_CHECK_POINT.fields[f][1] for f, _t in _lib.WallCheckPoint._fields_] == [
        getattr(_lib.WallCheckPoint, f).offset for f, _t in _lib.WallCheckPoint._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


def test_defaults():
    L = _lib.load()
    p = _lib.WallCheckParams()
    L.gm_wall_check_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallCheckParams) == 32 and p.reserved == 0
    assert (p.reference, p.min_count, p.threshold, p.gate) == (_lib.GM_WALL_CHECK_MEAN, 8, 0.05, 1.0)
    for k, v in kn.DEFAULTS.items():
        assert getattr(p, k) == v
    L.gm_wall_check_default_params(None)   # a NULL is ignored
    q = api.WallMap.check_params(reference=1, threshold=0.1)
    assert q.reference == 1 and q.threshold == 0.1 and q.min_count == 8
    with pytest.raises(TypeError):
        api.WallMap.check_params(struct_size=8)


def _classify(L, p, raw, e):
    """gm_wall_check_classify over arrays: (delta int64 [n], cls uint32 [n])."""
    raw = np.ascontiguousarray(raw, dtype=wn.RAW_CELL)
    e = np.asarray(e, np.float32)
    d, c = C.c_int64(0), C.c_uint32(0)
    dl, cl = np.empty(len(e), np.int64), np.empty(len(e), np.uint32)
    base = raw.ctypes.data
    for i in range(len(e)):
        cell = C.cast(C.c_void_p(base + i * wn.RAW_CELL.itemsize), C.POINTER(_lib.WallRawCell))
        assert L.gm_wall_check_classify(C.byref(p), cell, C.c_float(e[i]), C.byref(d), C.byref(c)) == _lib.GM_OK
        dl[i], cl[i] = d.value, c.value
    return dl, cl


def _cells(rng, n, min_count):
    """Random raw cells as an add builds them (sum within count * [min, max]), negative sums among them, plus the counts
    around min_count and empty cells."""
    cnt = rng.integers(1, 40, n)
    cnt[rng.random(n) < 0.1] = min_count - 1
    cnt[rng.random(n) < 0.1] = min_count
    cnt[rng.random(n) < 0.05] = 0
    centre = rng.normal(0.0, 0.08, n)
    half = np.abs(rng.normal(0.0, 0.03, n))
    lo = (centre - half).astype(np.float32)
    hi = (centre + half).astype(np.float32)
    mean = rng.uniform(lo.astype(np.float64), hi.astype(np.float64))
    raw = np.zeros(n, wn.RAW_CELL)
    raw["count"] = cnt
    # a sum an add could have produced: between count * fix(lo) and count * fix(hi)
    s = np.rint(mean * 2.0 ** 20).astype(np.int64) * cnt
    s = np.clip(s, kn.fix(lo) * cnt, kn.fix(hi) * cnt)
    s += np.where(cnt > 1, rng.integers(0, 2, n) * np.sign(centre).astype(np.int64), 0)   # not a multiple of count: the division rounds
    s = np.clip(s, kn.fix(lo) * cnt, kn.fix(hi) * cnt)
    raw["sum"] = np.where(cnt > 0, s, 0)
    raw["min_key"] = np.where(cnt > 0, ~wn.ordered(lo), 0)
    raw["max_key"] = np.where(cnt > 0, wn.ordered(hi), 0)
    return raw


@pytest.mark.parametrize("threshold,min_count,gate", ((0.05, 8, 1.0), (0.013, 1, 0.3), (2.0 ** -20, 3, 8.0)))
def test_classify_equals_twin(threshold, min_count, gate):
    L = _lib.load()
    rng = np.random.default_rng(int(threshold * 1e6) + min_count)
    n = 3000
    raw = _cells(rng, n, min_count)
    assert (raw["sum"] < 0).sum() > 200 and (raw["count"] == min_count - 1).sum() > 50 and (raw["count"] == 0).sum() > 20
    T = kn.threshold_q(threshold)
    g32 = np.float32(gate)
    e = rng.normal(0.0, 0.12, n).astype(np.float32)
    # delta exactly +-T and +-(T - 1) against the mean and against the envelope's edges
    q = kn.div_toward_zero(raw["sum"], np.maximum(raw["count"].astype(np.int64), 1))
    hq, lq = kn.fix(wn.unordered(raw["max_key"])), kn.fix(wn.unordered(~raw["min_key"]))
    edge = np.arange(n) % 16
    for k, (ref, off) in enumerate(((q, T), (q, -T), (q, T - 1), (q, -(T - 1)), (hq, T), (hq, T - 1), (lq, -T), (lq, -(T - 1)))):
        sel = edge == k
        e[sel] = ((ref[sel] + off).astype(np.float64) * 2.0 ** -20).astype(np.float32)   # exact: |.| < 2^24 units
        assert np.array_equal(kn.fix(e[sel]), ref[sel] + off)
    # |e| on either side of the gate, and NaN
    e[edge == 8] = g32
    e[edge == 9] = np.nextafter(g32, np.float32(np.inf))
    e[edge == 10] = -np.nextafter(g32, np.float32(np.inf))
    e[(edge == 11) & (np.arange(n) % 32 == 11)] = np.nan
    seen = set()
    both = {}
    for ref in (kn.MEAN, kn.ENVELOPE):
        p = api.WallMap.check_params(reference=ref, threshold=threshold, min_count=min_count, gate=gate)
        d, c = _classify(L, p, raw, e)
        td, tc = kn.classify(e, np.arange(n), raw, reference=ref, threshold=threshold, min_count=min_count, gate=gate)
        assert np.array_equal(c, tc) and np.array_equal(d, td), ref
        seen |= set(c.tolist())
        both[ref] = c
        with np.errstate(invalid="ignore"):
            beyond = ~(np.abs(e) <= g32)
        assert np.all(c[beyond] == kn.BEYOND) and np.all(c[~beyond & (raw["count"] < min_count)] == kn.UNSURVEYED)
        assert np.all(d[(c == kn.BEYOND) | (c == kn.UNSURVEYED)] == 0)
        assert np.all(d[c == kn.CHANGED_POS] >= T) and np.all(d[c == kn.CHANGED_NEG] <= -T) and np.all(np.abs(d[c == kn.UNCHANGED]) < T)
        # the single-pair binding gives the same answer
        for i in (0, 1, 2, 17):
            assert api.wall_check_classify(raw[i], e[i], reference=ref, threshold=threshold, min_count=min_count, gate=gate) == (d[i], c[i])
    assert seen == {kn.BEYOND, kn.UNSURVEYED, kn.UNCHANGED, kn.CHANGED_POS, kn.CHANGED_NEG}
    # envelope-changed implies mean-changed, with the same sign: lo_q <= q <= hi_q by monotone rounding
    usable = raw["count"] >= min_count
    assert np.all(lq[usable] <= q[usable]) and np.all(q[usable] <= hq[usable])
    env = both[kn.ENVELOPE] >= kn.CHANGED_POS
    assert env.sum() > 100 and np.array_equal(both[kn.ENVELOPE][env], both[kn.MEAN][env])


def test_division_goes_toward_zero():
    L = _lib.load()
    raw = np.zeros(2, wn.RAW_CELL)
    raw["count"] = 8
    raw["sum"] = (-15, 15)          # q = -1 and 1, not -2
    raw["min_key"] = ~wn.ordered(np.float32([-1.0, -1.0]))
    raw["max_key"] = wn.ordered(np.float32([1.0, 1.0]))
    p = api.WallMap.check_params(threshold=2.0 ** -20)
    d, c = _classify(L, p, raw, np.float32([0.0, 0.0]))
    assert d.tolist() == [1, -1] and c.tolist() == [kn.CHANGED_POS, kn.CHANGED_NEG]
    assert kn.classify(np.float32([0.0, 0.0]), [0, 1], raw, threshold=2.0 ** -20)[0].tolist() == [1, -1]


def test_refusals_without_a_device():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    raw = _lib.WallRawCell()
    d, c = C.c_int64(0), C.c_uint32(0)
    ok = api.WallMap.check_params()
    assert L.gm_wall_check_classify(C.byref(ok), C.byref(raw), 0.0, C.byref(d), C.byref(c)) == _lib.GM_OK
    assert L.gm_wall_check_classify(None, C.byref(raw), 0.0, C.byref(d), C.byref(c)) == bad
    assert L.gm_wall_check_classify(C.byref(ok), None, 0.0, C.byref(d), C.byref(c)) == bad
    assert L.gm_wall_check_classify(C.byref(ok), C.byref(raw), 0.0, None, C.byref(c)) == bad
    assert L.gm_wall_check_classify(C.byref(ok), C.byref(raw), 0.0, C.byref(d), None) == bad
    for k, v in (("struct_size", 24), ("threshold", 2.0 ** -22), ("threshold", 0.0), ("threshold", 8.5), ("threshold", float("nan")),
                 ("gate", 0.0), ("gate", 8.5), ("gate", float("nan")), ("reference", 2), ("min_count", 0)):
        p = api.WallMap.check_params()
        setattr(p, k, v)
        assert L.gm_wall_check_classify(C.byref(p), C.byref(raw), 0.0, C.byref(d), C.byref(c)) == bad, (k, v)
    # the device calls refuse a NULL map before anything else
    info, got = _lib.WallCheckInfo(), C.c_uint32(7)
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    assert L.gm_wall_map_check_frame(None, None, 0, pose, C.byref(ok), None) == bad
    assert L.gm_wall_map_get_check(None, 0, C.byref(info), None, 0, C.byref(got)) == bad
    assert L.gm_wall_map_check_points(None, None, 0, None, pose, C.byref(ok), None, C.byref(info), None, 0, C.byref(got),
                                      None, None, None, None) == bad
