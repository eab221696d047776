"""GPU tests of gm_wall_map_sections (csrc/k_wall_sections.hip + gm_wall.hip) against the twin tests/wall_sections_np.py.
Maps are filled with add_raw; every comparison with the twin is byte equality of the records and the sums and dict
equality of the info, on the basis table the library reports (gm_wall_section_basis)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib
from geometric_mapping_amd.api import RAW_CELL, WALL_SECTION, WALL_SECTION_SUMS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_clearance_np as gn  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_sections_np as sn  # noqa: E402
from test_wall_sections_abi import PHYS_COEF, PHYS_WALL, physics_cloud  # noqa: E402

pytestmark = pytest.mark.gpu
FILLS = (0.0, 0.05, 0.5, 1.0)


@contextlib.contextmanager
def chunk(sections):
    """Maps created inside walk their sections in chunks of `sections` (None: the default)."""
    old = os.environ.pop("GM_WALL_SECTION_CHUNK", None)
    if sections:
        os.environ["GM_WALL_SECTION_CHUNK"] = str(sections)
    try:
        yield
    finally:
        os.environ.pop("GM_WALL_SECTION_CHUNK", None)
        if old is not None:
            os.environ["GM_WALL_SECTION_CHUNK"] = old


def make(c, raw, sections=None, **kw):
    """(map, its gm_wall_params dict) holding the raw cells."""
    p = wn.params(n_stations=raw.shape[0], n_sectors=raw.shape[1], **kw)
    with chunk(sections):
        m = c.wall_map(**p)
    m.add_raw(raw)
    return m, p


def check(m, raw, station0=0, n=None, baseline=None, base_raw=None, **params):
    """One call against the twin, byte for byte; returns (info, records, sums)."""
    info, rec, sums = m.sections(station0, n, baseline=baseline, sums=True, **params)
    B = m.section_basis(params.get("harmonics", 2))
    winfo, wrec, wsums = sn.sections(raw, station0, n, base=base_raw, B=B, **params)
    assert rec.dtype == WALL_SECTION and sums.dtype == WALL_SECTION_SUMS
    assert info == winfo
    for f in WALL_SECTION.names:
        assert np.array_equal(rec[f], wrec[f]), f
    assert rec.tobytes() == wrec.tobytes() and sums.tobytes() == wsums.tobytes()
    assert info["empty"] + info["unusable"] + info["usable"] == info["sections"] * info["n_sectors"]
    assert info["sections_ok"] + info["sections_failed"] == info["sections"] == len(rec)
    return info, rec, sums


def ring(ns, n, usable, value=1000, count=16):
    """Raw cells whose sectors `usable` (bool [ns]) hold `count` points of value `value` units in every station."""
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = np.where(usable, count, 0)
    raw["sum"] = np.where(usable, count * value, 0)
    return raw


# ---- 1. shapes ----

@pytest.mark.parametrize("ns", (1, 2, 8, 9, 63, 64, 65, 90, 129, 4096))
@pytest.mark.parametrize("n", (1, 3, 4, 5, 64))
def test_shapes(gm, n, ns):
    rng = np.random.default_rng(1000 * n + ns)
    turn = 0
    statuses = set()
    with gm.GeometricMapping() as c:
        for fill in FILLS:
            raw = gn.random_raw(rng, n, ns, fill)
            m, p = make(c, raw, t_min=-3.0, radius=2.5)
            for S in sorted({1, 4, 7, n, n + 3}):
                H, passes = turn % 5, 1 + turn % 4
                turn += 1
                info, rec, sums = check(m, raw, section_stations=S, harmonics=H, passes=passes, min_columns=(1, 24)[turn % 2],
                                        reject=(0.05, 0.2)[turn % 3 == 0], max_gap_deg=(90.0, 0.0, 360.0)[turn % 3])
                statuses |= set(rec["status"].tolist())
                assert info["sections"] == (n + S - 1) // S and np.all(rec["stations"][:-1] == S)
                if fill == 0.0:
                    assert info["empty"] == info["sections"] * ns and np.all(rec["status"] & sn.TOO_FEW)
                    assert np.all(rec["largest_gap"] == ns) and np.all(rec["peak_out_sector"] == sn.U32_MAX)
                if ns < 1 + 2 * H:
                    assert np.all(rec["status"] & sn.FAILED_MASK == sn.TOO_FEW)   # n_sectors < P
                if fill == 1.0:
                    assert info["empty"] == 0
            m.close()
    failed = {s & sn.FAILED_MASK for s in statuses}
    assert sn.TOO_FEW in failed and (0 in failed or ns < 63 or n < 4)


@pytest.mark.parametrize("H", range(5))
@pytest.mark.parametrize("passes", (1, 2, 3, 4))
def test_every_harmonic_and_pass_count_on_a_noisy_series(gm, H, passes):
    rng = np.random.default_rng(10 * H + passes)
    ns, n = 90, 12
    noise = np.rint(rng.normal(0.0, 0.02, (n, ns)) * 2 ** 20).astype(np.int64)   # 2 cm: the passes reject differently
    raw = sn.fill_series(ns, n, rng.uniform(-0.05, 0.05, 1 + 2 * H), noise=noise)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec, sums = check(m, raw, harmonics=H, passes=passes, reject=0.01)
        assert info["sections_ok"] == 3 and info["rejected"] > 0 and info["passes"] == passes and info["harmonics"] == H
        assert np.all(rec["fitted"] == sums["fitted"]) and np.all(rec["coef_q"][:, 1 + 2 * H:] == 0)
        if passes == 1:
            assert np.all(rec["fitted"] == rec["usable"])


# ---- 2. a window inside the map, n = 0, the count query, the capacity, the refusals ----

def test_window_capacity_and_refusals(gm):
    rng = np.random.default_rng(3)
    raw = gn.random_raw(rng, 40, 33, 0.9)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw, 2)
        info, rec, _ = check(m, raw, 5, 22, section_stations=4, min_columns=5)
        assert len(rec) == 6 and rec["station_from"].tolist() == [5, 9, 13, 17, 21, 25] and rec["stations"][-1] == 2
        check(m, raw, 39, 1, min_columns=5)
        info, rec, sums = check(m, raw, 17, 0)          # n = 0 gives nothing
        assert len(rec) == 0 and info["sections"] == 0
        check(m, raw, 40, 0)
        for s0, n in ((39, 2), (41, 0), (0, 41)):
            with pytest.raises(gm.GmError) as e:
                m.sections(s0, n)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(TypeError):
            m.sections(threshold=0.1)
        L, h = c._L, m._h()
        SP, UP = C.POINTER(_lib.WallSection), C.POINTER(_lib.WallSectionSums)
        winfo, wrec, wsums = sn.sections(raw, 0, 40, B=m.section_basis(2), min_columns=5)
        prm = m.section_params(min_columns=5)

        def call(buf, cap, got, sums=None, q=prm, n=40, base=None, info=True):
            i = _lib.WallSectionsInfo()
            st = L.gm_wall_map_sections(h, base, 0, n, C.byref(q) if q is not None else None, C.byref(i) if info else None,
                                        buf.ctypes.data_as(SP) if buf is not None else None, cap,
                                        C.byref(got) if got is not None else None,
                                        sums.ctypes.data_as(UP) if sums is not None else None)
            return st, i

        got = C.c_uint32(99)
        st, i = call(None, 0, got)                      # the count query: the info is complete
        assert st == _lib.GM_OK and got.value == 10 and {k: int(getattr(i, k)) for k in sn.INFO_KEYS} == winfo
        assert i.struct_size == C.sizeof(_lib.WallSectionsInfo)
        buf, sbuf = np.zeros(12, WALL_SECTION), np.zeros(12, WALL_SECTION_SUMS)
        for cap in (9, 0):
            got.value = 99
            st, i = call(buf, cap, got, sbuf)
            assert st == _lib.GM_ERR_CAPACITY and got.value == 10 and i.sections == 10
            assert not buf.tobytes().strip(b"\0") and not sbuf.tobytes().strip(b"\0")   # neither array is written
        st, i = call(buf, 12, got, sbuf)
        assert st == _lib.GM_OK and got.value == 10 and buf[:10].tobytes() == wrec.tobytes() and sbuf[:10].tobytes() == wsums.tobytes()
        assert not buf[10:].tobytes().strip(b"\0")
        st, i = call(buf, 10, None, None, q=None)       # NULL: the defaults
        assert st == _lib.GM_OK and buf[:10].tobytes() == sn.sections(raw, B=m.section_basis(2))[1].tobytes()
        bad = _lib.GM_ERR_INVALID_ARG
        assert call(None, 0, got, info=False)[0] == bad
        assert call(None, 5, got)[0] == bad and call(None, 0, got, sbuf)[0] == bad     # NULL sections with a capacity, with sums
        assert call(None, 0, got, n=41)[0] == bad
        for k, v in (("struct_size", 8), ("section_stations", 0), ("harmonics", 5), ("passes", 0), ("passes", 5), ("min_count", 0),
                     ("min_columns", 0), ("max_gap_deg", 361.0), ("reject", 0.0), ("reject", 8.01), ("reject", float("nan"))):
            q = m.section_params()
            setattr(q, k, v)
            assert call(None, 0, got, q=q)[0] == bad, (k, v)
        # the baseline's refusals, as gm_wall_map_regions'
        assert call(None, 0, got, base=h)[0] == bad
        other, _ = make(c, raw[:, :32].copy())
        assert call(None, 0, got, base=other._h())[0] == bad
        shifted, _ = make(c, raw, t_min=0.5)
        assert call(None, 0, got, base=shifted._h())[0] == bad
        looser, _ = make(c, raw, gate=0.5)              # the gate may differ
        assert call(None, 0, got, base=looser._h())[0] == _lib.GM_OK


# ---- 3. the gap ----

@pytest.mark.parametrize("ns", (1, 2, 8, 63, 64, 65, 90, 129, 200, 4096))
def test_largest_gap(gm, ns):
    cases = {"full": np.ones(ns, bool), "empty": np.zeros(ns, bool)}
    one = np.zeros(ns, bool)
    one[ns // 3] = True
    cases["one column"] = one
    if ns >= 8:
        seam = np.ones(ns, bool)
        seam[ns - 3:] = False
        seam[:2] = False
        cases["across the seam"] = seam
        alt = np.arange(ns) % 2 == 0
        cases["alternating"] = alt
    for end in (63, 64, 65):    # a run of five unusable sectors that ends on sector `end`
        if ns > end + 2:
            run = np.ones(ns, bool)
            run[end - 4:end + 1] = False
            cases[f"run ending on {end}"] = run
    want = {"full": 0, "empty": ns, "one column": ns - 1, "across the seam": 5, "alternating": 1 if ns > 1 else 0}
    with gm.GeometricMapping() as c:
        for name, usable in cases.items():
            raw = ring(ns, 3, usable)
            m, p = make(c, raw)
            info, rec, sums = check(m, raw, section_stations=2, harmonics=0, passes=2, min_columns=1, max_gap_deg=10.0)
            g = want.get(name, 5)
            assert np.all(rec["largest_gap"] == g) and np.all(sums["largest_gap"] == g), (name, rec["largest_gap"], g)
            limit = int(np.floor(10.0 * ns / 360.0))
            assert info["max_gap_sectors"] == limit
            assert np.all((rec["status"] & sn.OPEN_ARC != 0) == (g > limit)), name
            if name != "empty":
                assert np.all(rec["status"] & sn.FAILED_MASK == 0) and np.all(rec["coef_q"][:, 0] == 1000)
            m.close()


def test_the_gap_is_of_the_fitted_columns_of_the_last_pass(gm):
    """A niche is usable but not fitted in pass 2: the gap counts it."""
    ns = 90
    raw = sn.fill_series(ns, 4, [0.01, 0.02, -0.01])
    raw["sum"][:, 40:52] += 16 * sn.fixed(0.3)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec, _ = check(m, raw, harmonics=1, passes=1, max_gap_deg=40.0)
        assert rec["largest_gap"][0] == 0 and rec["status"][0] == 0
        info, rec, _ = check(m, raw, harmonics=1, passes=3, max_gap_deg=40.0)
        assert rec["largest_gap"][0] == 12 and rec["status"][0] == sn.OPEN_ARC and rec["rejected"][0] == 12
        assert rec["peak_out_sector"][0] in range(40, 52) and info["sections_open_arc"] == 1 and info["sections_ok"] == 1


# ---- 4. the planted niche, the physics cloud, a baseline ----

@pytest.mark.parametrize("ns,H", ((63, 1), (64, 2), (65, 4), (90, 2), (128, 0), (360, 4)))
def test_planted_niche(gm, ns, H):
    rng = np.random.default_rng(ns + H)
    truth = rng.uniform(-0.06, 0.06, 1 + 2 * H)
    noise = np.rint(rng.uniform(-0.002, 0.002, (4, ns)) * 2 ** 20).astype(np.int64)
    w = int(round(0.08 * ns))
    planted = np.zeros(ns, bool)
    planted[(np.arange(w) - w // 2) % ns] = True
    noise[:, planted] += sn.fixed(0.3)
    raw = sn.fill_series(ns, 4, truth, noise=noise)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec, _ = check(m, raw, harmonics=H)
        assert rec["status"][0] & sn.FAILED_MASK == 0 and rec["rejected"][0] == w and rec["accepted"][0] == ns - w
        assert np.abs(rec["coef_q"][0][:1 + 2 * H] * 2.0 ** -20 - truth).max() <= 0.003
        assert planted[rec["peak_out_sector"][0]]
        met = m.section_metrics(rec[0], H)
        assert abs(met["radial_m"] - truth[0]) <= 0.003 and met["coverage"] == (ns - w) / ns


def test_physics_cloud_through_add_points(gm):
    wall = wn.params(**PHYS_WALL)
    xyz = physics_cloud(wall, PHYS_COEF)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**wall)
        m.add_points(xyz, np.eye(4)[:3], outputs=False)
        raw = m.read_raw()
        assert np.all(raw["count"] == 12)
        info, rec, _ = check(m, raw)
        assert info["sections_ok"] == 2 and info["accepted"] == 180
        # (the exact expectation and its derived bound are tests/test_wall_sections_abi.py's; here: the same tube)
        assert np.abs(rec["coef_q"][:, :5] * 2.0 ** -20 - np.array(PHYS_COEF)).max() < 2e-4
        met = m.section_metrics(rec[1])
        assert met["chainage_from"] == 1.0 and met["chainage_to"] == 2.0 and abs(met["radius_m"] - 1.988) < 2e-4
        assert np.allclose(met["centre"], [1.5, -PHYS_COEF[2], PHYS_COEF[1]], atol=2e-4)   # u = z, v = a x u = -y


def test_baseline_with_a_known_harmonic_difference(gm):
    ns, n = 90, 8
    rng = np.random.default_rng(8)
    then = np.array([0.010, 0.004, -0.003, 0.002, 0.001])
    diff = np.array([-0.008, 0.0, 0.0, 0.003, -0.002])     # 8 mm of convergence and some ovalisation since
    B = sn.basis(ns, 2)
    raw0 = sn.fill_series(ns, n, then)
    raw1 = raw0.copy()
    raw1["sum"] += 16 * sn.model(B, list(np.rint(diff * 2 ** 20).astype(np.int64)))
    raw1["count"][:, 10] = 1          # unusable in the map only (4 points per column)
    raw0["count"][:, 20] = 0          # empty in the baseline only: unusable, not empty
    raw0["sum"][:, 20] = 0
    for r in (raw0, raw1):
        r["count"][:, 30] = 0         # empty in both
        r["sum"][:, 30] = 0
    with gm.GeometricMapping() as c:
        m1, p = make(c, raw1)
        m0, _ = make(c, raw0)
        info, rec, _ = check(m1, raw1, baseline=m0, base_raw=raw0)
        assert info["empty"] == 2 and info["unusable"] == 4 and info["sections_ok"] == 2
        assert np.abs(rec["coef_q"][:, :5] - np.rint(diff * 2 ** 20)).max() <= 2
        assert np.all(rec["points"] == 87 * 16 * 4)           # of the map, not of the baseline
        alone = check(m1, raw1)[1]
        assert np.abs(alone["coef_q"][:, 0] - np.rint((then + diff)[0] * 2 ** 20)).max() <= 2
        check(m0, raw0, baseline=m1, base_raw=raw1, harmonics=4, passes=2)
        with pytest.raises(gm.GmError) as e:
            m1.sections(baseline=m1)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG


# ---- 5. chunks, reused scratch, no side effects ----

def test_chunks_and_reused_scratch_do_not_change_the_bytes(gm):
    rng = np.random.default_rng(11)
    raw = gn.random_raw(rng, 41, 129, 0.8)
    kw = dict(section_stations=3, harmonics=3, passes=4, min_columns=12, reject=0.1)
    with gm.GeometricMapping() as c:
        whole, p = make(c, raw)
        _, wrec, wsums = check(whole, raw, **kw)
        assert len(wrec) == 14 and np.any(wrec["status"] & sn.FAILED_MASK == 0)
        small_want = check(whole, raw, 7, 9, **kw)
        for sections in (1, 3, 5, 10 ** 9):
            m, _ = make(c, raw, sections)
            info, rec, sums = check(m, raw, **kw)                       # large
            assert rec.tobytes() == wrec.tobytes() and sums.tobytes() == wsums.tobytes()
            small = check(m, raw, 7, 9, **kw)                           # small, on the scratch of the large one
            assert small[1].tobytes() == small_want[1].tobytes() and small[2].tobytes() == small_want[2].tobytes()
            info, rec, sums = check(m, raw, **kw)                       # large again
            assert rec.tobytes() == wrec.tobytes() and sums.tobytes() == wsums.tobytes()
            check(m, raw, harmonics=0, passes=1)                        # a narrower basis on the same scratch
            m.close()


def test_no_side_effects_and_scratch(gm):
    rng = np.random.default_rng(9)
    raw = gn.random_raw(rng, 65, 90, 0.7)
    G = gn.random_gauges(rng, 1, 90, 2.0)
    L = _lib.load()
    with gm.GeometricMapping() as c:
        start = L.gm_debug_live_buffers()
        m, p = make(c, raw)
        before = m.read_raw().tobytes()
        regions, cloud, clearance = m.regions(), m.cloud(), m.clearance(0, None, G)
        other = L.gm_debug_live_buffers()                    # a map that never asks allocates nothing for it
        check(m, raw)
        asked = L.gm_debug_live_buffers()
        assert asked == other + 2                            # the basis table and the chunk block
        check(m, raw, 3, 40, harmonics=1)
        check(m, raw)
        assert L.gm_debug_live_buffers() == asked            # grow-only: nothing new for a call that fits
        assert m.read_raw().tobytes() == before == raw.tobytes()
        r2, c2, g2 = m.regions(), m.cloud(), m.clearance(0, None, G)
        assert r2[0] == regions[0] and r2[1].tobytes() == regions[1].tobytes()
        assert c2[0] == cloud[0] and c2[1].tobytes() == cloud[1].tobytes()
        assert g2[0] == clearance[0] and g2[1].tobytes() == clearance[1].tobytes() and g2[2].tobytes() == clearance[2].tobytes()
        m.close()
        assert L.gm_debug_live_buffers() == start
