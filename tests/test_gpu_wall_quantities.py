"""GPU tests of gm_wall_map_quantities (csrc/k_wall_quantities.hip + gm_wall.hip) against the twin
tests/wall_quantities_np.py.  Maps are filled with add_raw, so every integer is chosen; every comparison with the twin is
byte equality of the records and the profile rows and dict equality of the info.  No tolerance anywhere.

Run as a program (`python test_gpu_wall_quantities.py <out file>`) this file is the child of the chunk test: it makes
the maps under the GM_WALL_QUANTITY_CHUNK of its environment -- which is read at gm_wall_map_create -- and writes the
bytes of its calls."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest  # noqa: E402

from geometric_mapping_amd import _lib  # noqa: E402
from geometric_mapping_amd.api import RAW_CELL, WALL_QUANTITY  # noqa: E402

import wall_clearance_np as gn  # noqa: E402
import wall_np as wn  # noqa: E402
import wall_quantities_np as qn  # noqa: E402
from test_wall_quantities_abi import BOUNDARY_COLUMNS  # noqa: E402

pytestmark = pytest.mark.gpu
SAT = qn.SAT


def make(c, raw, **kw):
    """(map, its gm_wall_params dict) holding the raw cells."""
    p = wn.params(n_stations=raw.shape[0], n_sectors=raw.shape[1], **kw)
    m = c.wall_map(**p)
    m.add_raw(raw)
    return m, p


def check(m, p, raw, lo, hi, station0=0, n=None, baseline=None, base_raw=None, **kw):
    """One call against the twin, byte for byte; returns (info, records, rows)."""
    info, rec, rows = m.quantities(lo, hi, station0, n, baseline=baseline, profile_rows=True, **kw)
    winfo, wrec, wrows = qn.quantities(raw, lo, hi, p["radius"], station0, n, base=base_raw, **kw)
    assert rec.dtype == WALL_QUANTITY and rows.dtype == np.int32
    assert info == winfo
    for f in WALL_QUANTITY.names:
        assert np.array_equal(rec[f], wrec[f]), f
    assert rec.tobytes() == wrec.tobytes() and rows.tobytes() == wrows.tobytes()
    assert sum(info[k] for k in qn.CLASS_NAMES) == info["sections"] * info["n_sectors"]
    return info, rec, rows


def zones_of(rng, ns, nz, unmeasured=0.1, mixed=False):
    """A zone table with every zone but the last used where ns allows, some sectors not measured; the zones in runs along
    the ring or, mixed, changing from sector to sector."""
    z = rng.integers(0, max(nz - 1, 1), ns).astype(np.uint8)
    z = z if mixed else np.sort(z)
    z[rng.random(ns) < unmeasured] = qn.NOT_MEASURED
    return z


# ---- 1. lane and row edges ----

@pytest.mark.parametrize("ns", (1, 63, 64, 65, 90, 4096))
def test_lane_and_row_edges(gm, ns):
    rng = np.random.default_rng(ns)
    n = 13 if ns == 4096 else 64
    with gm.GeometricMapping() as c:
        for fill in (0.3, 1.0):
            raw = gn.random_raw(rng, n, ns, fill)
            m, p = make(c, raw, t_min=-3.0, radius=2.5)
            lo, hi = qn.random_tables(rng, 2, ns)
            for S, s0, nn in ((1, 0, n), (3, 0, n), (4, 0, n), (3, 2, 10), (4, n - 7, 7), (4, 5, 1), (n + 5, 0, n), (1, n - 1, 1),
                              (3, 1, n - 1)):
                NS = (nn + S - 1) // S
                prof = rng.integers(0, 2, NS).astype(np.uint8)
                for nz in (1, 8):
                    info, rec, rows = check(m, p, raw, lo, hi, s0, nn, section_stations=S, min_count=6, section_profile=prof,
                                            zone=zones_of(rng, ns, nz, mixed=fill == 1.0), n_zones=nz)
                    assert rec.shape == (NS, nz) and rows.shape == (NS, ns)
                    assert rec["stations"][-1, 0] == nn - (NS - 1) * S and rec["station_from"][0, 0] == s0
            m.close()


# ---- 2. chunks: the environment is read at create, so each map lives in a fresh child process ----

def _chunk_case():
    rng = np.random.default_rng(77)
    n, ns = 41, 129
    raw, base = gn.random_raw(rng, n, ns, 0.8), gn.random_raw(rng, n, ns, 0.9)
    lo, hi = qn.random_tables(rng, 3, ns)
    kw = dict(section_stations=3, min_count=5, section_profile=rng.integers(0, 3, 14).astype(np.uint8), zone=zones_of(rng, ns, 4),
              n_zones=4)
    return raw, base, lo, hi, kw


def _chunk_child(out):
    import geometric_mapping_amd as g
    raw, base, lo, hi, kw = _chunk_case()
    with g.GeometricMapping() as c:
        m, p = make(c, raw)
        b, _ = make(c, base)
        parts = []
        for call in (dict(), dict(baseline=b), dict()):     # (the third on the scratch of the first two)
            info, rec, rows = m.quantities(lo, hi, profile_rows=True, **call, **kw)
            parts += [repr(sorted(info.items())).encode(), rec.tobytes(), rows.tobytes()]
        small = dict(kw, section_profile=kw["section_profile"][:3])
        info, rec, rows = m.quantities(lo, hi, 7, 9, profile_rows=True, **small)
        parts += [repr(sorted(info.items())).encode(), rec.tobytes(), rows.tobytes()]
    with open(out, "wb") as f:
        for part in parts:
            f.write(len(part).to_bytes(8, "little") + part)


@pytest.fixture(scope="module")
def chunk_want():
    """The twin's bytes of the child's four calls, computed once."""
    raw, base, lo, hi, kw = _chunk_case()
    parts = []
    for b in (None, base, None):
        info, rec, rows = qn.quantities(raw, lo, hi, wn.DEFAULTS["radius"], base=b, **kw)
        parts += [repr(sorted(info.items())).encode(), rec.tobytes(), rows.tobytes()]
    info, rec, rows = qn.quantities(raw, lo, hi, wn.DEFAULTS["radius"], 7, 9, **dict(kw, section_profile=kw["section_profile"][:3]))
    parts += [repr(sorted(info.items())).encode(), rec.tobytes(), rows.tobytes()]
    return b"".join(len(part).to_bytes(8, "little") + part for part in parts)


@pytest.mark.parametrize("sections", ("1", "2", "5", None, "1000000000"))
def test_chunks_give_the_same_bytes(gm, tmp_path, chunk_want, sections):
    """14 sections in chunks of 1, 2, 5 (which does not divide 14), the default, and a value above it."""
    env = {k: v for k, v in os.environ.items() if k != "GM_WALL_QUANTITY_CHUNK"}
    if sections:
        env["GM_WALL_QUANTITY_CHUNK"] = sections
    out = str(tmp_path / "bytes")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == chunk_want


# ---- 3. zones and profiles ----

def test_zones_and_profiles(gm):
    rng = np.random.default_rng(5)
    n, ns = 10, 90
    raw = gn.random_raw(rng, n, ns, 0.9)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        lo, hi = qn.random_tables(rng, 256, ns)
        zone = np.repeat(np.array([0, 1, 3, 0xFF, 5, 7], np.uint8), 15)     # zones 2, 4 and 6 have no sector
        raw_full = raw.copy()
        assert (raw["count"][:, 45:60].sum(0) >= 8).any()                     # unmeasured sectors that hold usable cells
        for n_profiles in (1, 2, 256):
            prof = np.zeros(3, np.uint8)
            prof[-1] = n_profiles - 1                                         # switches in the last, short section
            info, rec, rows = check(m, p, raw_full, lo[:n_profiles], hi[:n_profiles], section_profile=prof, zone=zone, n_zones=8)
            assert rec.shape == (3, 8) and rec["stations"][-1, 0] == 2 and np.all(rec["profile"][-1] == n_profiles - 1)
            for z in (2, 4, 6):
                for f in ("under", "within", "over", "unsurveyed", "points", "under_area", "over_area", "excess_area"):
                    assert not rec[f][:, z].any()
                assert np.all(rec["peak_under_sector"][:, z] == qn.U32_MAX) and np.all(rec["peak_over_sector"][:, z] == qn.U32_MAX)
            assert info["unmeasured"] == 3 * 15 and (rows[:, 45:60] != qn.NO_VALUE).any()
        check(m, p, raw, lo[:1], hi[:1], n_zones=1)                           # NULL zone and NULL section_profile
        check(m, p, raw, lo[:2], hi[:2], zone=np.full(ns, 0xFF, np.uint8), n_zones=1)   # nothing is measured
        with pytest.raises(gm.GmError) as e:
            m.quantities(lo[:2], hi[:2], section_profile=np.array([0, 1, 2], np.uint8))
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(gm.GmError) as e:
            m.quantities(lo[:2], hi[:2], zone=np.full(ns, 3, np.uint8), n_zones=3)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG


# ---- 4. classes ----

def test_every_class_boundary_through_the_device(gm):
    ns = len(BOUNDARY_COLUMNS)
    raw = np.zeros((1, ns), RAW_CELL)
    lo, hi = np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    for k, (_name, total, count, lo_k, hi_k, _cls) in enumerate(BOUNDARY_COLUMNS):
        raw["sum"][0, k], raw["count"][0, k], lo[k], hi[k] = total, count, lo_k, hi_k
    with gm.GeometricMapping() as c:
        m, p = make(c, raw, radius=2.0)
        info, rec, rows = check(m, p, raw, lo, hi, section_stations=1)
        got = [qn.column(qn.radius_q(2.0), int(raw["count"][0, k]), int(raw["sum"][0, k]), int(lo[k]), int(hi[k])) for k in range(ns)]
        assert [g["cls"] for g in got] == [b[5] for b in BOUNDARY_COLUMNS]
        assert rows[0].tolist() == [qn.NO_VALUE if g["v"] is None else g["v"] for g in got]
        assert {k: info[k] for k in qn.CLASS_NAMES} == {name: sum(b[5] == i for b in BOUNDARY_COLUMNS) for i, name in enumerate(qn.CLASS_NAMES)}
        info, rec, rows = check(m, p, raw, lo, hi, section_stations=1, min_count=2)     # sum -7, count 2: q = -3, toward zero
        assert rows[0, 0] == -3 and info["unusable"] == 0
    # a radius of 0.25 m with a baseline at -2^24 and lo = -2^24: L clamps at 0
    raw1, raw0 = np.zeros((2, 3), RAW_CELL), np.zeros((2, 3), RAW_CELL)
    raw0["count"], raw0["sum"] = 8, -8 * SAT
    raw1["count"] = 8
    raw1["sum"][:, 0], raw1["sum"][:, 1], raw1["sum"][:, 2] = -8 * SAT, 8 * 1000, -8 * (SAT + 5)
    with gm.GeometricMapping() as c:
        m1, p = make(c, raw1, radius=0.25)
        m0, _ = make(c, raw0, radius=0.25)
        lo, hi = np.full(3, -SAT, np.int32), np.zeros(3, np.int32)
        info, rec, rows = check(m1, p, raw1, lo, hi, baseline=m0, base_raw=raw0, section_stations=2)
        x = (1 << 18) + 1000
        assert rows[0].tolist() == [0, 1000 + SAT, 0] and rec[0, 0]["over"] == 1 and rec[0, 0]["over_area"] == (x * x) >> 20
        assert rec[0, 0]["peak_over"] == 1000 + 2 * SAT and rec[0, 0]["peak_over_sector"] == 1


def test_ties_empty_sections_and_negative_sums(gm):
    ns, n = 130, 12
    raw = np.zeros((n, ns), RAW_CELL)
    raw["count"] = 9
    raw["sum"] = 9 * 700                                    # sections 0: every column over by the same 700 units
    raw["sum"][4:8] = -9 * 12345                            # section 1: every column under by the same, negative sums
    raw["sum"][4:8, 70] = -9 * 12345 - 8                    # (still -12345: toward zero)
    raw["count"][8:12] = 7                                  # section 2: no usable column
    raw["count"][8:12, ::2] = 0
    zero = np.zeros(ns, np.int32)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec, rows = check(m, p, raw, zero, zero, min_count=29)
        assert rec["peak_over_sector"][:, 0].tolist() == [0, qn.U32_MAX, qn.U32_MAX] and rec["peak_over"][0, 0] == 700
        assert rec["peak_under_sector"][:, 0].tolist() == [qn.U32_MAX, 0, qn.U32_MAX] and rec["peak_under"][1, 0] == 12345
        assert rec["unsurveyed"][2, 0] == ns and rec["points"][2, 0] == 0 and np.all(rows[2] == qn.NO_VALUE) and np.all(rows[1] == -12345)
        assert info["empty"] == ns // 2 and info["unusable"] == ns // 2 and info["sections_under"] == 1 and info["sections_over"] == 1
        zone = np.zeros(ns, np.uint8)
        zone[:67] = 1                                       # ties inside a zone that starts past a lane group's first lanes
        info, rec, rows = check(m, p, raw, zero, zero, min_count=29, zone=zone, n_zones=2)
        assert rec["peak_over_sector"][0].tolist() == [67, 0] and rec["peak_under_sector"][1].tolist() == [67, 0]
        empty, _ = make(c, np.zeros((n, ns), RAW_CELL))     # an all-empty window
        info, rec, rows = check(empty, p, np.zeros((n, ns), RAW_CELL), zero, zero)
        assert info["empty"] == 3 * ns and not rec["points"].any() and np.all(rows == qn.NO_VALUE)


# ---- 5. a baseline ----

def test_baseline(gm):
    rng = np.random.default_rng(8)
    ns, n = 90, 9
    raw0 = gn.random_raw(rng, n, ns, 1.0)
    raw0["count"] = np.maximum(raw0["count"], 8)
    raw1 = raw0.copy()
    t = 52429                                               # 0.05 m of lining
    raw1["sum"] -= raw1["count"].astype(np.int64) * rng.integers(t - 20000, t + 20000, (n, ns))
    raw1["count"][:, 10] = 1                                # usable in the baseline only
    raw0["count"][:, 20] = 0                                # empty in the baseline only: unusable, not empty
    raw0["sum"][:, 20] = 0
    for r in (raw0, raw1):
        r["count"][:, 30] = 0                               # empty in both
        r["sum"][:, 30] = 0
    zero, thin = np.zeros(ns, np.int32), np.full(ns, -t, np.int32)
    with gm.GeometricMapping() as c:
        m1, p = make(c, raw1)
        m0, _ = make(c, raw0)
        info, rec, rows = check(m1, p, raw1, zero, zero, baseline=m0, base_raw=raw0, section_stations=3)    # moved in / moved out
        assert info["empty"] == 3 and info["unusable"] == 6 and info["under"] > 0 and info["within"] + info["over"] >= 0
        assert np.all(rows[:, [10, 20, 30]] == qn.NO_VALUE) and rec["under_area"].sum() > 0
        a = check(m1, p, raw1, thin, thin, baseline=m0, base_raw=raw0, section_stations=3)                   # thinner than t
        assert a[0]["over"] > 0 and a[0]["under"] > 0 and a[0]["over"] + a[0]["under"] + a[0]["within"] == 3 * 87
        assert np.array_equal(a[2], rows)                                                                  # v does not depend on the lines
        check(m0, p, raw0, zero, thin + t + 5, baseline=m1, base_raw=raw1)                                 # the other way round
        alone = check(m1, p, raw1, zero, zero, section_stations=3)
        assert alone[0]["unusable"] == 3 and alone[0]["empty"] == 3
        # every refusal of a baseline, as gm_wall_map_regions': the map itself, another grid, another context
        for other in (m1, make(c, raw0[:, :32].copy())[0], make(c, raw0, t_min=0.5)[0]):
            with pytest.raises(gm.GmError) as e:
                m1.quantities(zero, zero, baseline=other)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with gm.GeometricMapping() as c2:
            foreign, _ = make(c2, raw0)
            with pytest.raises(gm.GmError) as e:
                m1.quantities(zero, zero, baseline=foreign)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        looser, _ = make(c, raw0, gate=0.5)                 # the gate may differ
        check(m1, p, raw1, zero, zero, baseline=looser, base_raw=raw0)


# ---- 6. the call's conventions ----

def test_call_conventions(gm):
    rng = np.random.default_rng(3)
    ns, n = 33, 40
    raw = gn.random_raw(rng, n, ns, 0.9)
    lo, hi = qn.random_tables(rng, 2, ns)
    zone = zones_of(rng, ns, 3)
    with gm.GeometricMapping() as c:
        m, p = make(c, raw)
        info, rec, rows = check(m, p, raw, lo, hi, 5, 22, zone=zone, n_zones=3)
        assert rec.shape == (6, 3) and rec["station_from"][:, 0].tolist() == [5, 9, 13, 17, 21, 25] and rec["stations"][-1, 0] == 2
        check(m, p, raw, lo, hi, 39, 1)                                       # ends at the map's last station
        info, rec, rows = check(m, p, raw, lo, hi, 17, 0, zone=zone, n_zones=3)   # n = 0 gives nothing
        assert rec.shape == (0, 3) and rows.shape == (0, ns) and info["sections"] == 0
        check(m, p, raw, lo, hi, 40, 0)
        for s0, nn in ((39, 2), (41, 0), (0, 41)):
            with pytest.raises(gm.GmError) as e:
                m.quantities(lo, hi, s0, nn)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(TypeError):
            m.quantities(lo, hi, threshold=0.1)
        L, h = c._L, m._h()
        QP, I32, U8 = C.POINTER(_lib.WallQuantity), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        prof = np.array([0, 1] * 5, np.uint8)
        winfo, wrec, wrows = qn.quantities(raw, lo, hi, p["radius"], section_profile=prof, zone=zone, n_zones=3)
        prm = m.quantity_params()

        def call(buf, cap, got, rows=None, q=prm, nn=n, base=None, info=True, lo=lo, hi=hi, n_profiles=2, prof=prof, zone=zone, nz=3):
            i = _lib.WallQuantitiesInfo()
            st = L.gm_wall_map_quantities(h, base, 0, nn, lo.ctypes.data_as(I32) if lo is not None else None,
                                          hi.ctypes.data_as(I32) if hi is not None else None, n_profiles,
                                          prof.ctypes.data_as(U8) if prof is not None else None,
                                          zone.ctypes.data_as(U8) if zone is not None else None, nz,
                                          C.byref(q) if q is not None else None, C.byref(i) if info else None,
                                          buf.ctypes.data_as(QP) if buf is not None else None, cap,
                                          C.byref(got) if got is not None else None,
                                          rows.ctypes.data_as(I32) if rows is not None else None)
            return st, i

        got = C.c_uint32(99)
        st, i = call(None, 0, got)                          # the count query: the info is complete
        assert st == _lib.GM_OK and got.value == 30 and {k: int(getattr(i, k)) for k in qn.INFO_KEYS} == winfo
        assert i.struct_size == C.sizeof(_lib.WallQuantitiesInfo)
        buf, rbuf = np.zeros(33, WALL_QUANTITY), np.zeros(10 * ns + 4, np.int32)
        for cap in (29, 0):
            got.value = 99
            st, i = call(buf, cap, got, rbuf)
            assert st == _lib.GM_ERR_CAPACITY and got.value == 30
            assert {k: int(getattr(i, k)) for k in qn.INFO_KEYS} == winfo          # ... and still fills info
            assert not buf.tobytes().strip(b"\0") and not rbuf.tobytes().strip(b"\0")   # neither array is written
        st, i = call(buf, 33, got, rbuf)                    # records with profile rows
        assert st == _lib.GM_OK and got.value == 30 and buf[:30].tobytes() == wrec.tobytes() and rbuf[:10 * ns].tobytes() == wrows.tobytes()
        assert not buf[30:].tobytes().strip(b"\0") and not rbuf[10 * ns:].any()
        buf[:] = 0
        st, i = call(buf, 30, None)                         # ... and without them
        assert st == _lib.GM_OK and buf[:30].tobytes() == wrec.tobytes()
        st, i = call(buf, 10, None, q=None, prof=None, zone=None, nz=1)   # NULL: the defaults, table 0, zone 0
        assert st == _lib.GM_OK and buf[:10].tobytes() == qn.quantities(raw, lo, hi, p["radius"])[1].tobytes()
        bad = _lib.GM_ERR_INVALID_ARG
        assert call(None, 0, got, info=False)[0] == bad
        assert call(None, 5, got)[0] == bad and call(None, 0, got, rbuf)[0] == bad     # NULL records with a capacity, with rows
        assert call(None, 0, got, nn=41)[0] == bad
        assert call(None, 0, got, lo=None)[0] == bad and call(None, 0, got, hi=None)[0] == bad
        assert call(None, 0, got, n_profiles=0)[0] == bad and call(None, 0, got, nz=0)[0] == bad and call(None, 0, got, nz=9)[0] == bad
        assert call(None, 0, got, lo=hi, hi=lo)[0] == bad                               # lo > hi somewhere
        for k, v in (("struct_size", 8), ("section_stations", 0), ("min_count", 0)):
            q = m.quantity_params()
            setattr(q, k, v)
            assert call(None, 0, got, q=q)[0] == bad, (k, v)
        assert call(None, 0, got, base=h)[0] == bad


# ---- 7. unchanged state ----

def test_no_side_effects_and_scratch(gm):
    rng = np.random.default_rng(9)
    raw, base = gn.random_raw(rng, 64, 90, 0.7), gn.random_raw(rng, 64, 90, 0.7)
    lo, hi = qn.random_tables(rng, 1, 90)
    G = gn.random_gauges(rng, 1, 90, 2.0)
    L = _lib.load()
    with gm.GeometricMapping() as c:
        start = L.gm_debug_live_buffers()
        m, p = make(c, raw)
        b, _ = make(c, base)
        before, bbefore = m.read_raw().tobytes(), b.read_raw().tobytes()
        sections, clearance = m.sections(), m.clearance(0, None, G)
        other = L.gm_debug_live_buffers()                    # a map that never asks allocates nothing for it
        check(m, p, raw, lo, hi)
        asked = L.gm_debug_live_buffers()
        assert asked == other + 4                            # the lines, the two index tables, the staging, the counters
        check(m, p, raw, lo, hi, 3, 40, baseline=b, base_raw=base, section_stations=7)
        check(m, p, raw, lo, hi)
        assert L.gm_debug_live_buffers() == asked            # grow-only: nothing new for a call that fits
        assert m.read_raw().tobytes() == before == raw.tobytes() and b.read_raw().tobytes() == bbefore == base.tobytes()
        s2, g2 = m.sections(), m.clearance(0, None, G)
        assert s2[0] == sections[0] and s2[1].tobytes() == sections[1].tobytes()
        assert g2[0] == clearance[0] and g2[1].tobytes() == clearance[1].tobytes() and g2[2].tobytes() == clearance[2].tobytes()
        m.close()
        b.close()
        assert L.gm_debug_live_buffers() == start


# ---- 8. end to end: real adds ----

def test_quantities_of_frames_added_with_poses(gm):
    from geometric_mapping_amd import synth
    p = wn.params(n_stations=48, n_sectors=90, station_length=0.25, gate=0.25, t_min=-6.0)
    lo, hi = np.full(90, -1049, np.int32), np.full(90, 1049, np.int32)      # +-1 mm about the design: 1 cm of noise crosses both
    zone = np.repeat(np.array([0, 1, 2, 1, 0xFF, 1], np.uint8), 15)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        for i, shift in enumerate((-1.0, 0.0, 1.5)):
            c.process_frame(synth.tunnel_frame(20000, seed=i, sigma=0.01))
            pose = np.eye(4)[:3].copy()
            pose[0, 3] = shift
            m.add_frame(0, pose)
        raw = m.read_raw()
        assert (raw["count"] >= 8).sum() > 1000
        info, rec, rows = check(m, p, raw, lo, hi, zone=zone, n_zones=3)
        assert info["under"] > 0 and info["over"] > 0 and info["within"] > 0 and rec["points"].sum() > 20000
        check(m, p, raw, lo, hi, 8, 30, zone=zone, n_zones=3, section_stations=1, min_count=3)


if __name__ == "__main__":
    _chunk_child(sys.argv[1])
