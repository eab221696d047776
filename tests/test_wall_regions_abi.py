"""gm_wall_map_regions without a GPU: the symbols, the struct layouts from plain C99, the defaults, the host-only
gm_wall_region_metrics against the twin (tests/regions_np.py), the refusal of a NULL map, the twin's labelling against
scipy.ndimage.label on wrapped fields, and the end-to-end drive through the twins alone."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_np as rn  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_map_regions", "gm_wall_region_metrics", "gm_wall_region_default_params")


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert L.gm_abi_version() == 3


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_region": (_lib.WallRegion, "gm_wall_region"),
        "gm_wall_region_params": (_lib.WallRegionParams, "gm_wall_region_params"),
        "gm_wall_regions_info": (_lib.WallRegionsInfo, "gm_wall_regions_info"),
        "gm_wall_region_metrics": (_lib.WallRegionMetrics, "struct gm_wall_region_metrics"),
    }
    lines = []
    for _, (ct, cname) in sorted(fields.items()):
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
    want = []
    for _, (ct, _c) in sorted(fields.items()):
        want.append(C.sizeof(ct))
        want += [getattr(ct, f).offset for f, _t in ct._fields_]
    assert out == want
    assert C.sizeof(_lib.WallRegion) == 64 and api.REGION.itemsize == 64 and rn.REGION == api.REGION
    assert [api.REGION.fields[f][1] for f, _t in _lib.WallRegion._fields_] == [getattr(_lib.WallRegion, f).offset
                                                                             for f, _t in _lib.WallRegion._fields_]


def test_defaults():
    p = _lib.WallRegionParams()
    _lib.load().gm_wall_region_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallRegionParams)
    assert (p.min_count, p.min_cells, p.connectivity, p.threshold, p.reserved) == (8, 4, 8, 0.05, 0)
    assert {k: getattr(p, k) for k in rn.DEFAULTS} == rn.DEFAULTS
    _lib.load().gm_wall_region_default_params(None)   # a NULL is ignored


def _record(ns, cells_jk, d, first=0):
    """A REGION record of hand-made cells [(j, k)] with values d, by the rule."""
    r = np.zeros(1, rn.REGION)
    j = np.array([c[0] for c in cells_jk])
    k = np.array([c[1] for c in cells_jk])
    t = (k + ns // 2) % ns
    idx = j * ns + k
    pk = int(np.argmax(np.abs(d)))
    r[0] = (idx.min(), 1 if d[0] > 0 else -1, len(j), j.min(), j.max(), k.min(), k.max(), t.min(), t.max(), idx[pk], d[pk],
            int(np.sum(d)), 10 * len(j))
    return r[0]


METRIC_CASES = {
    # a region across the seam: sectors 88, 89, 0, 1 of 90 -- the turned extent (4 sectors) beats the plain one (90)
    "seam": (dict(), 90, [(10, 88), (10, 89), (10, 0), (11, 1)], [200000, 180000, 170000, 160000]),
    "ring": (dict(), 90, [(3, k) for k in range(90)], [-100000 - k for k in range(90)]),
    "one_sector": (dict(station_length=0.5, t_min=-3.0), 1, [(0, 0), (1, 0)], [70000, 90000]),
    "odd_seam": (dict(radius=3.1, t_min=1000.125), 7, [(5, 6), (5, 0)], [-60000, -65000]),
    "odd_plain": (dict(radius=3.1), 7, [(5, 2), (6, 3), (6, 4)], [60000, 65000, 61000]),
    "negative_sum": (dict(), 90, [(40, 20), (40, 21), (41, 21)], [-157286, -157000, -100001]),
}


@pytest.mark.parametrize("case", sorted(METRIC_CASES))
def test_metrics_against_the_twin(case):
    kw, ns, cells, d = METRIC_CASES[case]
    p = wn.params(n_sectors=ns, **kw)
    rec = _record(ns, cells, np.array(d, np.int64))
    got = api.wall_region_metrics(api.WallMap.params(**p), rec)
    want = rn.metrics(p, rec)
    assert got == want, (got, want)
    area = p["station_length"] * p["radius"] * 2 * np.pi / ns
    assert got["area_m2"] == pytest.approx(len(cells) * area, rel=1e-15)
    assert got["mean_m"] == pytest.approx(np.mean(d) * 2.0 ** -20, rel=1e-15)
    if case == "seam":
        assert (got["angle_from_deg"], got["angle_to_deg"]) == (352.0, 8.0)       # from > to: across 0 degrees
        assert (got["chainage_from"], got["chainage_to"]) == (2.5, 3.0)
    if case == "ring":
        assert (got["angle_from_deg"], got["angle_to_deg"]) == (0.0, 360.0)
        assert got["volume_m3"] < 0 and got["peak_m"] == -(100000 + 89) * 2.0 ** -20
    if case == "one_sector":
        assert (got["angle_from_deg"], got["angle_to_deg"]) == (0.0, 360.0)
        assert (got["chainage_from"], got["chainage_to"]) == (-3.0, -2.0)
    if case == "odd_seam":
        assert got["angle_from_deg"] == 360.0 * 6 / 7 and got["angle_to_deg"] == 360.0 * 1 / 7
    if case == "odd_plain":
        assert got["angle_from_deg"] == 360.0 * 2 / 7 and got["angle_to_deg"] == 360.0 * 5 / 7
    if case == "negative_sum":
        assert got["volume_m3"] < 0 and got["mean_m"] < 0 and got["peak_m"] == -157286 * 2.0 ** -20


def test_metrics_refuses_bad_arguments():
    L = _lib.load()
    p = api.WallMap.params()
    rec = np.zeros(1, rn.REGION)
    rec["cells"] = 1
    rp = rec.ctypes.data_as(C.POINTER(_lib.WallRegion))
    out = _lib.WallRegionMetrics()
    assert L.gm_wall_region_metrics(C.byref(p), rp, C.byref(out)) == _lib.GM_OK
    assert L.gm_wall_region_metrics(None, rp, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_region_metrics(C.byref(p), None, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    assert L.gm_wall_region_metrics(C.byref(p), rp, None) == _lib.GM_ERR_INVALID_ARG
    rec["sector_max"] = 90
    assert L.gm_wall_region_metrics(C.byref(p), rp, C.byref(out)) == _lib.GM_ERR_INVALID_ARG
    rec["sector_max"] = 0
    rec["cells"] = 0
    assert L.gm_wall_region_metrics(C.byref(p), rp, C.byref(out)) == _lib.GM_ERR_INVALID_ARG


def test_null_map_is_refused():
    L = _lib.load()
    info = _lib.WallRegionsInfo()
    got = C.c_uint32(7)
    assert L.gm_wall_map_regions(None, None, 0, 0, None, C.byref(info), None, 0, C.byref(got), None) == _lib.GM_ERR_INVALID_ARG


def test_twin_quotient_divides_toward_zero():
    s = np.array([-7, 7, -8, 8, -1, 0, 5], np.int64)
    c = np.array([2, 2, 2, 2, 3, 4, 0], np.uint32)
    assert rn.quotient(s, c).tolist() == [-3, 3, -4, 4, 0, 0, 0]
    assert rn.threshold_q(0.05) == 52429 and rn.threshold_q(0.075) == 78643


def _scipy_partition(mask, conn):
    """Components of a boolean field whose columns wrap, through scipy: one wrapped column is appended, and the labels
    of that column are identified with those of column 0 (the same cells)."""
    ndi = pytest.importorskip("scipy.ndimage")
    st = np.ones((3, 3), int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    lab, k = ndi.label(np.concatenate([mask, mask[:, :1]], axis=1), structure=st)
    parent = list(range(k + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(lab[:, 0], lab[:, -1]):
        if a:
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(k + 1)])[lab[:, :-1]]


@pytest.mark.parametrize("conn", (4, 8))
def test_twin_labelling_agrees_with_scipy(conn):
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(conn)
    for n, ns in ((1, 5), (7, 3), (40, 33), (65, 64), (30, 129)):
        for density in (0.35, 0.45, 0.6):
            u = rng.random((n, ns))
            sign = np.where(u < density / 2, 1, np.where(u < density, -1, 0)).astype(np.int8)
            lab = rn.label(sign, conn, first=0)
            assert np.array_equal(lab >= 0, sign != 0)
            for s in (1, -1):
                ref = _scipy_partition(sign == s, conn)
                m = sign == s
                pairs = set(zip(lab[m].tolist(), ref[m].tolist()))
                assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})   # a bijection
            flat = lab.reshape(-1)
            for name in np.unique(flat[flat >= 0]):
                assert name == np.flatnonzero(flat == name).min()   # the label is the smallest index


def drive_raw(seed):
    """The end-to-end drive through the twins: the raw cells of the map after every frame was added."""
    drive = synth.tunnel_drive(12, 150_000, seed=seed, sigma=0.01)
    p = wn.params(n_stations=208, **drive["design"])
    design = wn.design_frame(p)
    es, cs = [], []
    for cloud, pose in drive["frames"]:
        r = wn.points(cloud, None, wn.add_frame(design, p, pose), p)
        es.append(r["e"].astype(np.float32))
        cs.append(r["cell"])
    return p, wn.cells_from(np.concatenate(es), np.concatenate(cs), 208 * 90).reshape(208, 90)


E2E = dict(threshold=0.075, min_count=1, min_cells=4, connectivity=8)
# (sign, cells, stations, sectors): DRIVE_PATCHES on 0.25 m x 4 degree cells
E2E_REGIONS = ((1, 48, (40, 47), (5, 10)), (-1, 48, (100, 107), (79, 84)), (1, 40, (132, 135), (25, 34)))


def check_e2e(p, info, reg, metrics):
    assert info["regions"] == len(reg) == 3
    for r, m, (sign, cells, (j0, j1), (k0, k1)) in zip(reg, metrics, E2E_REGIONS):
        assert (r["sign"], r["cells"], r["station_min"], r["station_max"], r["sector_min"], r["sector_max"]) == (sign, cells, j0, j1, k0, k1)
        assert r["label"] == j0 * 90 + k0
        assert abs(abs(m["mean_m"]) - 0.15) <= 0.005 and np.sign(m["mean_m"]) == sign
        assert m["area_m2"] == cells * (0.25 * 2 * (2 * np.pi) / 90)
        assert (m["chainage_from"], m["chainage_to"]) == (j0 * 0.25, (j1 + 1) * 0.25)
        assert (m["angle_from_deg"], m["angle_to_deg"]) == (k0 * 4.0, (k1 + 1) * 4.0)


@pytest.mark.parametrize("seed", (21, 5))
def test_end_to_end_through_the_twins(seed):
    p, raw = drive_raw(seed)
    info, reg, labels = rn.regions(raw, **E2E)
    check_e2e(p, info, reg, [rn.metrics(p, r) for r in reg])
    q = np.abs(rn.quotient(raw["sum"], raw["count"])) * 2.0 ** -20
    hit = raw["count"] > 0
    print(f"seed {seed}: largest |q| unflagged {q[hit & (labels < 0)].max():.4f} m, smallest flagged {q[labels >= 0].min():.4f} m")
    assert q[hit & (labels < 0)].max() < 0.03 and q[labels >= 0].min() > 0.12   # 0.075 sits far from both
    assert info["components"] == 3 and info["flagged_pos"] == 88 and info["flagged_neg"] == 48
