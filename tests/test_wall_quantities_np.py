"""The twin of gm_wall_map_quantities (tests/wall_quantities_np.py) against itself: the vectorised quantities() against
the scalar column() column by column, the identities of the rule, and the 2^60 bound in Python integers."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_np as wn  # noqa: E402
import wall_quantities_np as qn  # noqa: E402

SAT = qn.SAT


def _random_raw(rng, n, ns, fill=0.8, spread=300000):
    raw = np.zeros((n, ns), wn.RAW_CELL)
    raw["count"] = np.where(rng.random((n, ns)) < fill, rng.integers(1, 20, (n, ns)), 0)
    raw["sum"] = raw["count"].astype(np.int64) * rng.integers(-spread, spread, (n, ns)) + rng.integers(-3, 4, (n, ns)) * (raw["count"] > 0)
    return raw


def test_the_bound_at_the_extreme_inputs():
    """R_q = 2^32, q = +-2^24, tables at +-2^24, 4096 sectors: no product reaches 2^60, no record sum 2^52."""
    product, record = qn.ann_bound()
    assert product == 3 * SAT * (2 ** 33 + SAT) < 2 ** 60
    assert record < 2 ** 52
    # the same through column(): the widest ring a column can report
    c = qn.column(2 ** 32, 8, 8 * SAT, -SAT, SAT, base=(8, -8 * SAT))
    assert c["cls"] == qn.OVER and c["over_area"] == (3 * SAT * (2 * 2 ** 32 + SAT - SAT - SAT)) >> 20 and c["over_area"] * 4096 < 2 ** 52
    c = qn.column(2 ** 32, 8, -8 * SAT, SAT, SAT, base=(8, 8 * SAT))
    assert c["cls"] == qn.UNDER and c["under_area"] == (3 * SAT * (2 * 2 ** 32 + SAT + SAT - SAT)) >> 20


def test_quantities_equal_the_scalar_column_rule():
    rng = np.random.default_rng(2)
    n, ns, nz, S, mc = 10, 37, 4, 3, 5
    raw, base = _random_raw(rng, n, ns), _random_raw(rng, n, ns, 0.9)
    lo, hi = qn.random_tables(rng, 3, ns)
    zone = rng.integers(0, nz - 1, ns).astype(np.uint8)    # zone 3 has no sector
    zone[[4, 20]] = qn.NOT_MEASURED
    prof = np.array([2, 0, 1, 2], np.uint8)
    for b in (None, base):
        info, rec, rows = qn.quantities(raw, lo, hi, 2.0, 1, 9, base=b, section_profile=prof[:3], zone=zone, n_zones=nz,
                                        section_stations=S, min_count=mc)
        assert rec.shape == (3, nz) and rows.shape == (3, ns) and info["sections"] == 3
        for f in ("under", "within", "over", "unsurveyed", "points", "under_area", "over_area", "excess_area", "peak_under", "peak_over"):
            assert not rec[:, 3][f].any(), f
        assert np.all(rec[:, 3]["peak_under_sector"] == qn.U32_MAX)
        totals = dict.fromkeys(qn.CLASS_NAMES, 0)
        for i in range(3):
            j0, j1 = 1 + i * S, 1 + min((i + 1) * S, 9)
            want = np.zeros(nz, qn.QUANTITY)
            want["peak_under_sector"] = want["peak_over_sector"] = qn.U32_MAX
            for k in range(ns):
                blk = raw[j0:j1, k]
                cnt, sm = int(blk["count"].sum()), int(blk["sum"][blk["count"] > 0].sum())
                bb = None
                if b is not None:
                    bk = b[j0:j1, k]
                    bb = (int(bk["count"].sum()), int(bk["sum"][bk["count"] > 0].sum()))
                g = int(prof[i])
                c = qn.column(qn.radius_q(2.0), cnt, sm, int(lo[g, k]), int(hi[g, k]), bb, mc, int(zone[k]))
                totals[qn.CLASS_NAMES[c["cls"]]] += 1
                assert rows[i, k] == (qn.NO_VALUE if c["v"] is None else c["v"])
                if c["cls"] == qn.UNMEASURED:
                    continue
                w = want[zone[k]]
                name = {qn.UNDER: "under", qn.WITHIN: "within", qn.OVER: "over"}.get(c["cls"], "unsurveyed")
                w[name] += 1
                if c["v"] is not None:
                    w["points"] += cnt
                    for f in ("under_area", "over_area", "excess_area"):
                        w[f] += c[f]
                    if c["cls"] == qn.UNDER and -c["over_line"] > w["peak_under"]:
                        w["peak_under"], w["peak_under_sector"] = -c["over_line"], k
                    if c["over_line"] > 0 and c["over_line"] > w["peak_over"]:
                        w["peak_over"], w["peak_over_sector"] = c["over_line"], k
            for f in ("under", "within", "over", "unsurveyed", "points", "under_area", "over_area", "excess_area", "peak_under",
                      "peak_over", "peak_under_sector", "peak_over_sector"):
                assert np.array_equal(rec[i][f], want[f]), (i, f)
            assert np.all(rec[i]["station_from"] == j0) and np.all(rec[i]["stations"] == j1 - j0) and np.all(rec[i]["profile"] == prof[i])
        assert {k: info[k] for k in qn.CLASS_NAMES} == totals and info["unmeasured"] == 6
        assert np.all(rec["excess_area"] <= rec["over_area"])        # H >= L: the excess is part of the overbreak


def test_identities_of_the_rule():
    rng = np.random.default_rng(4)
    raw = _random_raw(rng, 8, 16, 1.0)
    zero = np.zeros(16, np.int32)
    # lo = hi = 0 against itself as the baseline: nothing moved
    info, rec, rows = qn.quantities(raw, zero, zero, 2.0, base=raw, min_count=1)
    assert info["within"] == 2 * 16 and np.all(rows == 0) and not rec["over_area"].any() and not rec["under_area"].any()
    # a wider pay line can only move OVER to WITHIN; over_area does not depend on hi
    lo, hi = qn.random_tables(rng, 1, 16)
    a = qn.quantities(raw, lo, hi, 2.0, min_count=1)
    b = qn.quantities(raw, lo, np.full(16, SAT, np.int32), 2.0, min_count=1)
    assert b[0]["over"] == 0 and b[0]["within"] == a[0]["within"] + a[0]["over"] and b[0]["under"] == a[0]["under"]
    assert np.array_equal(a[1]["over_area"], b[1]["over_area"]) and not b[1]["excess_area"].any()
    # n = 0 gives nothing; a window's records are the whole map's
    info, rec, rows = qn.quantities(raw, lo, hi, 2.0, 3, 0)
    assert rec.shape == (0, 1) and rows.shape == (0, 16) and info["sections"] == 0
    whole = qn.quantities(raw, lo, hi, 2.0, section_stations=4)
    part = qn.quantities(raw, lo, hi, 2.0, 4, 4, section_stations=4)
    assert part[1].tobytes() == whole[1][1:].tobytes() and part[2].tobytes() == whole[2][1:].tobytes()
    # ties resolve to the smallest sector
    flat = np.zeros((2, 16), wn.RAW_CELL)
    flat["count"], flat["sum"] = 8, 8 * 700
    info, rec, rows = qn.quantities(flat, zero, zero, 2.0, section_stations=2)
    assert rec[0, 0]["peak_over"] == 700 and rec[0, 0]["peak_over_sector"] == 0 and rec[0, 0]["peak_under_sector"] == qn.U32_MAX
