"""numpy twin of the wall map's over- and underbreak per section and zone (gm_wall_map_quantities,
csrc/k_wall_quantities.hip + gm_wall.hip + gm_wall_host.hip; include/gm_hip.h states it).

quantities() is the device rule in integers on a raw-cell table (wall_np.RAW_CELL, the map's read_raw()): exact, so
every comparison with the device is byte equality.  column() restates gm_wall_quantity_column in Python integers,
metrics() and runs() restate gm_wall_quantity_metrics and gm_wall_quantity_runs in Python floats, one operation per
statement as the library's.  ann_bound() states the 2^60 bound at the extreme inputs in Python integers."""
import math

import numpy as np

QUANTITY = np.dtype([("station_from", "<u4"), ("stations", "<u4"), ("zone", "<u4"), ("profile", "<u4"), ("under", "<u4"),
                     ("within", "<u4"), ("over", "<u4"), ("unsurveyed", "<u4"), ("points", "<u8"), ("under_area", "<i8"),
                     ("over_area", "<i8"), ("excess_area", "<i8"), ("peak_under", "<i8"), ("peak_over", "<i8"),
                     ("peak_under_sector", "<u4"), ("peak_over_sector", "<u4")])
RUN = np.dtype([("station_from", "<u4"), ("stations", "<u4"), ("zone", "<u4"), ("sections", "<u4"), ("chainage_from", "<f8"),
                ("chainage_to", "<f8"), ("under", "<u8"), ("within", "<u8"), ("over", "<u8"), ("unsurveyed", "<u8"),
                ("points", "<u8"), ("under_volume_m3", "<f8"), ("over_volume_m3", "<f8"), ("excess_volume_m3", "<f8"),
                ("paid_volume_m3", "<f8"), ("peak_under", "<i8"), ("peak_over", "<i8"), ("peak_under_station", "<u4"),
                ("peak_under_sector", "<u4"), ("peak_over_station", "<u4"), ("peak_over_sector", "<u4")])
DEFAULTS = dict(section_stations=4, min_count=8)
INFO_KEYS = ("station0", "n_stations", "n_sectors", "section_stations", "sections", "n_zones", "n_profiles", "radius_q",
             "unmeasured", "empty", "unusable", "under", "over", "within", "sections_under", "sections_over")
UNMEASURED, EMPTY, UNUSABLE, UNDER, OVER, WITHIN = range(6)
CLASS_NAMES = ("unmeasured", "empty", "unusable", "under", "over", "within")
NOT_MEASURED = 0xFF
SAT = 1 << 24
U32_MAX = 2 ** 32 - 1
NO_VALUE = -2 ** 31
MAX_PROFILES, MAX_ZONES, MAX_SECTORS = 256, 8, 4096


def radius_q(radius):
    """(int64) rint(radius 2^20) in fp64: R_q."""
    return int(np.rint(np.float64(radius) * 2.0 ** 20))


def params_ok(radius, n_sectors, lo, hi, n_profiles, section_profile=None, n=0, zone=None, n_zones=1, **kw):
    """gm_wall_quantity_check_params' rule on the tables as sequences."""
    p = dict(DEFAULTS)
    p.update(kw)
    if not (1 <= n_sectors <= MAX_SECTORS) or not (radius > 0.0 and math.isfinite(radius)) or radius_q(radius) > 2 ** 32:
        return False
    if p["section_stations"] < 1 or p["min_count"] < 1 or not (1 <= n_profiles <= MAX_PROFILES) or not (1 <= n_zones <= MAX_ZONES):
        return False
    lo, hi = np.asarray(lo, np.int64).reshape(-1), np.asarray(hi, np.int64).reshape(-1)
    if np.any(lo < -SAT) or np.any(hi > SAT) or np.any(lo > hi):
        return False
    NS = (n + p["section_stations"] - 1) // p["section_stations"]
    if section_profile is not None and any(int(g) >= n_profiles for g in list(section_profile)[:NS]):
        return False
    if zone is not None and any(int(z) >= n_zones and int(z) != NOT_MEASURED for z in zone):
        return False
    return True


def toward_zero(s, c):
    """C division of Python integers."""
    return abs(s) // c if s >= 0 else -(abs(s) // c)


def ann(a, b):
    """((b - a) (b + a)) >> 20 for b >= a >= 0."""
    assert 0 <= a <= b
    return ((b - a) * (b + a)) >> 20


def column(Rq, count, total, lo, hi, base=None, min_count=8, zone_entry=0):
    """gm_wall_quantity_column in Python integers: the class, v (None when the column is not usable), the three area terms
    and x - L; base: the baseline's (count, sum) or None."""
    out = dict(cls=UNUSABLE, v=None, under_area=0, over_area=0, excess_area=0, over_line=0)
    unmeasured = zone_entry == NOT_MEASURED
    usable = count >= min_count and (base is None or base[0] >= min_count)
    if count == 0 and (base is None or base[0] == 0):
        out["cls"] = EMPTY
    if unmeasured:
        out["cls"] = UNMEASURED
    if not usable:
        return out
    q = max(-SAT, min(SAT, toward_zero(total, count)))
    b0 = Rq if base is None else Rq + max(-SAT, min(SAT, toward_zero(base[1], base[0])))
    x = Rq + q
    L, H = b0 + lo, b0 + hi
    out["v"], out["over_line"] = x - b0, x - L
    if unmeasured:
        return out
    xc, Lc, Hc = max(x, 0), max(L, 0), max(H, 0)
    if out["v"] < lo:
        out["cls"] = UNDER
        out["under_area"] = ann(xc, Lc)
    elif out["v"] > hi:
        out["cls"] = OVER
        out["excess_area"] = ann(Hc, xc)
    else:
        out["cls"] = WITHIN
    if x > L:
        out["over_area"] = ann(Lc, xc)
    return out


def ann_bound():
    """The bound of include/gm_hip.h at the extreme inputs, in Python integers: the largest product of an area term, the
    largest sum of a record."""
    Rq = 2 ** 32
    worst = 0
    for q in (-SAT, SAT):
        for qb in (None, -SAT, SAT):
            for lo, hi in ((-SAT, -SAT), (-SAT, SAT), (SAT, SAT)):
                b0 = Rq if qb is None else Rq + qb
                x, L, H = Rq + q, b0 + lo, b0 + hi
                for a, b in ((x, L), (L, x), (H, x)):
                    a, b = max(a, 0), max(b, 0)
                    if b >= a:
                        assert b - a < 2 ** 26 and b + a < 2 ** 34
                        worst = max(worst, (b - a) * (b + a))
    return worst, (worst >> 20) * MAX_SECTORS


def merged(raw, S):
    """(count, sum) int64 [NS, ns] of the columns of raw [n, ns]: an empty cell adds nothing."""
    n, ns = raw.shape
    NS = (n + S - 1) // S
    cnt, sm = np.zeros((NS, ns), np.int64), np.zeros((NS, ns), np.int64)
    for i in range(NS):
        blk = raw[i * S:min((i + 1) * S, n)]
        cnt[i] = blk["count"].astype(np.int64).sum(0)
        sm[i] = np.where(blk["count"] > 0, blk["sum"], 0).sum(0)
    return cnt, sm


def _q(sm, cnt):
    c = np.maximum(cnt, 1)
    return np.clip(np.where(sm >= 0, sm // c, -((-sm) // c)), -SAT, SAT)


def quantities(raw, lo, hi, radius, station0=0, n=None, base=None, section_profile=None, zone=None, n_zones=1, **kw):
    """(info dict, QUANTITY records [NS, n_zones], int32 profile rows [NS, ns]) of stations [station0, station0 + n) of the
    map's raw cells `raw` [n_stations, n_sectors] against lo / hi [n_profiles, ns]; base: the baseline's raw cells."""
    p = dict(DEFAULTS)
    p.update(kw)
    ns = raw.shape[1]
    n = raw.shape[0] - station0 if n is None else n
    S, mc = p["section_stations"], p["min_count"]
    NS = (n + S - 1) // S
    lo, hi = np.asarray(lo, np.int64).reshape(-1, ns), np.asarray(hi, np.int64).reshape(-1, ns)
    Rq = radius_q(radius)
    info = dict.fromkeys(INFO_KEYS, 0)
    info.update(station0=station0, n_stations=n, n_sectors=ns, section_stations=S, sections=NS, n_zones=n_zones,
                n_profiles=lo.shape[0], radius_q=Rq)
    rec, rows = np.zeros((NS, n_zones), QUANTITY), np.full((NS, ns), NO_VALUE, np.int32)
    if n == 0:
        return info, rec, rows
    zone = np.zeros(ns, np.int64) if zone is None else np.asarray(zone, np.int64)
    measured = zone != NOT_MEASURED
    cnt, sm = merged(raw[station0:station0 + n], S)
    usable, empty = cnt >= mc, cnt == 0
    x = Rq + _q(sm, cnt)
    b0 = np.full((NS, ns), Rq, np.int64)
    if base is not None:
        bc, bs = merged(base[station0:station0 + n], S)
        usable &= bc >= mc
        empty &= bc == 0
        b0 = Rq + _q(bs, bc)
    for i in range(NS):
        g = int(section_profile[i]) if section_profile is not None else 0
        L, H = b0[i] + lo[g], b0[i] + hi[g]
        v = x[i] - b0[i]
        rows[i] = np.where(usable[i], v, NO_VALUE)
        m_use = measured & usable[i]
        under, over = m_use & (v < lo[g]), m_use & (v > hi[g])
        within, above = m_use & ~under & ~over, m_use & (x[i] > L)
        xc, Lc, Hc = np.maximum(x[i], 0), np.maximum(L, 0), np.maximum(H, 0)
        ua = np.where(under, ((Lc - xc) * (Lc + xc)) >> 20, 0)
        oa = np.where(above, ((xc - Lc) * (xc + Lc)) >> 20, 0)
        ea = np.where(over, ((xc - Hc) * (xc + Hc)) >> 20, 0)
        info["unmeasured"] += int((~measured).sum())
        info["empty"] += int((measured & empty[i]).sum())
        info["unusable"] += int((measured & ~empty[i] & ~usable[i]).sum())
        info["under"] += int(under.sum())
        info["over"] += int(over.sum())
        info["within"] += int(within.sum())
        info["sections_under"] += int(under.any())
        info["sections_over"] += int(over.any())
        for z in range(n_zones):
            r = rec[i, z]
            mine = zone == z
            r["station_from"] = station0 + i * S
            r["stations"] = min(S, n - i * S)
            r["zone"], r["profile"] = z, g
            r["under"], r["within"], r["over"] = int((mine & under).sum()), int((mine & within).sum()), int((mine & over).sum())
            r["unsurveyed"] = int((mine & ~usable[i]).sum())
            r["points"] = int(cnt[i][mine & usable[i]].sum())
            r["under_area"], r["over_area"], r["excess_area"] = int(ua[mine].sum()), int(oa[mine].sum()), int(ea[mine].sum())
            r["peak_under_sector"] = r["peak_over_sector"] = U32_MAX
            if (mine & under).any():
                d = np.where(mine & under, L - x[i], -1)
                r["peak_under"], r["peak_under_sector"] = d.max(), int(np.argmax(d))   # (argmax: the first among equals)
            if (mine & above).any():
                d = np.where(mine & above, x[i] - L, -1)
                r["peak_over"], r["peak_over_sector"] = d.max(), int(np.argmax(d))
    assert sum(info[k] for k in CLASS_NAMES) == NS * ns
    return info, rec, rows


def _angle(sector, ns):
    return (360.0 * (float(sector) * 2.0 + 1.0)) / (float(ns) * 2.0)


def _volumes(wall, r, length):
    """(areas [4], volumes [4]) of a record: under, over, excess, paid."""
    units = (int(r["under_area"]), int(r["over_area"]), int(r["excess_area"]), int(r["over_area"]) - int(r["excess_area"]))
    areas = [((float(u) * 2.0 ** -20) * math.pi) / float(wall["n_sectors"]) for u in units]
    return areas, [a * length for a in areas]


def metrics(wall, r):
    """gm_wall_quantity_metrics in Python floats on the gm_wall_params dict `wall`."""
    ds, t_min, ns = float(wall["station_length"]), float(wall["t_min"]), int(wall["n_sectors"])
    sf, st = float(int(r["station_from"])), float(int(r["stations"]))
    out = dict(chainage_from=t_min + sf * ds, chainage_to=t_min + (sf + st) * ds, length=st * ds)
    areas, vols = _volumes(wall, r, out["length"])
    for name, a, v in zip(("under", "over", "excess", "paid"), areas, vols):
        out[name + "_area_m2"], out[name + "_volume_m3"] = a, v
    for name in ("peak_under", "peak_over"):
        out[name + "_m"] = float(int(r[name])) * 2.0 ** -20
        k = int(r[name + "_sector"])
        out[name + "_angle_deg"] = _angle(k, ns) if k != U32_MAX else 0.0
    usable = int(r["under"]) + int(r["within"]) + int(r["over"])
    measured = usable + int(r["unsurveyed"])
    out["coverage"] = float(usable) / float(measured) if measured else 0.0
    return out


def runs(wall, records, n_zones=1, run_sections=1, all_zones=False):
    """gm_wall_quantity_runs in Python on the records [NS, n_zones]."""
    rec = np.asarray(records, QUANTITY).reshape(-1, n_zones)
    NS = len(rec)
    NR, per = (NS + run_sections - 1) // run_sections, 1 if all_zones else n_zones
    ds, t_min = float(wall["station_length"]), float(wall["t_min"])
    out = np.zeros(NR * per, RUN)
    for R in range(NR):
        s0, s1 = R * run_sections, min((R + 1) * run_sections, NS)
        for o in range(per):
            run = out[R * per + o]
            run["station_from"] = rec[s0, 0]["station_from"]
            run["zone"] = U32_MAX if all_zones else o
            run["sections"] = s1 - s0
            for f in ("peak_under_station", "peak_under_sector", "peak_over_station", "peak_over_sector"):
                run[f] = U32_MAX
            vol = [0.0, 0.0, 0.0, 0.0]
            stations = 0
            for s in range(s0, s1):
                stations += int(rec[s, 0]["stations"])
                length = float(int(rec[s, 0]["stations"])) * ds
                for z in (range(n_zones) if all_zones else (o,)):
                    r = rec[s, z]
                    for f in ("under", "within", "over", "unsurveyed", "points"):
                        run[f] += r[f]
                    _, v = _volumes(wall, r, length)
                    vol = [a + b for a, b in zip(vol, v)]
                    for name in ("peak_under", "peak_over"):
                        if int(r[name + "_sector"]) != U32_MAX and int(r[name]) > int(run[name]):
                            run[name], run[name + "_station"], run[name + "_sector"] = r[name], r["station_from"], r[name + "_sector"]
            run["stations"] = stations
            run["under_volume_m3"], run["over_volume_m3"], run["excess_volume_m3"], run["paid_volume_m3"] = vol
            sf = float(int(run["station_from"]))
            run["chainage_from"] = t_min + sf * ds
            run["chainage_to"] = t_min + (sf + float(stations)) * ds
    return out


def random_tables(rng, n_profiles, ns, spread=0.3):
    """(lo, hi) int32 [n_profiles, ns] with lo <= hi, a few entries at the limits."""
    a = np.rint(rng.uniform(-spread, spread, (2, n_profiles, ns)) * 2 ** 20).astype(np.int64)
    lo, hi = a.min(0), a.max(0)
    edge = rng.random((n_profiles, ns))
    lo[edge < 0.02], hi[edge > 0.98] = -SAT, SAT
    same = (edge > 0.45) & (edge < 0.55)
    hi[same] = lo[same]
    return lo.astype(np.int32), hi.astype(np.int32)
