"""numpy twin of the wall map's profile fit per chainage section (gm_wall_map_sections, csrc/k_wall_sections.hip +
gm_wall.hip + gm_wall_host.hip; include/gm_hip.h states it).

sections() is the device rule in integers on a raw-cell table (wall_np.RAW_CELL, the map's read_raw()) with the solve
restated in Python floats, one operation per statement as the library's: exact, so every comparison with the device is
byte equality -- given the basis table the call used (gm_wall_section_basis; basis() is the numpy statement of it, which
may differ by one unit where the rint flips).  metrics() restates gm_wall_section_metrics."""
import math

import numpy as np

OK, TOO_FEW, SINGULAR, UNBOUNDED, FAILED_MASK, OPEN_ARC = 0, 1, 2, 4, 0xFF, 1 << 8
SECTION = np.dtype([("station_from", "<u4"), ("stations", "<u4"), ("status", "<u4"), ("usable", "<u4"), ("fitted", "<u4"),
                    ("accepted", "<u4"), ("rejected", "<u4"), ("largest_gap", "<u4"), ("points", "<u8"),
                    ("coef_q", "<i8", (9,)), ("rss", "<u8"), ("peak_out", "<i8"), ("peak_in", "<i8"),
                    ("peak_out_sector", "<u4"), ("peak_in_sector", "<u4")])
SUMS = np.dtype([("N", "<i8", (45,)), ("r", "<i8", (9,)), ("fitted", "<u4"), ("largest_gap", "<u4"), ("points", "<u8")])
DEFAULTS = dict(section_stations=4, harmonics=2, passes=3, min_count=8, min_columns=24, max_gap_deg=90.0, reject=0.05)
INFO_KEYS = ("station0", "n_stations", "n_sectors", "section_stations", "sections", "harmonics", "passes", "reject_q",
             "max_gap_sectors", "sections_ok", "sections_failed", "sections_open_arc", "empty", "unusable", "usable",
             "accepted", "rejected")
SAT = 1 << 24
U32_MAX = 2 ** 32 - 1
ONE = 1 << 20


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def fixed(x):
    """(int64) rint(x 2^20) in fp64: Tr."""
    return int(np.rint(np.float64(x) * 2.0 ** 20))


def params_ok(**kw):
    """gm_wall_section_check_params' rule."""
    p = params(**kw)
    if p["section_stations"] < 1 or not (0 <= p["harmonics"] <= 4) or not (1 <= p["passes"] <= 4):
        return False
    if p["min_count"] < 1 or p["min_columns"] < 1 or not (0.0 <= p["max_gap_deg"] <= 360.0):
        return False
    return bool(0.0 < p["reject"] <= 8.0) and fixed(p["reject"]) >= 1


def basis(ns, H):
    """The numpy statement of the basis table: int64 [ns, 1 + 2 H]."""
    phi = 2.0 * np.pi * (2.0 * np.arange(ns) + 1.0) / (2.0 * ns)
    B = np.zeros((ns, 1 + 2 * H), np.int64)
    B[:, 0] = ONE
    for h in range(1, H + 1):
        B[:, 2 * h - 1] = np.rint(np.cos(h * phi) * 2.0 ** 20)
        B[:, 2 * h] = np.rint(np.sin(h * phi) * 2.0 ** 20)
    return B


def div_toward_zero(s, c):
    s, c = np.asarray(s, np.int64), np.asarray(c, np.int64)
    return np.where(s >= 0, s // c, -((-s) // c))


def merged(raw, S):
    """(count uint64 [NS, ns], sum int64 [NS, ns]) of the columns of raw [n, ns]."""
    n, ns = raw.shape
    NS = (n + S - 1) // S
    cnt = np.zeros((NS, ns), np.uint64)
    sm = np.zeros((NS, ns), np.int64)
    for i in range(NS):
        blk = raw[i * S:min((i + 1) * S, n)]
        cnt[i] = blk["count"].astype(np.uint64).sum(0)
        sm[i] = np.where(blk["count"] > 0, blk["sum"], 0).sum(0)
    return cnt, sm


def columns(raw, S, min_count, base=None):
    """(empty, usable bool [NS, ns], m int64 [NS, ns] (0 where not usable), count uint64) of the window's raw cells."""
    cnt, sm = merged(raw, S)
    one = np.uint64(1)
    q = div_toward_zero(sm, np.maximum(cnt, one).astype(np.int64))
    empty, usable = cnt == 0, cnt >= np.uint64(min_count)
    if base is not None:
        bc, bs = merged(base, S)
        with np.errstate(over="ignore"):
            q = q - div_toward_zero(bs, np.maximum(bc, one).astype(np.int64))   # (wraps, as the device's)
        empty &= bc == 0
        usable &= bc >= np.uint64(min_count)
    return empty, usable, np.where(usable, np.clip(q, -SAT, SAT), 0), cnt


def largest_gap(sel):
    """The longest cyclic run of False in the bool vector sel."""
    ns = len(sel)
    idx = np.flatnonzero(sel)
    if len(idx) == 0:
        return ns
    return int((np.diff(np.concatenate([idx, idx[:1] + ns])) - 1).max())


def sums_of(B, m, sel, cnt):
    """One SUMS record over the selected columns."""
    P = B.shape[1]
    s = np.zeros((), SUMS)
    Bs, ms = B[sel], m[sel]
    N = Bs.T @ Bs
    idx = 0
    for p in range(P):
        for q in range(p, P):
            s["N"][idx] = N[p, q]
            idx += 1
    s["r"][:P] = Bs.T @ ms
    s["fitted"] = int(sel.sum())
    s["largest_gap"] = largest_gap(sel)
    s["points"] = int(cnt[sel].sum())
    return s


def solve(s, H, min_columns):
    """gm_wall_section_solve in Python floats, one operation per statement: (coef_q [9] ints, status)."""
    P = 1 + 2 * H
    zero = [0] * 9
    if int(s["fitted"]) < max(min_columns, P):
        return zero, TOO_FEW
    A = [[0.0] * P for _ in range(P)]
    L = [[0.0] * P for _ in range(P)]
    idx = 0
    for p in range(P):
        for q in range(p, P):
            A[p][q] = A[q][p] = float(int(s["N"][idx])) * 2.0 ** -40
            idx += 1
    b = [float(int(s["r"][p])) * 2.0 ** -20 for p in range(P)]
    for j in range(P):
        d = A[j][j]
        for k in range(j):
            t = L[j][k] * L[j][k]
            d = d - t
        if not d > 1e-12 * A[j][j]:
            return zero, SINGULAR
        ljj = math.sqrt(d)
        L[j][j] = ljj
        for i in range(j + 1, P):
            v = A[i][j]
            for k in range(j):
                t = L[i][k] * L[j][k]
                v = v - t
            L[i][j] = v / ljj
    y, c = [0.0] * P, [0.0] * P
    for i in range(P):
        v = b[i]
        for k in range(i):
            t = L[i][k] * y[k]
            v = v - t
        y[i] = v / L[i][i]
    for i in reversed(range(P)):
        v = y[i]
        for k in range(i + 1, P):
            t = L[k][i] * c[k]
            v = v - t
        c[i] = v / L[i][i]
    cq = list(zero)
    for p in range(P):
        rc = float(np.rint(c[p]))
        if not abs(rc) <= 16777216.0:
            return zero, UNBOUNDED
        cq[p] = int(rc)
    return cq, OK


def model(B, cq):
    """M_k of the coefficients cq (ints) on the table B: int64 [ns]."""
    P = B.shape[1]
    return (B @ np.asarray(cq[:P], np.int64) + (1 << 19)) >> 20


def sections(raw, station0=0, n=None, base=None, B=None, **kw):
    """(info dict, SECTION records, SUMS records of the last fitting pass that ran) of stations [station0, station0 + n)
    of the map's raw cells `raw` [n_stations, n_sectors]; base: the baseline's raw cells; B: the call's basis table."""
    p = params(**kw)
    ns = raw.shape[1]
    n = raw.shape[0] - station0 if n is None else n
    S, H, Pf = p["section_stations"], p["harmonics"], p["passes"]
    Tr = fixed(p["reject"])
    NS = (n + S - 1) // S
    B = basis(ns, H) if B is None else np.asarray(B, np.int64)
    gap_limit = int(math.floor(p["max_gap_deg"] * float(ns) / 360.0))
    info = dict.fromkeys(INFO_KEYS, 0)
    info.update(station0=station0, n_stations=n, n_sectors=ns, section_stations=S, sections=NS, harmonics=H, passes=Pf,
                reject_q=Tr, max_gap_sectors=gap_limit)
    rec, sums = np.zeros(NS, SECTION), np.zeros(NS, SUMS)
    if n == 0:
        return info, rec, sums
    win = raw[station0:station0 + n]
    bwin = base[station0:station0 + n] if base is not None else None
    empty, usable, m, cnt = columns(win, S, p["min_count"], bwin)
    info["empty"], info["usable"] = int(empty.sum()), int(usable.sum())
    info["unusable"] = NS * ns - info["empty"] - info["usable"]
    for i in range(NS):
        r = rec[i]
        r["station_from"] = station0 + i * S
        r["stations"] = min(S, n - i * S)
        r["usable"] = int(usable[i].sum())
        cq, status = [0] * 9, OK
        for ps in range(1, Pf + 1):
            sel = usable[i].copy()
            if ps > 1:
                sel &= np.abs(m[i] - model(B, cq)) <= Tr << (Pf - ps)
            sums[i] = sums_of(B, m[i], sel, cnt[i])
            cq, status = solve(sums[i], H, p["min_columns"])
            if status:
                break
        r["fitted"], r["largest_gap"] = sums[i]["fitted"], sums[i]["largest_gap"]
        r["status"] = status
        if status:
            r["peak_out_sector"] = r["peak_in_sector"] = U32_MAX
            info["sections_failed"] += 1
        else:
            rho = m[i] - model(B, cq)
            acc = usable[i] & (np.abs(rho) <= Tr)
            r["coef_q"] = cq
            r["accepted"] = int(acc.sum())
            r["rejected"] = int(r["usable"]) - int(r["accepted"])
            r["points"] = int(cnt[i][acc].sum())
            r["rss"] = int((rho[acc] * rho[acc]).sum())
            if r["usable"]:
                big = np.where(usable[i], rho, -(1 << 62))
                small = np.where(usable[i], rho, 1 << 62)
                r["peak_out"], r["peak_out_sector"] = big.max(), int(np.argmax(big))
                r["peak_in"], r["peak_in_sector"] = small.min(), int(np.argmin(small))
            else:
                r["peak_out_sector"] = r["peak_in_sector"] = U32_MAX
            info["sections_ok"] += 1
            info["accepted"] += int(r["accepted"])
            info["rejected"] += int(r["rejected"])
        if r["largest_gap"] > gap_limit:
            r["status"] |= OPEN_ARC
            info["sections_open_arc"] += 1
    return info, rec, sums


def metrics(wall, design, r, H):
    """gm_wall_section_metrics in Python floats on the gm_wall_params dict `wall` and wall_np.design_frame(wall)."""
    ds, t_min = float(wall["station_length"]), float(wall["t_min"])
    out = dict.fromkeys(("radius_m", "radial_m", "centre_u", "centre_v", "oval_m", "oval_angle_deg", "diameter_max",
                         "diameter_min", "rms_m", "area_m2", "coverage"), 0.0)
    out["chainage_from"] = t_min + float(int(r["station_from"])) * ds
    out["chainage_to"] = t_min + (float(int(r["station_from"])) + float(int(r["stations"]))) * ds
    out["centre"] = np.zeros(3)
    if int(r["status"]) & FAILED_MASK:
        return out
    P = 1 + 2 * H
    c = [float(int(r["coef_q"][q])) * 2.0 ** -20 if q < P else 0.0 for q in range(9)]
    radius = design["R"] + c[0]
    mid = (out["chainage_from"] + out["chainage_to"]) * 0.5
    out.update(radius_m=radius, radial_m=c[0], centre_u=c[1], centre_v=c[2])
    out["centre"] = np.array([((design["o"][k] + mid * design["a"][k]) + c[1] * design["u"][k]) + c[2] * design["v"][k]
                              for k in range(3)])
    oval = math.hypot(c[3], c[4])
    out["oval_m"] = oval
    if oval > 0.0:
        deg = ((math.atan2(c[4], c[3]) * 0.5) * 180.0) / math.pi
        if deg < 0.0:
            deg = deg + 180.0
        if deg >= 180.0:
            deg = deg - 180.0
        out["oval_angle_deg"] = deg
    out["diameter_max"], out["diameter_min"] = 2.0 * (radius + oval), 2.0 * (radius - oval)
    if int(r["accepted"]):
        out["rms_m"] = math.sqrt(float(int(r["rss"])) / float(int(r["accepted"]))) * 2.0 ** -20
    sq = 0.0
    for q in range(1, P):
        sq = sq + c[q] * c[q]
    out["area_m2"] = math.pi * (radius * radius) + (math.pi / 2) * sq
    out["coverage"] = float(int(r["accepted"])) / float(wall["n_sectors"])
    return out


def fill_series(ns, n, coef_m, count=16, noise=None):
    """Raw cells [n, ns] whose cell means are the Fourier series coef_m (metres: c0, a1, b1, ...) at the sector centres,
    exactly count times an integer value each (so the integer mean is that value), plus per-cell `noise` (units)."""
    H = (len(coef_m) - 1) // 2
    phi = 2.0 * np.pi * (2.0 * np.arange(ns) + 1.0) / (2.0 * ns)
    val = np.full(ns, coef_m[0], np.float64)
    for h in range(1, H + 1):
        val = val + coef_m[2 * h - 1] * np.cos(h * phi) + coef_m[2 * h] * np.sin(h * phi)
    q = np.rint(val * 2.0 ** 20).astype(np.int64)
    import wall_np as wn
    raw = np.zeros((n, ns), wn.RAW_CELL)
    v = np.broadcast_to(q, (n, ns)) + (0 if noise is None else noise)
    raw["sum"] = v * count
    raw["count"] = count
    e = (v * 2.0 ** -20).astype(np.float32)
    raw["min_key"], raw["max_key"] = ~wn.ordered(e), wn.ordered(e)
    return raw
