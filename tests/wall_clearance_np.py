"""numpy twin of the wall map's clearance against a structure gauge (gm_wall_map_clearance, csrc/k_wall_clearance.hip +
gm_wall.hip; include/gm_hip.h states it), of the polygon helper and of the runs.

clearance() is the device rule in integers on a raw-cell table (wall_np.RAW_CELL, the map's read_raw()): exact, so every
comparison with the device is byte equality.  gauge_from_polygon() restates gm_wall_gauge_from_polygon in fp64 with
numpy's cos and sin: an entry may differ from the library's by one unit where the ceil flips.  gauge_by_sampling() is the
brute-force check of that rule: the boundary sampled densely.  runs() folds station records in integers and fp64 with
one rounding per operation, byte for byte."""
import numpy as np

import wall_check_np as ck
import wall_np as wn

MIN, MEAN = 0, 1
UNGAUGED, EMPTY, UNUSABLE, INFRINGED, TIGHT, CLEAR = range(6)
NAMES = ("ungauged", "empty", "unusable", "infringed", "tight", "clear")
STATION = np.dtype([("min_clearance", "<i8"), ("min_sector", "<u4"), ("usable", "<u4"), ("tight", "<u4"), ("infringed", "<u4"),
                    ("unsurveyed", "<u4"), ("gauge", "<u4")])
CELL = np.dtype([("cell", "<u4"), ("count", "<u4"), ("clearance", "<i8")])
RUN = np.dtype([("station_from", "<u4"), ("station_to", "<u4"), ("chainage_from", "<f8"), ("chainage_to", "<f8"),
                ("min_clearance", "<i8"), ("min_clearance_m", "<f8"), ("min_station", "<u4"), ("min_sector", "<u4"),
                ("angle_deg", "<f8"), ("tight", "<u8"), ("infringed", "<u8")])
DEFAULTS = dict(reference=MIN, min_count=8, margin=0.10)
INFO_KEYS = ("station0", "n_stations", "n_sectors", "margin_q", "radius_q", "ungauged", "empty", "unusable", "infringed", "tight",
             "clear", "stations_tight", "stations_infringed", "min_clearance", "min_cell")
I64_MAX, U32_MAX = 2 ** 63 - 1, 2 ** 32 - 1
SAT = 1 << 30


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def fixed(x):
    """(int64) rint(x 2^20) in fp64: R_q and T."""
    return int(np.rint(np.float64(x) * 2.0 ** 20))


def params_ok(wall, gauge_q, station_gauge=None, n=0, **kw):
    """gm_wall_clearance_check_params' rule on a gm_wall_params dict."""
    p = params(**kw)
    g = np.asarray(gauge_q)
    if g.ndim == 1:
        g = g.reshape(1, -1)
    if not (1 <= wall["n_sectors"] <= 4096) or p["reference"] not in (MIN, MEAN) or p["min_count"] < 1:
        return False
    if not (0.0 <= p["margin"] <= 8.0) or not (wall["radius"] > 0 and np.isfinite(wall["radius"])) or fixed(wall["radius"]) > 2 ** 32:
        return False
    if not (1 <= g.shape[0] <= 256) or g.shape[1] != wall["n_sectors"] or np.any(g < 0):
        return False
    return station_gauge is None or bool(np.all(np.asarray(station_gauge)[:n] < g.shape[0]))


def wall_value(raw, reference):
    """w per cell (int64; meaningless where count is 0)."""
    if reference == MEAN:
        q = ck.div_toward_zero(raw["sum"], np.maximum(raw["count"].astype(np.int64), 1))
        return np.clip(q, -SAT, SAT)
    return ck.fix(wn.unordered(~raw["min_key"]))


def classify(raw, G, radius_q, margin_q, reference, min_count):
    """(class uint8, c int64) of cells raw [n, ns] against the per-station gauge rows G [n, ns]."""
    count = raw["count"].astype(np.int64)
    c = radius_q + wall_value(raw, reference) - G.astype(np.int64)
    cls = np.where(c < 0, INFRINGED, np.where(c < margin_q, TIGHT, CLEAR)).astype(np.uint8)
    cls[count < min_count] = UNUSABLE
    cls[count == 0] = EMPTY
    cls[G == 0] = UNGAUGED
    return cls, np.where(cls >= INFRINGED, c, 0)


def clearance(raw, wall, station0=0, n=None, gauge_q=None, station_gauge=None, **kw):
    """(info dict, STATION records, CELL records) of stations [station0, station0 + n) of the map's raw cells `raw`
    [n_stations, n_sectors] under the gm_wall_params dict `wall`."""
    p = params(**kw)
    ns = raw.shape[1]
    n = raw.shape[0] - station0 if n is None else n
    g = np.asarray(gauge_q, np.int32)
    if g.ndim == 1:
        g = g.reshape(1, -1)
    sg = np.zeros(n, np.int64) if station_gauge is None else np.asarray(station_gauge, np.int64).reshape(-1)
    assert params_ok(wall, g, sg, n, **kw) and len(sg) == n and station0 + n <= raw.shape[0]
    T, Rq = fixed(p["margin"]), fixed(wall["radius"])
    win = raw[station0:station0 + n]
    cls, c = classify(win, g[sg], Rq, T, p["reference"], p["min_count"])
    info = dict(station0=station0, n_stations=n, n_sectors=ns, margin_q=T, radius_q=Rq)
    for k, name in enumerate(NAMES):
        info[name] = int((cls == k).sum())
    st = np.zeros(n, STATION)
    usable = cls >= INFRINGED
    cm = np.where(usable, c, I64_MAX)
    st["min_clearance"] = cm.min(axis=1) if ns and n else I64_MAX
    st["min_sector"] = np.where(usable.any(axis=1), cm.argmin(axis=1), U32_MAX) if n else 0   # argmin: the first among equals
    st["usable"] = usable.sum(axis=1)
    st["tight"] = (cls == TIGHT).sum(axis=1)
    st["infringed"] = (cls == INFRINGED).sum(axis=1)
    st["unsurveyed"] = ((cls == EMPTY) | (cls == UNUSABLE)).sum(axis=1)
    st["gauge"] = sg
    info["stations_tight"] = int((st["tight"] + st["infringed"] > 0).sum())
    info["stations_infringed"] = int((st["infringed"] > 0).sum())
    if usable.any():
        flat = cm.reshape(-1)
        at = int(flat.argmin())
        info["min_clearance"], info["min_cell"] = int(flat[at]), station0 * ns + at
    else:
        info["min_clearance"], info["min_cell"] = I64_MAX, U32_MAX
    idx = np.flatnonzero((cls == TIGHT) | (cls == INFRINGED))
    cells = np.zeros(len(idx), CELL)
    cells["cell"] = station0 * ns + idx
    cells["count"] = win["count"].reshape(-1)[idx]
    cells["clearance"] = c.reshape(-1)[idx]
    return info, st, cells


# ---- the tests' inputs ----

def random_raw(rng, n, ns, fill):
    """Raw cells as the cloud tests make them: counts 1 .. 20, sums of both signs, keys consistent through wn.ordered."""
    raw = np.zeros((n, ns), wn.RAW_CELL)
    hit = rng.random((n, ns)) < fill
    cnt = rng.integers(1, 21, (n, ns))
    lo = rng.uniform(-0.25, 0.0, (n, ns)).astype(np.float32)
    hi = rng.uniform(0.0, 0.25, (n, ns)).astype(np.float32)
    mean = rng.uniform(lo, hi)
    raw["count"] = np.where(hit, cnt, 0)
    raw["sum"] = np.where(hit, np.rint(mean * cnt * 2.0 ** 20).astype(np.int64), 0)
    raw["min_key"] = np.where(hit, ~wn.ordered(lo), 0)
    raw["max_key"] = np.where(hit, wn.ordered(hi), 0)
    return raw


def random_gauges(rng, n_gauges, ns, radius):
    """G = R_q + U(-0.3, 0.1) m, one sector in ten not gauged."""
    g = fixed(radius) + np.rint(rng.uniform(-0.3, 0.1, (n_gauges, ns)) * 2.0 ** 20).astype(np.int64)
    g[rng.random((n_gauges, ns)) < 0.1] = 0
    return g.astype(np.int32)


# ---- the polygon helper ----

def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _meet(a, b, c, d):
    o1, o2, o3, o4 = _cross(b - a, c - a), _cross(b - a, d - a), _cross(d - c, a - c), _cross(d - c, b - c)
    if ((o1 > 0 > o2) or (o1 < 0 < o2)) and ((o3 > 0 > o4) or (o3 < 0 < o4)):
        return True

    def on(p, q, r):
        return bool(np.all(np.minimum(p, q) <= r) and np.all(r <= np.maximum(p, q)))
    return (o1 == 0 and on(a, b, c)) or (o2 == 0 and on(a, b, d)) or (o3 == 0 and on(c, d, a)) or (o4 == 0 and on(c, d, b))


def polygon_ok(P):
    """The library's acceptance rule: 3 .. 4096 finite vertices, no edge of length 0, simple, the axis strictly inside."""
    P = np.asarray(P, np.float64).reshape(-1, 2)
    nv = len(P)
    if not (3 <= nv <= 4096) or not np.all(np.isfinite(P)):
        return False
    zero = np.zeros(2)
    wn_ = 0
    for i in range(nv):
        a, b = P[i], P[(i + 1) % nv]
        if np.array_equal(a, b):
            return False
        left = _cross(a, b)
        if left == 0 and _meet(a, b, zero, zero):
            return False
        if a[1] <= 0:
            wn_ += 1 if (b[1] > 0 and left > 0) else 0
        elif b[1] <= 0 and left < 0:
            wn_ -= 1
    if wn_ == 0:
        return False
    for i in range(nv):
        a, b = P[i], P[(i + 1) % nv]
        for j in range(i + 1, nv):
            c, d = P[j], P[(j + 1) % nv]
            nxt, prv = j == i + 1, (i == 0 and j == nv - 1)
            if nxt or prv:
                s, x, y = (b, a, d) if nxt else (a, b, c)
                e, f = x - s, y - s
                if _cross(e, f) == 0 and e @ f > 0:
                    return False
            elif _meet(a, b, c, d):
                return False
    return True


def gauge_from_polygon(uv, n_sectors, offset=(0.0, 0.0)):
    """int32 [n_sectors], or None for a polygon the library refuses."""
    P = np.asarray(uv, np.float64).reshape(-1, 2) + np.asarray(offset, np.float64)
    if not polygon_ok(P):
        return None
    ns, nv = n_sectors, len(P)
    phi = 2.0 * np.pi * (np.arange(ns, dtype=np.float64) / float(ns))
    d = np.stack([np.cos(phi), np.sin(phi)], axis=1)                 # [ns, 2]
    a, e = P, np.roll(P, -1, axis=0) - P                             # edges a + s e
    with np.errstate(divide="ignore", invalid="ignore"):
        den = e[None, :, 0] * d[:, None, 1] - e[None, :, 1] * d[:, None, 0]                 # cross(e, d)  [ns, nv]
        s = -(a[None, :, 0] * d[:, None, 1] - a[None, :, 1] * d[:, None, 0]) / den
        x = a[None] + s[..., None] * e[None]
        t = x[..., 0] * d[:, None, 0] + x[..., 1] * d[:, None, 1]
        ok = (den != 0) & (s >= 0) & (s <= 1) & (t >= 0)
    ray = np.where(ok, t, -1.0).max(axis=1)                          # [ns]
    r = np.hypot(P[:, 0], P[:, 1])
    d1 = np.roll(d, -1, axis=0)
    if ns == 1:
        inside = np.ones((1, nv), bool)
    else:
        inside = ((d[:, None, 0] * P[None, :, 1] - d[:, None, 1] * P[None, :, 0] >= 0) &
                  (P[None, :, 0] * d1[:, None, 1] - P[None, :, 1] * d1[:, None, 0] >= 0))
    g = np.maximum(np.maximum(ray, np.roll(ray, -1)), np.where(inside, r[None], -1.0).max(axis=1))
    q = np.ceil(g * 2.0 ** 20)
    if not np.all(g > 0) or not np.all(q < 2.0 ** 31):
        return None
    return q.astype(np.int32)


def gauge_by_sampling(uv, n_sectors, offset=(0.0, 0.0), samples=800_000):
    """fp64 [n_sectors] metres: the largest distance of `samples` boundary points per sector (they miss the true
    maximum by at most one sample spacing)."""
    P = np.asarray(uv, np.float64).reshape(-1, 2) + np.asarray(offset, np.float64)
    Q = np.roll(P, -1, axis=0)
    L = np.hypot(*(Q - P).T)
    per = np.maximum(2, np.ceil(samples * L / L.sum()).astype(int))
    pts = np.concatenate([P[i] + np.linspace(0.0, 1.0, per[i])[:, None] * (Q[i] - P[i]) for i in range(len(P))])
    phi = np.mod(np.arctan2(pts[:, 1], pts[:, 0]), 2 * np.pi)
    k = np.minimum((phi / (2 * np.pi) * n_sectors).astype(int), n_sectors - 1)
    out = np.zeros(n_sectors)
    np.maximum.at(out, k, np.hypot(pts[:, 0], pts[:, 1]))
    return out


# ---- runs ----

def runs(stations, wall, station0=0, max_gap=0):
    """RUN records of the STATION records of a window that starts at map station station0."""
    st = np.asarray(stations, STATION).reshape(-1)
    n = len(st)
    flagged = (st["tight"].astype(np.int64) + st["infringed"]) > 0
    ds, t_min, ns = np.float64(wall["station_length"]), np.float64(wall["t_min"]), wall["n_sectors"]
    out = []
    i = 0
    while i < n:
        if not flagged[i]:
            i += 1
            continue
        last = i
        j = i + 1
        while j < n and j - last <= max_gap + 1:
            if flagged[j]:
                last = j
            j += 1
        seg = st[i:last + 1]
        at = i + int(seg["min_clearance"].argmin())
        r = np.zeros(1, RUN)[0]
        r["station_from"], r["station_to"] = station0 + i, station0 + last
        r["chainage_from"] = t_min + np.float64(station0 + i) * ds
        r["chainage_to"] = t_min + (np.float64(station0 + last) + 1.0) * ds
        r["min_clearance"] = st["min_clearance"][at]
        r["min_clearance_m"] = np.float64(st["min_clearance"][at]) * 2.0 ** -20
        r["min_station"], r["min_sector"] = station0 + at, st["min_sector"][at]
        r["angle_deg"] = (360.0 * (np.float64(st["min_sector"][at]) * 2.0 + 1.0)) / (np.float64(ns) * 2.0)
        r["tight"], r["infringed"] = int(seg["tight"].sum(dtype=np.uint64)), int(seg["infringed"].sum(dtype=np.uint64))
        out.append(r)
        i = last + 1
    return np.array(out, RUN) if out else np.zeros(0, RUN)
