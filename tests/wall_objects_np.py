"""numpy twin of the check's objects (gm_wall_map_check_objects / gm_wall_check_objects, csrc/k_wall_objects.hip +
gm_wall_slot.hip; include/gm_hip.h states the rule).  Integer from the decoding of a row on, so the device must reproduce it
byte for byte: info, records, object_of_row.

For rows (wall_check_np.POINT), the map's n_stations and n_sectors, an anchor station and the parameters:
    per row   c = cell, j = c // n_sectors, k = c % n_sectors, dq = fix(delta) (rint(delta 2^20), fp32 product, saturating);
              rejected: c outside the map, dq == 0, or x, y, z, e not finite
    blocks    J = j // bs, K = k // bk, NK = ceil(n_sectors / bk), B = J NK + K (anchored on the map, ragged at the ends)
    window    stations [max(0, j_f - H), min(n_stations, j_f + H)) widened to the block rows J0 .. J1; a row outside them
              is outside_window, and so is every row that is not rejected when the window is empty
    planes    positive and negative rows apart: (B, s) is flagged iff it holds >= min_block_points rows; else sparse
    joined    flagged blocks of one sign at (J +- 1, K) inside the window, (J, (K +- 1) mod NK) and, with connectivity 8,
              (J +- 1, (K +- 1) mod NK)
    objects   components of >= min_points rows, ascending by (label = smallest B, sign); rows of the others are small
Components are found by a plain flood fill over a dictionary of flagged blocks -- no union-find, no tiles -- and the
records are computed with Python integers.
"""
import numpy as np

import wall_check_np as kn
import wall_np as wn

OBJECT = np.dtype([("label", "<u4"), ("sign", "<i4"), ("blocks", "<u4"), ("peak_index", "<u4"), ("station_min", "<u4"),
                   ("station_max", "<u4"), ("sector_min", "<u4"), ("sector_max", "<u4"), ("sector_min_turned", "<u4"),
                   ("sector_max_turned", "<u4"), ("points", "<u8"), ("peak", "<i8"), ("sum_delta", "<i8"), ("sum_x", "<i8"),
                   ("sum_y", "<i8"), ("sum_z", "<i8"), ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)), ("e_min", "<f4"),
                   ("e_max", "<f4"), ("reserved", "<u8")])
DEFAULTS = dict(block_stations=1, block_sectors=1, min_block_points=2, min_points=8, connectivity=8, half_window_stations=128)
INFO_KEYS = ("n_rows", "station0", "n_stations", "blocks_stations", "blocks_sectors", "rejected", "outside_window", "sparse",
             "small", "in_object", "flagged_pos", "flagged_neg", "components", "objects")
CLASSES = ("rejected", "outside_window", "sparse", "small", "in_object")
MAX_BLOCKS = 1 << 20


def fix16(x):
    """(int64) rint(x 2^16): the fp32 product rounded to nearest even, saturating at the int32 range, 0 for a NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(x, np.float32) * np.float32(2.0 ** 16)
        r = np.rint(p.astype(np.float64))
    r = np.where(np.isnan(r), 0.0, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1))
    return r.astype(np.int64)


def window(n_stations, n_sectors, anchor, p):
    """(J0, nJ, NK, station0, n_stations of the block rows); nJ = 0 for an empty window.  ValueError above MAX_BLOCKS."""
    bs, bk, H = int(p["block_stations"]), int(p["block_sectors"]), int(p["half_window_stations"])
    NK = -(-n_sectors // bk)
    lo, hi = max(0, int(anchor) - H), min(n_stations, int(anchor) + H)
    if lo >= hi:
        return 0, 0, NK, 0, 0
    J0, J1 = lo // bs, (hi - 1) // bs
    if (J1 - J0 + 1) * NK > MAX_BLOCKS:
        raise ValueError("the window holds more than 2^20 blocks")
    return J0, J1 - J0 + 1, NK, J0 * bs, min((J1 + 1) * bs, n_stations) - J0 * bs


def _neighbours(Jl, K, nJ, NK, conn8):
    for dj, dk in ((1, 0), (-1, 0), (0, 1), (0, -1)) + (((1, 1), (1, -1), (-1, 1), (-1, -1)) if conn8 else ()):
        if 0 <= Jl + dj < nJ:
            yield Jl + dj, (K + dk) % NK


def objects(rows, n_stations, n_sectors, anchor, **params):
    """(info dict, OBJECT array in (label, sign) order, object_of_row int32 [len(rows)])."""
    p = dict(DEFAULTS)
    p.update(params)
    rows = np.asarray(rows, kn.POINT).reshape(-1)
    n = len(rows)
    bs, bk = int(p["block_stations"]), int(p["block_sectors"])
    J0, nJ, NK, st0, nst = window(n_stations, n_sectors, anchor, p)
    cells = n_stations * n_sectors
    c = rows["cell"].astype(np.int64)
    dq = kn.fix(rows["delta"])
    finite = np.isfinite(rows["x"]) & np.isfinite(rows["y"]) & np.isfinite(rows["z"]) & np.isfinite(rows["e"])
    rejected = (c < 0) | (c >= cells) | (dq == 0) | ~finite
    cc = np.where(rejected, 0, c)
    j, k = cc // n_sectors, cc % n_sectors
    J, K = j // bs, k // bk
    outside = ~rejected & ((J < J0) | (J >= J0 + nJ))
    live = ~rejected & ~outside
    plane = (dq > 0).astype(np.int64)
    info = dict(n_rows=n, station0=st0, n_stations=nst, blocks_stations=nJ, blocks_sectors=NK, rejected=int(rejected.sum()),
                outside_window=int(outside.sum()), sparse=0, small=0, in_object=0, flagged_pos=0, flagged_neg=0, components=0,
                objects=0)
    of_row = np.full(n, -1, np.int32)
    # rows per (plane, window block)
    members = {}
    for i in np.flatnonzero(live):
        members.setdefault((int(plane[i]), int(J[i] - J0), int(K[i])), []).append(int(i))
    flagged = {key for key, idx in members.items() if len(idx) >= p["min_block_points"]}
    info["sparse"] = sum(len(idx) for key, idx in members.items() if key not in flagged)
    info["flagged_neg"] = sum(1 for key in flagged if key[0] == 0)
    info["flagged_pos"] = sum(1 for key in flagged if key[0] == 1)
    conn8 = p["connectivity"] == 8
    seen, found = set(), []
    for start in sorted(flagged):
        if start in seen:
            continue
        seen.add(start)
        comp, stack = [], [start]
        while stack:                                             # a plain flood fill
            pl, Jl, Kk = stack.pop()
            comp.append((pl, Jl, Kk))
            for nb in _neighbours(Jl, Kk, nJ, NK, conn8):
                key = (pl,) + nb
                if key in flagged and key not in seen:
                    seen.add(key)
                    stack.append(key)
        found.append(comp)
    info["components"] = len(found)
    recs = []
    half = n_sectors // 2
    for comp in found:
        idx = np.array(sorted(i for key in comp for i in members[key]), np.int64)
        if len(idx) < p["min_points"]:
            info["small"] += len(idx)
            continue
        info["in_object"] += len(idx)
        r = rows[idx]
        d = [int(x) for x in dq[idx]]
        mag = [min(abs(x), 2 ** 32 - 1) for x in d]
        best = max(zip(mag, (~r["index"].astype(np.uint32)).tolist()))      # the 64-bit key: |dq| << 32 | ~index
        jj, kk = j[idx], k[idx]
        tt = (kk + half) % n_sectors
        rec = np.zeros((), OBJECT)
        rec["label"] = min((J0 + Jl) * NK + Kk for _, Jl, Kk in comp)
        rec["sign"] = 1 if comp[0][0] else -1
        rec["blocks"] = len(comp)
        rec["peak_index"] = (~np.uint32(best[1])) & np.uint32(0xFFFFFFFF)
        rec["station_min"], rec["station_max"] = jj.min(), jj.max()
        rec["sector_min"], rec["sector_max"] = kk.min(), kk.max()
        rec["sector_min_turned"], rec["sector_max_turned"] = tt.min(), tt.max()
        rec["points"] = len(idx)
        rec["peak"] = best[0] if comp[0][0] else -best[0]
        rec["sum_delta"] = sum(d)
        for f in "xyz":
            rec["sum_" + f] = sum(int(v) for v in fix16(r[f]))
        for a, f in enumerate("xyz"):
            keys = wn.ordered(r[f])
            rec["box_min"][a] = wn.unordered(keys.min())
            rec["box_max"][a] = wn.unordered(keys.max())
        keys = wn.ordered(r["e"])
        rec["e_min"], rec["e_max"] = wn.unordered(keys.min()), wn.unordered(keys.max())
        recs.append((int(rec["label"]), int(rec["sign"]), rec, idx))
    recs.sort(key=lambda t: (t[0], t[1]))
    out = np.zeros(len(recs), OBJECT)
    for pos, (_, _, rec, idx) in enumerate(recs):
        out[pos] = rec
        of_row[idx] = pos
    info["objects"] = len(recs)
    assert sum(info[c_] for c_ in CLASSES) == n
    return info, out, of_row


def metrics(p, o):
    """gm_wall_object_metrics: p a dict of gm_wall_params fields, o one OBJECT record."""
    ns = int(p["n_sectors"])
    ds, t_min = float(p["station_length"]), float(p["t_min"])
    pts = float(int(o["points"]))
    sum_m = float(int(o["sum_delta"])) * 2.0 ** -20
    plain = int(o["sector_max"]) - int(o["sector_min"]) + 1
    turned = int(o["sector_max_turned"]) - int(o["sector_min_turned"]) + 1
    k_from, k_end = int(o["sector_min"]), int(o["sector_max"]) + 1
    if turned < plain:
        k_from = (int(o["sector_min_turned"]) + ns - ns // 2) % ns
        k_end = (int(o["sector_max_turned"]) + ns - ns // 2) % ns + 1
    return dict(centroid=np.array([float(int(o["sum_" + f])) * 2.0 ** -16 / pts for f in "xyz"]), mean_m=sum_m / pts,
                peak_m=float(int(o["peak"])) * 2.0 ** -20,
                size=np.array([float(o["box_max"][a]) - float(o["box_min"][a]) for a in range(3)]),
                chainage_from=t_min + float(int(o["station_min"])) * ds,
                chainage_to=t_min + (float(int(o["station_max"])) + 1.0) * ds,
                angle_from_deg=360.0 * float(k_from) / float(ns), angle_to_deg=360.0 * float(k_end) / float(ns))


def make_rows(cell, delta, index=None, xyz=None, e=None, seed=0):
    """POINT rows for the given cells and deltas; coordinates and residuals drawn from `seed` unless given."""
    cell = np.asarray(cell, np.int64)
    n = len(cell)
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, kn.POINT)
    xyz = rng.uniform(-5.0, 5.0, (n, 3)).astype(np.float32) if xyz is None else np.asarray(xyz, np.float32)
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rows["delta"] = np.asarray(delta, np.float32)
    rows["e"] = rng.uniform(-1.0, 1.0, n).astype(np.float32) if e is None else np.asarray(e, np.float32)
    rows["cell"] = cell.astype(np.int32)
    rows["index"] = np.arange(n, dtype=np.uint32) if index is None else np.asarray(index, np.uint32)
    rows["row"] = rows["index"]
    return rows
