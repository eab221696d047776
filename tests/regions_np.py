"""numpy twin of gm_wall_map_regions (csrc/k_wall_regions.hip + gm_wall.hip; include/gm_hip.h states the rule).

Integer throughout, so the device must reproduce it byte for byte.  For raw cells (wall_np.RAW_CELL: sum int64 in units
of 2^-20 m, count):
    q        = sum / count by C integer division (toward zero): sign(sum) * (|sum| // count)
    d        = q, usable iff count >= min_count; with a baseline d = q(map) - q(baseline), usable iff both counts are
    T        = rint(threshold 2^20) in fp64
    sign     = +1 if usable and d >= T, -1 if usable and d <= -T, else 0
    joined   = neighbours of one non-zero sign: (j +- 1, k) inside the window, (j, (k +- 1) mod n_sectors) and, with
               connectivity 8, (j +- 1, (k +- 1) mod n_sectors): the sector index wraps, the station index does not
    label    = the smallest map-wide index j * n_sectors + k of the component; a region has >= min_cells cells
    classes  = flagged_pos, flagged_neg, empty (count 0, and the baseline's too), unusable (not empty, not usable)
Labelling is minimum-label propagation with pointer jumping over the wrapped grid; records and metrics are computed in
Python integers and fp64 in the order of operations gm_wall_region_metrics states.
"""
import math

import numpy as np

REGION = np.dtype([("label", "<u4"), ("sign", "<i4"), ("cells", "<u4"), ("station_min", "<u4"), ("station_max", "<u4"),
                   ("sector_min", "<u4"), ("sector_max", "<u4"), ("sector_min_turned", "<u4"), ("sector_max_turned", "<u4"),
                   ("peak_cell", "<u4"), ("peak", "<i8"), ("sum_d", "<i8"), ("points", "<u8")])
DEFAULTS = dict(min_count=8, min_cells=4, connectivity=8, threshold=0.05)
_BIG = np.int64(1) << 40


def threshold_q(threshold):
    return int(np.rint(np.float64(threshold) * np.float64(2.0 ** 20)))


def quotient(s, c):
    """C division toward zero of int64 sums by counts (0 where the count is 0)."""
    s = np.asarray(s, np.int64)
    c = np.asarray(c).astype(np.int64)
    return np.where(c > 0, np.sign(s) * (np.abs(s) // np.maximum(c, 1)), 0).astype(np.int64)


def cell_values(raw, base=None, min_count=8):
    """(d int64, usable, empty) of raw cells against the design or against the raw cells of a baseline."""
    d = quotient(raw["sum"], raw["count"])
    usable = raw["count"].astype(np.int64) >= min_count
    empty = raw["count"] == 0
    if base is not None:
        d = d - quotient(base["sum"], base["count"])
        usable &= base["count"].astype(np.int64) >= min_count
        empty &= base["count"] == 0
    return d, usable, empty


def signs(d, usable, T):
    return np.where(usable & (d >= T), 1, np.where(usable & (d <= -T), -1, 0)).astype(np.int8)


def _shift(a, dj, dk, fill):
    """a[j + dj, (k + dk) mod n_sectors], `fill` where j + dj leaves the window."""
    out = np.roll(a, -dk, axis=1) if dk else a
    if dj:
        pad = np.full((abs(dj), a.shape[1]), fill, a.dtype)
        out = np.concatenate([out[dj:], pad]) if dj > 0 else np.concatenate([pad, out[:dj]])
    return out


def label(sign, connectivity=8, first=0):
    """Component labels (n, n_sectors) int64 of a sign field: the smallest index first + j * n_sectors + k of the
    component, -1 where the sign is 0."""
    n, ns = sign.shape
    flagged = sign != 0
    own = np.arange(n * ns, dtype=np.int64).reshape(n, ns)
    lab = np.where(flagged, own, _BIG)
    steps = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    if connectivity == 8:
        steps += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    while True:
        new = lab
        for dj, dk in steps:
            same = flagged & (_shift(sign, dj, dk, 0) == sign)
            new = np.where(same, np.minimum(new, _shift(lab, dj, dk, _BIG)), new)
        flat = new.reshape(-1)
        while True:   # pointer jumping: a label is a cell of the same component with a label of its own
            jump = np.where(flat < _BIG, flat[np.minimum(flat, n * ns - 1)], _BIG)
            if np.array_equal(jump, flat):
                break
            flat = jump
        new = flat.reshape(n, ns)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(flagged, lab + first, -1).astype(np.int64)


def regions(raw, base=None, station0=0, n=None, **params):
    """The call on the raw cells (n_stations, n_sectors) of a map (and of a baseline): (info dict, REGION array ascending by
    label, labels (n, n_sectors) int32 with -1 outside regions)."""
    p = dict(DEFAULTS)
    p.update(params)
    ns = raw.shape[1]
    n = raw.shape[0] - station0 if n is None else n
    win = raw[station0:station0 + n]
    bwin = None if base is None else base[station0:station0 + n]
    T = threshold_q(p["threshold"])
    d, usable, empty = cell_values(win, bwin, p["min_count"])
    sg = signs(d, usable, T)
    first = station0 * ns
    lab = label(sg, p["connectivity"], first) if n else np.zeros((0, ns), np.int64)
    info = dict(station0=station0, n_stations=n, n_sectors=ns, threshold_q=T, flagged_pos=int((sg > 0).sum()),
                flagged_neg=int((sg < 0).sum()), unusable=int((~usable & ~empty).sum()), empty=int((~usable & empty).sum()))
    fl = lab.reshape(-1)
    idx = np.flatnonzero(fl >= 0)
    names, inv, counts = np.unique(fl[idx], return_inverse=True, return_counts=True)
    info["components"] = len(names)
    keep = counts >= p["min_cells"]
    info["regions"] = int(keep.sum())
    out = np.zeros(info["regions"], REGION)
    labels = np.where(keep[inv], fl[idx], -1) if len(idx) else np.zeros(0, np.int64)
    full = np.full(n * ns, -1, np.int64)
    full[idx] = labels
    dd, cc = d.reshape(-1), win["count"].reshape(-1)
    order = np.argsort(inv, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(counts)])
    r = 0
    for c in range(len(names)):
        if not keep[c]:
            continue
        cells = idx[order[bounds[c]:bounds[c + 1]]]          # window-local, ascending
        j, k = cells // ns + station0, cells % ns
        t = (k + ns // 2) % ns
        dv = [int(x) for x in dd[cells]]
        mag = [min(abs(x), 2 ** 32 - 1) for x in dv]
        pk = mag.index(max(mag))                               # the first: the smallest index among equals
        out[r] = (int(names[c]), 1 if dv[0] > 0 else -1, len(cells), j.min(), j.max(), k.min(), k.max(), t.min(), t.max(),
                  int(cells[pk]) + first, dv[pk], sum(dv), sum(int(x) for x in cc[cells]))
        r += 1
    return info, out, full.reshape(n, ns).astype(np.int32)


def cell_area(p):
    return float(p["station_length"]) * float(p["radius"]) * (2 * math.pi) / float(p["n_sectors"])


def metrics(p, r):
    """gm_wall_region_metrics: p a dict of gm_wall_params fields, r one REGION record."""
    ns = int(p["n_sectors"])
    ds, t_min = float(p["station_length"]), float(p["t_min"])
    area = cell_area(p)
    cells = int(r["cells"])
    sum_m = float(int(r["sum_d"])) * 2.0 ** -20
    plain = int(r["sector_max"]) - int(r["sector_min"]) + 1
    turned = int(r["sector_max_turned"]) - int(r["sector_min_turned"]) + 1
    k_from, k_end = int(r["sector_min"]), int(r["sector_max"]) + 1
    if turned < plain:
        k_from = (int(r["sector_min_turned"]) + ns - ns // 2) % ns
        k_end = (int(r["sector_max_turned"]) + ns - ns // 2) % ns + 1
    return dict(area_m2=float(cells) * area, volume_m3=sum_m * area, peak_m=float(int(r["peak"])) * 2.0 ** -20,
                mean_m=sum_m / float(cells), chainage_from=t_min + float(int(r["station_min"])) * ds,
                chainage_to=t_min + (float(int(r["station_max"])) + 1.0) * ds,
                angle_from_deg=360.0 * float(k_from) / float(ns), angle_to_deg=360.0 * float(k_end) / float(ns))


def raw_from(count, total, dtype):
    """Raw cells (dtype: RAW_CELL) with the given counts and sums, keys left empty: all the regions rule reads."""
    raw = np.zeros(np.shape(count), dtype)
    raw["count"] = count
    raw["sum"] = total
    return raw


def random_field(rng, n, ns, density, T, dtype, min_count=8):
    """A random +/0/- field as raw cells: a share `density` of the cells flagged, the sign drawn per block of 11 x 13 cells
    (so that inside a block the flagged cells of one sign have the density itself -- 0.41 and 0.59 are the 8- and
    4-connected percolation thresholds, where components are largest and most tangled -- and opposite signs meet along
    the block borders); the rest usable below the threshold, thin (count < min_count) or empty; magnitudes and counts
    vary, sums are not multiples of counts."""
    blocks = rng.choice(np.array([-1, 1]), (-(-n // 11), -(-ns // 13)))
    sg = np.where(rng.random((n, ns)) < density, np.repeat(np.repeat(blocks, 11, axis=0), 13, axis=1)[:n, :ns], 0)
    count = rng.integers(min_count, min_count + 40, (n, ns))
    q = np.where(sg != 0, sg * rng.integers(T, 3 * T, (n, ns)), rng.integers(-T + 1, T, (n, ns)))
    total = q * count + np.sign(q) * rng.integers(0, min_count, (n, ns))   # the remainder a division toward zero drops
    other = rng.random((n, ns))
    thin = (sg == 0) & (other < 0.1)
    count = np.where(thin, rng.integers(1, min_count, (n, ns)), count)
    gone = (sg == 0) & (other > 0.9)
    count = np.where(gone, 0, count)
    total = np.where(gone, 0, total)
    return raw_from(count.astype(np.uint32), total.astype(np.int64), dtype)
