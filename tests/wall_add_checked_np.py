"""numpy twin of the add less the check's changed rows (gm_wall_map_add_*_checked, csrc/k_wall_add_checked.hip +
gm_wall_add_checked.hip; include/gm_hip.h states it).  The rule is integer from a row's delta on, so the twin is exact:
select() classes the rows (wall_check_np.POINT records, any order, duplicates allowed) and returns the set of skipped
indices; info() adds the point classes from the per-point (e fp32, cell) pairs of an add of the SAME cloud under the same
pose -- wall_np's conventions: cell is -1 unless mapped, e is NaN for a plane point -- so that the five point counts are
those of the library.  The map's bytes after a checked add are, by the defining property, those of a plain add of the
cloud with skipped() deleted: keep() is that filter."""
import numpy as np

import wall_check_np as wk

SKIP_NEG, SKIP_POS = 1, 2
NEG, POS, KEPT, REJECTED = range(4)
ROW_NAMES = ("rows_neg", "rows_pos", "rows_kept", "rows_rejected")
DEFAULTS = dict(skip=SKIP_NEG | SKIP_POS, min_delta=0.0)


def params(**kw):
    for k in kw:
        if k not in DEFAULTS:
            raise TypeError(f"unknown checked-add parameter {k!r}")
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_ok(skip=3, min_delta=0.0):
    """gm_wall_add_checked_check_params' rule."""
    return bool(skip in (1, 2, 3) and 0.0 <= float(min_delta) <= 8.0)


def min_delta_q(min_delta):
    """S = (int64) rint(min_delta 2^20) in fp64."""
    return int(np.rint(np.float64(min_delta) * 2.0 ** 20))


def classify_rows(rows, n_points, **kw):
    """Per row: NEG / POS (selected, by sign), KEPT or REJECTED, as uint8."""
    p = params(**kw)
    rows = np.asarray(rows, wk.POINT).reshape(-1)
    S = min_delta_q(p["min_delta"])
    delta = rows["delta"]
    dq = wk.fix(delta)                       # gm_wall_map_check_objects' own rule
    idx = rows["index"].astype(np.int64)
    rejected = (dq == 0) | ~np.isfinite(delta) | (idx >= int(n_points))
    neg = ~rejected & (dq < 0) & bool(p["skip"] & SKIP_NEG) & (-dq >= S)
    pos = ~rejected & (dq > 0) & bool(p["skip"] & SKIP_POS) & (dq >= S)
    cls = np.full(len(rows), KEPT, np.uint8)
    cls[rejected] = REJECTED
    cls[neg] = NEG
    cls[pos] = POS
    return cls


def select(rows, n_points, **kw):
    """(row classes uint8 [n_rows], skipped indices int64, ascending and unique)."""
    rows = np.asarray(rows, wk.POINT).reshape(-1)
    cls = classify_rows(rows, n_points, **kw)
    return cls, np.unique(rows["index"][cls <= POS].astype(np.int64))


def keep(n_points, skipped):
    """Boolean mask [n_points]: the points a plain add must take to give the checked add's bytes."""
    m = np.ones(int(n_points), bool)
    m[np.asarray(skipped, np.int64)] = False
    return m


def info(rows, e, cell, gate, labels=None, status=0, **kw):
    """The gm_wall_add_checked_info dict.  e, cell: per point of the WHOLE cloud, from an add under the same pose whose
    gate is `gate` (the map's), whether or not that add skipped anything (a skipped point's cell is not looked at)."""
    p = params(**kw)
    e = np.asarray(e, np.float32)
    cell = np.asarray(cell, np.int64)
    n = len(e)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    cls, skipped = select(rows, n, **p)
    live = keep(n, skipped)
    with np.errstate(invalid="ignore"):
        inside = np.abs(e) <= np.float32(gate)
    plane = live & (lab == 1)
    beyond = live & ~plane & ~inside
    mapped = live & ~plane & inside & (cell >= 0)
    outside = live & ~plane & inside & (cell < 0)
    d = dict(status=int(status), min_delta_q=min_delta_q(p["min_delta"]), n_points=n, n_rows=len(cls), reserved=0)
    for k, name in enumerate(ROW_NAMES):
        d[name] = int((cls == k).sum())
    d.update(skipped=len(skipped), plane=int(plane.sum()), beyond_gate=int(beyond.sum()), outside=int(outside.sum()),
             mapped=int(mapped.sum()))
    return d
