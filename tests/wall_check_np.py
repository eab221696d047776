"""numpy twin of the wall-map check (gm_wall_map_check_*, csrc/k_wall_check.hip + gm_wall_slot.hip; include/gm_hip.h states
it).  The rule is integer from e on, so the twin is exact: classify() applies it to per-point (e fp32, cell) pairs -- the
per-point outputs of an add or a check under the same pose and gate -- and a raw-cell table (wall_np.RAW_CELL, the
checked map's read_raw()); check() builds the info and the records from it.

A point's `cell` is -1 unless it is mapped; whether an unmapped point is plane, beyond_gate or outside is decided by the
label, e and the gate: plane when the label is 1, beyond_gate when not (|e| <= gate), else outside."""
import numpy as np

import wall_np as wn

MEAN, ENVELOPE = 0, 1
PLANE, BEYOND, OUTSIDE, UNSURVEYED, UNCHANGED, CHANGED_POS, CHANGED_NEG = range(7)
NAMES = ("plane", "beyond_gate", "outside", "unsurveyed", "unchanged", "changed_pos", "changed_neg")
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("delta", "<f4"), ("e", "<f4"), ("cell", "<i4"),
                  ("index", "<u4"), ("row", "<u4")])
DEFAULTS = dict(reference=MEAN, min_count=8, threshold=0.05, gate=1.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def threshold_q(threshold):
    """T = (int64) rint(threshold 2^20) in fp64."""
    return int(np.rint(np.float64(threshold) * 2.0 ** 20))


def fix(e):
    """(int64) rint(e 2^20): the fp32 product rounded to nearest even, saturating at the int32 range, 0 for a NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(e, np.float32) * np.float32(2.0 ** 20)
        r = np.rint(p.astype(np.float64))
    r = np.where(np.isnan(r), 0.0, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1))
    return r.astype(np.int64)


def div_toward_zero(s, c):
    """C's s / c on int64 (c > 0)."""
    s = np.asarray(s, np.int64)
    c = np.asarray(c, np.int64)
    q = np.abs(s) // c
    return np.where(s < 0, -q, q)


def classify(e, cell, raw, labels=None, **kw):
    """Per point: (delta int64, cls uint8).  e fp32 [n] (NaN for plane points), cell [n] (-1 unless mapped), raw: the
    map's RAW_CELL table (any shape; flattened)."""
    p = params(**kw)
    e = np.asarray(e, np.float32)
    cell = np.asarray(cell, np.int64)
    raw = np.asarray(raw).reshape(-1)
    n = len(e)
    T = threshold_q(p["threshold"])
    gate = np.float32(p["gate"])
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    with np.errstate(invalid="ignore"):
        inside = np.abs(e) <= gate
    cls = np.full(n, OUTSIDE, np.uint8)
    cls[~inside] = BEYOND
    cls[lab == 1] = PLANE
    delta = np.zeros(n, np.int64)
    m = (cell >= 0) & (lab != 1) & inside
    c = raw[cell[m]]
    usable = c["count"] >= p["min_count"]
    eq = fix(e[m])
    if p["reference"] == ENVELOPE:
        lq, hq = fix(wn.unordered(~c["min_key"])), fix(wn.unordered(c["max_key"]))
        d = np.where(eq > hq, eq - hq, np.where(eq < lq, eq - lq, 0))
    else:
        d = eq - div_toward_zero(c["sum"], np.maximum(c["count"].astype(np.int64), 1))
    d = np.where(usable, d, 0)
    k = np.where(d >= T, CHANGED_POS, np.where(d <= -T, CHANGED_NEG, UNCHANGED))
    cls[m] = np.where(usable, k, UNSURVEYED)
    delta[m] = d
    return delta, cls


def check(xyz, e, cell, raw, labels=None, rows=None, status=0, **kw):
    """(info dict, POINT records ascending by index) of a check over the valid cloud xyz [n,3] with the per-point (e, cell)
    pairs.  rows: the valid cloud's pad words (None: row = index, the stage call)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    delta, cls = classify(e, cell, raw, labels, **kw)
    info = dict(status=int(status), threshold_q=threshold_q(params(**kw)["threshold"]), n_points=len(xyz))
    for k, name in enumerate(NAMES):
        info[name] = int((cls == k).sum())
    pos, neg = delta[cls == CHANGED_POS], delta[cls == CHANGED_NEG]
    info["peak_pos"] = int(pos.max()) if len(pos) else 0
    info["peak_neg"] = int(neg.min()) if len(neg) else 0
    idx = np.flatnonzero(cls >= CHANGED_POS)
    rec = np.zeros(len(idx), POINT)
    rec["x"], rec["y"], rec["z"] = xyz[idx, 0], xyz[idx, 1], xyz[idx, 2]
    rec["delta"] = delta[idx].astype(np.float32) * np.float32(2.0 ** -20)
    rec["e"] = np.asarray(e, np.float32)[idx]
    rec["cell"] = np.asarray(cell, np.int64)[idx]
    rec["index"] = idx
    rec["row"] = idx if rows is None else np.asarray(rows).view(np.uint32).reshape(-1)[idx]
    return info, rec
