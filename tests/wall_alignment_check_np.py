"""numpy twin of the check on a wall alignment (gm_wall_alignment_check_*, csrc/k_wall_check_joint.hip +
gm_wall_alignment.hip; include/gm_hip.h states the rule), written from the header.

It composes what the other twins already hold: the owner by the add's fp32 rule (wall_alignment_np.owner32), the owner's
chain on its per-add block (wall_alignment_locate_np.side_chain on the blocks of the plan's start, which ARE the sides'
per-add frames), and the check's integer rule on the owner's raw cells (wall_check_np.classify).  check() returns the info
of gm_wall_alignment_check_info, the rows with cell = side << 24 | cell, and the per-point side, cell, delta and class.

FAULTS names two deliberate errors that the assertions of tests/test_wall_alignment_check_np.py must catch: the owner
taken from the joints in the wrong order (the HIGHEST joint with d < 0 wins), and the gather from the neighbour's table.
"""
import numpy as np

import wall_alignment_locate_np as aln
import wall_alignment_np as al_np
import wall_check_np as wc

F = np.float32
FAULTS = ("joint_order", "neighbour_table")
N_CLS = len(wc.NAMES)


def sides_of(xyz, add, fault=None):
    """The owner of every point as an index into the plan's sides, int64 [n]."""
    ns = add["n_sides"]
    if fault == "joint_order":
        side = np.full(len(xyz), ns - 1, np.int64)
        for k in range(ns - 1):   # ascending overwrite: the HIGHEST joint with d < 0 stays, not the lowest
            side[al_np.joint_d32(xyz, add["joint_o"][k], add["joint_a"][k]) < 0.0] = k
        return side
    return al_np.owner32(xyz, dict(n_sides=ns, side_element=list(range(ns)), joint_o=add["joint_o"], joint_a=add["joint_a"])).astype(np.int64)


def split_cell(rows):
    """(side, cell) of rows whose cell holds side << 24 | cell."""
    c = np.asarray(rows["cell"]).view(np.uint32)
    return (c >> np.uint32(24)).astype(np.int64), (c & np.uint32(0xFFFFFF)).astype(np.int64)


def chains(xyz, plan, grid, n_stations, side):
    """Per point, on its owner's chain alone: (e float32, cell int64 relative to the owner's map, -1 unless the chain maps
    the point).  e of a point whose guard fails is NaN, which the check's rule classes beyond_gate."""
    state = dict(o=plan["c"], a=plan["d"], u=plan["u"], v=plan["v"])
    blk = aln.blocks(plan, state)
    pf = aln.plan_fields(plan)
    n = len(xyz)
    e, cell = np.full(n, np.nan, F), np.full(n, -1, np.int64)
    for k in range(len(pf["side_element"])):
        sel = np.flatnonzero(side == k)
        r = aln.side_chain(xyz[sel], pf["side_kind"][k], blk["side"][k], pf["side_axis"][k], grid, int(pf["side_anchor"][k]), n_stations[k])
        e[sel] = np.where(r["guard"], np.asarray(r["e"], F), np.nan)
        cell[sel] = np.where(r["guard"], r["cell"], -1)
    return e, cell


def check(xyz, labels, plan, grid, n_stations, raws, fault=None, **kw):
    """The whole check under the locate plan `plan` (WallAlignmentRule.locate_plan of the check's pose).  n_stations and
    raws are per side: the owner's station count and RAW_CELL table."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    add = plan["add"]
    ns = add["n_sides"]
    n = len(xyz)
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    side = sides_of(xyz, add, fault)
    e, cell = chains(xyz, plan, grid, n_stations, side)
    p = wc.params(**kw)
    with np.errstate(invalid="ignore"):
        cell = np.where(np.abs(e) <= F(p["gate"]), cell, -1)   # (the chain stops at the gate: no station, no cell)
    cell = np.where(lab == 1, -1, cell)
    delta, cls = np.zeros(n, np.int64), np.zeros(n, np.uint8)
    for k in range(ns):
        sel = np.flatnonzero(side == k)
        table = raws[(k + 1) % ns if fault == "neighbour_table" else k]
        c = np.where(cell[sel] < len(np.asarray(table).reshape(-1)), cell[sel], -1)
        delta[sel], cls[sel] = wc.classify(e[sel], c, table, lab[sel], **kw)
    info = dict(threshold_q=wc.threshold_q(p["threshold"]), n_points=n, n_sides=ns,
                side_class=np.array([[int(((side == k) & (cls == q)).sum()) for q in range(N_CLS)] for k in range(ns)], np.uint32))
    for q, name in enumerate(wc.NAMES):
        info[name] = int((cls == q).sum())
    pos, neg = delta[cls == wc.CHANGED_POS], delta[cls == wc.CHANGED_NEG]
    info["peak_pos"] = int(pos.max()) if len(pos) else 0
    info["peak_neg"] = int(neg.min()) if len(neg) else 0
    idx = np.flatnonzero(cls >= wc.CHANGED_POS)
    rows = np.zeros(len(idx), wc.POINT)
    rows["x"], rows["y"], rows["z"] = xyz[idx, 0], xyz[idx, 1], xyz[idx, 2]
    rows["delta"] = delta[idx].astype(F) * F(2.0 ** -20)
    rows["e"] = e[idx]
    rows["cell"] = ((side[idx] << 24) | cell[idx]).astype(np.uint32).view(np.int32)
    rows["index"] = idx
    rows["row"] = idx
    return dict(info=info, rows=rows, side=side, e=e, cell=cell, delta=delta, cls=cls)


def assert_partition(t, xyz, labels, add, raws, log=print, **kw):
    """What a check through an alignment must satisfy, whoever computed it (t: check()'s dict; add: the check's plan):
    the owners are owner32's; every point is in exactly one (side, class); the rows of side i are wall_check_np.check of
    the sub-cloud side i owns, with the indices mapped back; the summed classes and the peaks are those over the sides."""
    info, rows = t["info"], t["rows"]
    n = len(xyz)
    assert np.array_equal(t["side"], sides_of(np.asarray(xyz, F), add)), "owner"
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    assert int(info["side_class"].sum()) == n == info["n_points"]
    assert np.all(np.diff(rows["index"].astype(np.int64)) > 0)
    rs, rc = split_cell(rows)
    peak_pos = peak_neg = 0
    for k in range(info["n_sides"]):
        sel = np.flatnonzero(t["side"] == k)
        ri, rr = wc.check(xyz[sel], t["e"][sel], t["cell"][sel], raws[k], lab[sel], **kw)
        mine = rows[rs == k]
        log(f"side {k}: {len(sel)} points, {len(rr)} rows, classes {[ri[q] for q in wc.NAMES]}")
        assert [ri[q] for q in wc.NAMES] == [int(v) for v in info["side_class"][k]], k
        assert len(mine) == len(rr), k
        for q in ("x", "y", "z", "delta", "e"):
            assert np.array_equal(mine[q].view(np.uint32), rr[q].view(np.uint32)), (k, q)
        assert np.array_equal(rc[rs == k], rr["cell"]) and np.array_equal(mine["index"], sel[rr["index"]]), k
        peak_pos, peak_neg = max(peak_pos, ri["peak_pos"]), min(peak_neg, ri["peak_neg"])
    assert (info["peak_pos"], info["peak_neg"]) == (peak_pos, peak_neg)
    for q, name in enumerate(wc.NAMES):
        assert info[name] == int(info["side_class"][:, q].sum()), name
