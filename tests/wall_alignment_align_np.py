"""numpy twin of the align on a wall alignment (gm_wall_alignment_align_*, csrc/k_wall_align_joint.hip +
gm_wall_alignment_align.hip; include/gm_hip.h states the rule), written from the header.

It composes what the other twins already hold: the owner by the add's fp32 rule (wall_alignment_np.owner32), the owner's
chain on its per-add block (wall_alignment_locate_np.side_chain on the blocks of the plan's start, which ARE the sides'
per-add frames) with the PATCH as its range (anchor = row0 of the side, 2P rows), and the integer rule of the map's align
(wall_align_np.patch_from, values, table, select) on the map image, which is the element raws concatenated in global
station order.  plan() is the header's integers (G_f, row0 per side, the pieces, the one-straight-side rule), pose() the
header's pose from the library's design frames.

FAULTS names three deliberate errors that tests/test_wall_alignment_align_np.py must see in the table or in the pose on the
joint cases: every side binned with the SENSOR side's row0 (the neighbour's wall with the wrong chain), the image rows of
every element but the sensor's unusable (an element map's own align), and the pose moved along the tangent at s instead of
along the alignment.
"""
import numpy as np

import wall_align_np as an
import wall_alignment_locate_np as aln
import wall_alignment_np as al_np
import wall_np as wn

F = np.float32
FAULTS = ("row0_of_sensor_side", "neighbour_rows_none", "pose_on_tangent")
MAX_PIECES = 8
CLASSES = an.CLASSES
PLANE, BEYOND, OUTSIDE, BINNED = range(4)


def bases(n_stations):
    """base_i per element and the total: [0, n_0, n_0 + n_1, ...]."""
    return [0] + [int(x) for x in np.cumsum([int(n) for n in n_stations])]


def plan(add, n_stations, kinds, ap):
    """The header's integers from the add's plan dict: dict(anchor_global, total, home, row0 [n_sides], pieces
    [(element, first_row, n_stations)], own); None for more than MAX_PIECES pieces."""
    P, A = ap["half_patch_stations"], ap["max_station_shift"]
    base = bases(n_stations)
    home = add["element"] - add["side_element"][0]
    gf = base[add["element"]] + int(add["side_anchor"][home])
    row0 = [base[i] + int(a) - gf + P for i, a in zip(add["side_element"], add["side_anchor"])]
    g0, g1 = gf - P - A, gf + P + A
    pieces = [(i, base[i], int(n_stations[i])) for i in range(len(n_stations)) if base[i] < g1 and base[i + 1] > g0]
    if len(pieces) > MAX_PIECES:
        return None
    own = add["n_sides"] == 1 and kinds[add["element"]] == aln.STRAIGHT and all(p[0] == add["element"] for p in pieces)
    return dict(anchor_global=gf, total=base[-1], home=home, row0=np.array(row0, np.int64), pieces=pieces, own=int(own))


def chains(xyz, labels, lplan, row0, grid, ap, fault=None):
    """Per point, on its owner's chain alone under the align's gate: dict(side, e float32 (NaN for plane points), cell
    (jr n_sectors + k of a binned point, else -1), cls (index into CLASSES))."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    add = lplan["add"]
    ns, n = add["n_sides"], len(xyz)
    P = ap["half_patch_stations"]
    lab = np.zeros(n, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    side = al_np.owner32(xyz, dict(n_sides=ns, side_element=list(range(ns)), joint_o=add["joint_o"], joint_a=add["joint_a"])).astype(np.int64)
    state = dict(o=lplan["c"], a=lplan["d"], u=lplan["u"], v=lplan["v"])
    blk = aln.blocks(lplan, state)
    pf = aln.plan_fields(lplan)
    home = add["element"] - add["side_element"][0]
    e, cell, cls = np.full(n, np.nan, F), np.full(n, -1, np.int64), np.full(n, BEYOND, np.int8)
    gate = F(ap["gate"])
    for k in range(ns):
        sel = np.flatnonzero(side == k)
        r0 = int(row0[home] if fault == "row0_of_sensor_side" else row0[k])
        r = aln.side_chain(xyz[sel], pf["side_kind"][k], blk["side"][k], pf["side_axis"][k], grid, r0, 2 * P)
        ek = np.asarray(r["e"], F)
        with np.errstate(invalid="ignore"):
            inside = r["guard"] & (np.abs(ek) <= gate)
        e[sel] = ek
        cls[sel] = np.where(inside, np.where(r["cell"] >= 0, BINNED, OUTSIDE), BEYOND)
        cell[sel] = np.where(inside, r["cell"], -1)
    plane = lab == 1
    e[plane], cell[plane], cls[plane] = np.nan, -1, PLANE
    return dict(side=side, e=e, cell=cell, cls=cls)


def concat_raw(raws, n_stations, n_sectors, sensor_element=None, fault=None):
    """The alignment's raw cells in global station order, (total, n_sectors) RAW_CELL: element i's rows at base_i.  raws:
    per element a RAW_CELL array or None (never surveyed)."""
    out = []
    for i, nst in enumerate(n_stations):
        r = raws[i] if raws[i] is not None else np.zeros(int(nst) * n_sectors, wn.RAW_CELL)
        r = np.asarray(r).reshape(int(nst), n_sectors)
        if fault == "neighbour_rows_none" and i != sensor_element:
            r = np.zeros_like(r)
        out.append(r)
    return np.concatenate(out, axis=0)


def table(e, cell, raws, n_stations, pl, n_sectors, ap, sensor_element=None, fault=None):
    """(SCORE table (2A + 1, 2B + 1), patch sum, patch count) of per-point (e, patch cell) pairs against the element raws."""
    P = ap["half_patch_stations"]
    psum, pcnt = an.patch_from(e, cell, 2 * P * n_sectors)
    cat = concat_raw(raws, n_stations, n_sectors, sensor_element, fault)
    return an.table(psum, pcnt, cat, pl["anchor_global"], n_sectors, ap), psum, pcnt


def frame_of(rule, x):
    """F(x) = [a u v] (columns) and P(x) of the header, from the library's point rule (wall_alignment_np.axes)."""
    P, a, u, v = al_np.axes(rule, x)
    return np.stack([a, u, v], axis=1), P


def pose(rule, pose_in, s, shift_m, roll, fault=None):
    """The header's pose: M = F(s') Q F(s)^T, Rm' = M Rm, tr' = P(s') + M (tr - P(s)); (3, 4)."""
    m = np.asarray(pose_in, np.float64)[:3]
    F1, P1 = frame_of(rule, s)
    if fault == "pose_on_tangent":   # the straight map's rule on the section at s: the curve ahead is not followed
        return an.compose(dict(a=F1[:, 0], o=P1), m, shift_m, roll)
    F2, P2 = frame_of(rule, s + shift_m)
    c, sn = np.cos(roll), np.sin(roll)
    Q = np.array([[1.0, 0.0, 0.0], [0.0, c, -sn], [0.0, sn, c]])
    M = F2 @ Q @ F1.T
    return np.concatenate([M @ m[:, :3], (P2 + M @ (m[:, 3] - P1)).reshape(3, 1)], axis=1)


def select(tab, rule, pose_in, add, pl, grid, ap, fault=None):
    """The host rule on a SCORE table: wall_align_np.select's dict with the alignment's anchor_station (j_f of the sensor's
    side) and pose."""
    dummy = wn.params(n_stations=1, n_sectors=int(grid["n_sectors"]), station_length=float(grid["station_length"]),
                      radius=float(grid["radius"]))
    out = an.select(tab, dummy, np.eye(4)[:3], ap)
    out["anchor_station"] = int(add["side_anchor"][pl["home"]])
    if not out["status"] & an.FAILED_MASK:
        out["pose"] = pose(rule, pose_in, float(add["chainage"]), out["shift_m"], out["roll"], fault)
    return out


def align(xyz, labels, rule, pose_in, bound, raws, grid, ap, fault=None):
    """The whole align: (select() dict with the class counts, side_class, patch_cells_usable, n_sides, the twin's plan
    under "twin_plan" and the per-point dict under "points"; table).  raws: per ELEMENT of the alignment."""
    lplan = rule.locate_plan(pose_in, bound)
    add = lplan["add"]
    ne = rule.n_elements
    eps = [rule.element_params(i) for i in range(ne)]
    nst = [int(e[0].n_stations) for e in eps]
    kinds = [aln.CLOTHOID if e[2] is not None else (aln.ARC if e[1] is not None else aln.STRAIGHT) for e in eps]
    pl = plan(add, nst, kinds, ap)
    assert pl is not None, "more than MAX_PIECES pieces"
    pts = chains(xyz, labels, lplan, pl["row0"], grid, ap, fault)
    nsec = int(grid["n_sectors"])
    e32 = np.where(np.isnan(pts["e"]), F(0.0), pts["e"]).astype(F)
    tab, psum, pcnt = table(e32, pts["cell"], raws, nst, pl, nsec, ap, add["element"], fault)
    out = select(tab, rule, pose_in, add, pl, grid, ap, fault)
    out.update({q: int((pts["cls"] == i).sum()) for i, q in enumerate(CLASSES)})
    out["side_class"] = np.array([[int(((pts["side"] == k) & (pts["cls"] == q)).sum()) for q in range(4)] for k in range(add["n_sides"])],
                                 np.uint32)
    out.update(patch_cells_usable=int((pcnt >= ap["min_frame_count"]).sum()), n_sides=add["n_sides"], n_points=len(pts["e"]),
               twin_plan=pl, points=pts, add=add)
    return out, tab
