"""numpy twin of a check's objects on a wall alignment (gm_wall_alignment_check_objects / _check_objects_rows,
csrc/k_wall_objects_joint.hip + gm_wall_alignment_objects.hip; include/gm_hip.h states the rule).

The rule is gm_wall_map_check_objects' on a virtual straight map of `total` stations: a row's cell holds
side << 24 | cell, side indexes the plan's side_element, and the row goes to the global station
G = base_e + cell // n_sectors of its side's element e.  So the twin only REWRITES the rows -- cell becomes
G * n_sectors + k, or -1 for a row whose side is >= n_sides or whose cell lies past its side's own cells -- and calls
wall_objects_np.objects on (total, n_sectors) around G_f = base_e + side_anchor[e] of the sensor's side.  Everything
else (dq == 0, the finite test, blocks, window, planes, components, records) is that twin's.

`variant` swaps in one deliberately WRONG reading of the rule (tests/test_wall_alignment_objects_np.py shows that each
changes the result): "per_element_blocks" anchors the blocks on each element's own station 0, "open_joint" does not join
blocks across a joint, "cells_of_side0" takes every side's cell limit from side 0.
"""
import numpy as np

import wall_check_np as kn
import wall_objects_np as on

MAX_SIDES = 4
INFO_KEYS = on.INFO_KEYS + ("element", "n_sides", "anchor_global", "total", "side_element", "side_first", "side_rows")


def bases(n_stations):
    """base_i of every element and the total."""
    b = np.concatenate([[0], np.cumsum(np.asarray(n_stations, np.int64))])
    return [int(x) for x in b[:-1]], int(b[-1])


def supported(n_stations, n_sectors, p):
    """The size rule: total <= 2^32 - 1 and ceil(total / bs) NK <= 2^32 - 1."""
    total = bases(n_stations)[1]
    NK = -(-int(n_sectors) // int(p["block_sectors"]))
    return total <= 2 ** 32 - 1 and -(-total // int(p["block_stations"])) * NK <= 2 ** 32 - 1


def plan_ok(n_elements, plan):
    se = [int(x) for x in plan["side_element"]]
    return (1 <= len(se) <= MAX_SIDES and all(0 <= e < n_elements for e in se) and
            all(se[i] == se[i - 1] + 1 for i in range(1, len(se))) and int(plan["element"]) in se)


def split(rows):
    c = np.asarray(rows["cell"]).view(np.uint32)
    return (c >> np.uint32(24)).astype(np.int64), (c & np.uint32(0xFFFFFF)).astype(np.int64)


def rewrite(rows, n_stations, n_sectors, plan, variant=None, first=None):
    """(rows with cell = G n_sectors + k or -1, side, station G, ok); first: the sides' first stations, if not the bases."""
    rows = np.asarray(rows, kn.POINT).reshape(-1)
    base, total = bases(n_stations)
    se = [int(x) for x in plan["side_element"]]
    ns = len(se)
    first = np.array([base[e] for e in se] if first is None else first, np.int64)
    cells = np.array([int(n_stations[e]) * n_sectors for e in se], np.int64)
    if variant == "cells_of_side0":
        cells[:] = cells[0]
    side, cell = split(rows)
    ok = side < ns
    sc = np.where(ok, side, 0)
    ok &= cell < cells[sc]
    G = first[sc] + cell // n_sectors
    out = rows.copy()
    out["cell"] = np.where(ok, G * n_sectors + cell % n_sectors, -1).astype(np.int32)
    return out, side, G, ok


def window(n_stations, n_sectors, plan, p):
    """The info's host half: what gm_wall_alignment_object_window fills."""
    base, total = bases(n_stations)
    se = [int(x) for x in plan["side_element"]]
    home = int(plan["element"]) - se[0]
    Gf = base[se[home]] + int(plan["side_anchor"][home])
    J0, nJ, NK, st0, nst = on.window(total, n_sectors, Gf, p)
    return dict(station0=st0, n_stations=nst, blocks_stations=nJ, blocks_sectors=NK, element=int(plan["element"]), n_sides=len(se),
                anchor_global=Gf, total=total, side_element=se, side_first=[base[e] for e in se])


def objects(rows, n_stations, n_sectors, plan, variant=None, **params):
    """(info dict, OBJECT array in (label, sign) order, object_of_row int32 [len(rows)]); station extents and the window
    are global.  plan: element, side_element, side_anchor of a gm_wall_alignment_add_info."""
    p = dict(on.DEFAULTS)
    p.update(params)
    n_stations = [int(x) for x in n_stations]
    assert supported(n_stations, n_sectors, p) and plan_ok(len(n_stations), plan)
    base, total = bases(n_stations)
    assert total * n_sectors < 2 ** 31, "the twin keeps the rewritten cell in the row's int32"
    w = window(n_stations, n_sectors, plan, p)
    if variant == "per_element_blocks":   # WRONG: every element padded to whole blocks, so each starts a block
        bs = int(p["block_stations"])
        pad = np.concatenate([[0], np.cumsum([-(-n // bs) * bs for n in n_stations])])
        g, side, G, ok = rewrite(rows, n_stations, n_sectors, plan, first=[int(pad[e]) for e in w["side_element"]])
        home = w["element"] - w["side_element"][0]
        info, obj, of_row = on.objects(g, int(pad[-1]), n_sectors, int(pad[w["element"]]) + int(plan["side_anchor"][home]), **p)
    elif variant == "open_joint":         # WRONG: each side labelled on its own, nothing joined across a joint
        g, side, G, ok = rewrite(rows, n_stations, n_sectors, plan)
        parts, of_row = [], np.full(len(g), -1, np.int32)
        info = None
        for s in range(len(w["side_element"])):
            h = g.copy()
            h["cell"] = np.where(side == s, h["cell"], -1)
            i_s, o_s, r_s = on.objects(h, total, n_sectors, w["anchor_global"], **p)
            parts.append((o_s, r_s))
            info = i_s if info is None else info
        obj = np.concatenate([o for o, _ in parts])
        order = np.lexsort((obj["sign"], obj["label"]))
        at, shift = np.zeros(len(obj) + 1, np.int64), 0   # (one spare entry: the index a row without an object is given)
        at[order] = np.arange(len(obj))
        for o_s, r_s in parts:
            of_row = np.where(r_s >= 0, at[np.where(r_s >= 0, r_s + shift, len(obj))], of_row).astype(np.int32)
            shift += len(o_s)
        obj = obj[order]
        info = dict(info, objects=len(obj))
    else:
        g, side, G, ok = rewrite(rows, n_stations, n_sectors, plan, variant)
        info, obj, of_row = on.objects(g, total, n_sectors, w["anchor_global"], **p)
    dq = kn.fix(g["delta"])
    finite = np.isfinite(g["x"]) & np.isfinite(g["y"]) & np.isfinite(g["z"]) & np.isfinite(g["e"])
    kept = ok & (dq != 0) & finite
    info = dict(info)
    info.update({k: w[k] for k in ("element", "n_sides", "anchor_global", "total", "side_element", "side_first")})
    info["side_rows"] = [int((kept & (side == s)).sum()) for s in range(len(w["side_element"]))]
    return info, obj, of_row


def metrics(p, n_stations, o):
    """gm_wall_alignment_object_metrics: p the template's gm_wall_params fields, o one OBJECT record on the global grid."""
    base, total = bases(n_stations)
    d = on.metrics(p, o)
    edges = np.array(base + [total], np.int64)
    for key, st in (("from", int(o["station_min"])), ("to", int(o["station_max"]))):
        e = int(np.searchsorted(edges, st, side="right")) - 1
        d["element_" + key], d["station_" + key] = e, st - base[e]
    return d


def with_sides(rows, side):
    """rows whose cell gains the side bits."""
    out = np.asarray(rows, kn.POINT).copy()
    out["cell"] = ((np.asarray(side, np.uint32) << np.uint32(24)) | out["cell"].view(np.uint32)).view(np.int32)
    return out
