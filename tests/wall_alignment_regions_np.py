"""numpy twin of gm_wall_alignment_regions (csrc/gm_wall_alignment_regions.hip + k_wall_regions_joint.hip; include/gm_hip.h
states the rule): gm_wall_map_regions' rule on the virtual map of `total` stations whose raw cells are the element maps'
concatenated in element order.  No labelling code of its own: regions_np.regions on the concatenated array IS the rule;
this module adds the size rule, the window's pieces and the metrics on the global station grid (the peak's design
position through the library's point rule, as wall_alignment_np.axes takes its sections)."""
import numpy as np

import regions_np as rn

MAX_CELLS = 1 << 26
INFO_KEYS = ("station0", "n_stations", "n_sectors", "threshold_q", "flagged_pos", "flagged_neg", "unusable", "empty", "components",
             "regions", "cell_area", "total", "n_pieces", "element_from", "element_to", "station_from", "station_to")
COUNTS = ("threshold_q", "flagged_pos", "flagged_neg", "unusable", "empty", "components", "regions")
TWO_PI = 6.283185307179586476925286766559


def bases(n_stations):
    return [0] + [int(x) for x in np.cumsum(np.asarray(n_stations, np.int64))]


def locate(n_stations, G):
    """(element, station inside it) of global station G."""
    b = bases(n_stations)
    e = int(np.searchsorted(b, G, side="right")) - 1
    return e, G - b[e]


def window_status(n_stations, n_sectors, station0, n):
    """"ok", "invalid" (the window leaves [0, total]) or "unsupported" (the size rule), in the call's order."""
    total = bases(n_stations)[-1]
    if total * n_sectors > 2 ** 31 - 1:
        return "unsupported"
    if station0 + n > total:
        return "invalid"
    return "unsupported" if n * n_sectors > MAX_CELLS else "ok"


def window(p, n_stations, station0, n):
    """The window fields of the info for an accepted window; the counts 0."""
    ns = int(p["n_sectors"])
    d = dict.fromkeys(INFO_KEYS, 0)
    d.update(station0=station0, n_stations=n, n_sectors=ns, cell_area=rn.cell_area(p), total=bases(n_stations)[-1])
    if n:
        (e0, j0), (e1, j1) = locate(n_stations, station0), locate(n_stations, station0 + n - 1)
        d.update(n_pieces=e1 - e0 + 1, element_from=e0, element_to=e1, station_from=j0, station_to=j1)
    return d


def concat(raws):
    return np.concatenate(list(raws), axis=0)


def regions(p, raws, base_raws=None, station0=0, n=None, **params):
    """The call on the element maps' raw cells (a list of (n_stations_e, n_sectors) arrays; base_raws: the baseline's):
    (info dict with INFO_KEYS, REGION array ascending by label, labels (n, n_sectors) int32)."""
    n_stations = [len(r) for r in raws]
    n = bases(n_stations)[-1] - station0 if n is None else n
    info, reg, labels = rn.regions(concat(raws), None if base_raws is None else concat(base_raws), station0, n, **params)
    out = window(p, n_stations, station0, n)
    out.update({k: info[k] for k in COUNTS})
    return out, reg, labels


def metrics(A, p, n_stations, r):
    """gm_wall_alignment_region_metrics: A a WallAlignmentRule (its point rule), p a dict of the template's fields, r one
    REGION record on the global grid."""
    ns = int(p["n_sectors"])
    d = rn.metrics(p, r)
    (d["element_from"], d["station_from"]) = locate(n_stations, int(r["station_min"]))
    (d["element_to"], d["station_to"]) = locate(n_stations, int(r["station_max"]))
    G, k = divmod(int(r["peak_cell"]), ns)
    (d["peak_element"], d["peak_station"]), d["peak_sector"] = locate(n_stations, G), k
    d["peak_point"] = A.point(*peak_arguments(p, r))[0]
    return d


def peak_arguments(p, r):
    """(chainage, angle, rho) of the peak cell's centre, every operation rounded once."""
    ns = int(p["n_sectors"])
    G, k = divmod(int(r["peak_cell"]), ns)
    chainage = float(p["t_min"]) + (float(G) + 0.5) * float(p["station_length"])
    angle = TWO_PI * (float(k) + 0.5) / float(ns)
    rho = float(p["radius"]) + float(int(r["peak"])) * 2.0 ** -20
    return chainage, angle, rho
