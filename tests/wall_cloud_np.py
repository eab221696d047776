"""numpy twin of gm_wall_map_cloud (csrc/k_wall_cloud.hip + gm_wall.hip; include/gm_hip.h states the rule).

merge_blocks() is the integer merge of a window's raw cells into blocks; cloud() classifies the blocks, converts the
survivors as gm_wall_map_read converts a cell and places them in fp64, one rounding per operation in the header's
order, one astype(float32) at the end.  The direction table is an argument (gm_wall_cloud_directions' table, or
directions() below from numpy's cos / sin), so positions compare byte for byte without depending on a second libm.
"""
import numpy as np

import wall_np as wn

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("mean", "<f4"), ("min", "<f4"), ("max", "<f4"),
                  ("block", "<u4"), ("cells", "<u4"), ("count", "<u8")])
MERGED = np.dtype([("sum", "<i8"), ("count", "<u8"), ("min_key", "<u4"), ("max_key", "<u4"), ("cells", "<u4")])
DEFAULTS = dict(block_stations=1, block_sectors=1, min_count=1, exaggeration=1.0, anchor=(0.0, 0.0, 0.0))
INFO_KEYS = ("station0", "n_stations", "n_sectors", "blocks_stations", "blocks_sectors", "blocks", "points",
             "below_min_count", "empty")


def grid(n, ns, bs, bk):
    """(bs, bk clamped to the window and the ring, NJ, NK)."""
    bs, bk = min(int(bs), max(n, 1)), min(int(bk), ns)
    return bs, bk, -(-n // bs), -(-ns // bk)


def merge_blocks(win, bs, bk):
    """MERGED [NJ, NK] of the raw cells win [n, n_sectors]: ragged last blocks, nothing wraps.  An all-zero cell is the
    identity of wall_np.merge_raw, so the window is padded with such cells to whole blocks and folded with it."""
    n, ns = win.shape
    bs, bk, NJ, NK = grid(n, ns, bs, bk)
    pad = np.zeros((NJ * bs, NK * bk), wn.RAW_CELL)
    pad[:n, :ns] = win
    tiles = pad.reshape(NJ, bs, NK, bk)
    # (the merge is associative and commutative: station rows first, then sector columns.  merge_raw's u32 count may
    # wrap; the u64 count is summed below)
    rows = pad.reshape(NJ, bs, NK * bk)
    acc = np.zeros((NJ, NK * bk), wn.RAW_CELL)
    for i in range(bs):
        acc = wn.merge_raw(acc, rows[:, i])
    cols = acc.reshape(NJ, NK, bk)
    acc = np.zeros((NJ, NK), wn.RAW_CELL)
    for k in range(bk):
        acc = wn.merge_raw(acc, cols[:, :, k])
    out = np.zeros((NJ, NK), MERGED)
    out["sum"], out["min_key"], out["max_key"] = acc["sum"], acc["min_key"], acc["max_key"]
    out["count"] = tiles["count"].astype(np.uint64).sum(axis=(1, 3), dtype=np.uint64)
    out["cells"] = (tiles["count"] > 0).sum(axis=(1, 3))
    return out


def directions(ns, bk):
    """The header's table from numpy's cos / sin (the library's comes from the host's libm)."""
    bk = min(int(bk), ns)
    K = np.arange(-(-ns // bk), dtype=np.int64)
    nk = np.minimum(bk, ns - K * bk)
    phi = np.float64(2.0 * np.pi) * ((2 * K * bk + nk).astype(np.float64) / np.float64(2 * ns))
    return np.stack([np.cos(phi), np.sin(phi)], axis=1)


def cloud(raw, p, station0=0, n=None, directions=None, frame=None, **params):
    """(info dict, POINT records) of stations [station0, station0 + n) of the whole map's raw cells raw [n_stations,
    n_sectors] under the gm_wall_params dict p.  directions: [NK, 2] float64 (cos, sin).  frame: the design frame
    (o, a, u, v, R in fp64) the map REPORTED (gm_wall_map_info), as wall_np.points takes the reported add frame: the
    library derives it with its own dot products, whose last bit a BLAS need not share; None: wall_np.design_frame(p),
    which is the same bits for an axis-aligned design."""
    prm = dict(DEFAULTS)
    prm.update(params)
    nst, ns = raw.shape
    n = nst - station0 if n is None else n
    if station0 + n > nst:
        raise ValueError("the window leaves the map")
    bs, bk, NJ, NK = grid(n, ns, prm["block_stations"], prm["block_sectors"])
    info = dict(station0=station0, n_stations=n, n_sectors=ns, blocks_stations=NJ, blocks_sectors=NK, blocks=NJ * NK,
                points=0, below_min_count=0, empty=0)
    if n == 0:
        return info, np.zeros(0, POINT)
    m = merge_blocks(raw[station0:station0 + n], bs, bk).reshape(-1)
    empty = m["count"] == 0
    below = ~empty & (m["count"] < np.uint64(prm["min_count"]))
    keep = ~empty & ~below
    info.update(points=int(keep.sum()), below_min_count=int(below.sum()), empty=int(empty.sum()))
    block = np.flatnonzero(keep)
    m = m[keep]
    out = np.zeros(len(block), POINT)
    out["block"], out["cells"], out["count"] = block, m["cells"], m["count"]
    mean = (m["sum"].astype(np.float64) * np.float64(2.0 ** -20)) / m["count"].astype(np.float64)
    as_cell = np.zeros(len(block), wn.RAW_CELL)
    as_cell["count"], as_cell["min_key"], as_cell["max_key"] = 1, m["min_key"], m["max_key"]
    _, _, out["min"], out["max"] = wn.records_from(as_cell)
    out["mean"] = mean.astype(np.float32)
    # position: fp64, the header's order
    d = wn.design_frame(p) if frame is None else frame
    J, K = block // NK, block % NK
    j0 = station0 + J * bs
    nsj = np.minimum(bs, station0 + n - j0)
    h = (2 * j0 + nsj).astype(np.float64) * np.float64(0.5)
    tc = np.float64(p["t_min"]) + h * np.float64(p["station_length"])
    rho = np.float64(d["R"]) + np.float64(prm["exaggeration"]) * mean
    tab = np.asarray(directions, np.float64)
    if tab.shape != (NK, 2):
        raise ValueError("the direction table is not [NK, 2]")
    c, s = tab[K, 0], tab[K, 1]
    anchor = np.asarray(prm["anchor"], np.float64)
    for i, f in enumerate("xyz"):
        w = c * np.float64(d["u"][i]) + s * np.float64(d["v"][i])
        q = ((np.float64(d["o"][i]) - anchor[i]) + tc * np.float64(d["a"][i])) + rho * w
        out[f] = q.astype(np.float32)
    return info, out
