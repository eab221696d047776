"""numpy twin of gm_wall_map_mesh (csrc/k_wall_mesh.hip + gm_wall.hip; include/gm_hip.h states the rule).

triangles() is the triangle rule on the alive blocks of an NJ x NK block grid and the vertices' fp32 means; mesh() builds
the vertices with wall_cloud_np.cloud and triangulates them.  Everything is whole-array numpy: the quads' four corner
indices, the one corner each slot leaves out, the fp32 step cut, and a boolean selection in slot order.
"""
import numpy as np

import wall_cloud_np as cn

OUTWARD, NO_WRAP = 1, 2
INFO_KEYS = ("wrapped", "quads", "quads_two", "quads_one", "quads_none", "cut_by_step", "triangles")
# the cyclic order A, B, C, D with corner `drop` left out
_ORDER = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], np.int64)


def grid(NJ, NK, flags=0):
    """(wrapped, NKq, quads)."""
    wrapped = int(NK >= 3 and not (flags & NO_WRAP))
    NKq = NK if wrapped else max(NK - 1, 0)
    return wrapped, NKq, max(NJ - 1, 0) * NKq


def triangles(NJ, NK, alive_blocks, mean, flags=0, max_step=0.0):
    """(uint32 [nt, 3], info dict) of the vertex list whose i-th vertex is block alive_blocks[i] (strictly ascending,
    < NJ NK) with the fp32 mean mean[i]."""
    alive_blocks = np.asarray(alive_blocks, np.int64).reshape(-1)
    mean = np.asarray(mean, np.float32).reshape(-1)
    if len(alive_blocks) != len(mean) or np.any(np.diff(alive_blocks) <= 0) or np.any(alive_blocks >= NJ * NK):
        raise ValueError("blocks must ascend strictly below NJ NK, one mean each")
    wrapped, NKq, quads = grid(NJ, NK, flags)
    info = dict(wrapped=wrapped, quads=quads, quads_two=0, quads_one=0, quads_none=0, cut_by_step=0, triangles=0)
    if quads == 0:
        return np.zeros((0, 3), np.uint32), info
    rank = np.full(NJ * NK, -1, np.int64)
    rank[alive_blocks] = np.arange(len(alive_blocks))
    R = rank.reshape(NJ, NK)
    K = np.arange(NKq)
    K1 = (K + 1) % NK
    corners = np.stack([R[:-1][:, K], R[1:][:, K], R[1:][:, K1], R[:-1][:, K1]], axis=-1).reshape(quads, 4)   # A, B, C, D
    live = corners >= 0
    na = live.sum(axis=1)
    info.update(quads_two=int((na == 4).sum()), quads_one=int((na == 3).sum()), quads_none=int((na < 3).sum()))
    dead = np.argmin(live, axis=1)                      # (the one dead corner where na == 3)
    drop = np.stack([np.where(na == 4, 3, dead), np.ones(quads, np.int64)], axis=1)     # slot 2Q: (A, B, C); 2Q + 1: (A, C, D)
    slots = np.take_along_axis(corners[:, None, :], _ORDER[drop], axis=2)               # [quads, 2, 3]
    keep = np.stack([na >= 3, na == 4], axis=1)
    if max_step > 0.0:
        with np.errstate(over="ignore"):
            step = np.float32(max_step)
        m = mean[np.maximum(slots, 0)] if len(mean) else np.zeros(slots.shape, np.float32)
        d = np.abs(np.stack([m[..., 0] - m[..., 1], m[..., 1] - m[..., 2], m[..., 0] - m[..., 2]], axis=-1))   # fp32 - fp32
        assert d.dtype == np.float32
        cut = keep & np.any(d > step, axis=-1)
        info["cut_by_step"] = int(cut.sum())
        keep &= ~cut
    tri = slots[keep]                                   # C order: ascending by slot
    if flags & OUTWARD:
        tri = tri[:, [0, 2, 1]]
    info["triangles"] = len(tri)
    return np.ascontiguousarray(tri, dtype=np.uint32), info


def mesh(raw, p, station0=0, n=None, directions=None, frame=None, flags=0, max_step=0.0, **cloud_params):
    """(info dict with the cloud's under "cloud", POINT vertices, uint32 [nt, 3]) as WallMap.mesh returns them."""
    cinfo, v = cn.cloud(raw, p, station0, n, directions, frame=frame, **cloud_params)
    tri, info = triangles(cinfo["blocks_stations"], cinfo["blocks_sectors"], v["block"], v["mean"], flags, max_step)
    info["cloud"] = cinfo
    return info, v, tri
