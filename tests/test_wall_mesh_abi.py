"""gm_wall_map_mesh without a GPU: the symbols, the struct layouts from plain C99, the defaults, the refusals that need
no device, the host-only triangle rule (gm_wall_mesh_triangulate) against the twin tests/wall_mesh_np.py byte for byte,
the rule's invariants (indices, the two identities, a closed tube's edges, the winding) and the PLY file read back."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_cloud_np as cn  # noqa: E402
import wall_mesh_np as mn  # noqa: E402
import wall_np as wn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_wall_mesh_default_params", "gm_wall_map_mesh", "gm_wall_mesh_triangulate", "gm_wall_mesh_write_ply")
OUTWARD, NO_WRAP = _lib.GM_WALL_MESH_OUTWARD, _lib.GM_WALL_MESH_NO_WRAP
FLAGS = (0, OUTWARD, NO_WRAP, OUTWARD | NO_WRAP)


def test_symbols_are_exported_declared_and_prototyped():
    L = _lib.load()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(L, n) and n in L._gm_proto, n
    assert (OUTWARD, NO_WRAP) == (mn.OUTWARD, mn.NO_WRAP) == (1, 2)


def test_struct_layouts_from_c99_match_ctypes():
    fields = {
        "gm_wall_mesh_params": _lib.WallMeshParams,
        "gm_wall_mesh_triangle": _lib.WallMeshTriangle,
        "gm_wall_mesh_info": _lib.WallMeshInfo,
    }
    lines = ['printf("%u %u\\n", GM_WALL_MESH_OUTWARD, GM_WALL_MESH_NO_WRAP);']
    for cname, ct in sorted(fields.items()):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _t in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gm_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    want = [OUTWARD, NO_WRAP]
    for _, ct in sorted(fields.items()):
        want.append(C.sizeof(ct))
        want += [getattr(ct, f).offset for f, _t in ct._fields_]
    assert out == want
    assert C.sizeof(_lib.WallMeshTriangle) == 12 == 3 * api.WALL_MESH_TRIANGLE.itemsize


def test_defaults():
    L = _lib.load()
    p = _lib.WallMeshParams()
    L.gm_wall_mesh_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_lib.WallMeshParams) and (p.flags, p.max_step, p.reserved) == (0, 0.0, 0)
    c = api.WallMap.cloud_params()
    assert bytes(p.cloud) == bytes(c) and p.cloud.struct_size == C.sizeof(_lib.WallCloudParams)
    L.gm_wall_mesh_default_params(None)   # a NULL is ignored


def test_null_bad_struct_size_and_unknown_flags_are_refused_without_a_device():
    L = _lib.load()
    bad = _lib.GM_ERR_INVALID_ARG
    info, nv, nt = _lib.WallMeshInfo(), C.c_uint64(7), C.c_uint64(7)
    assert L.gm_wall_map_mesh(None, 0, 0, None, C.byref(info), None, 0, None, 0, C.byref(nv), C.byref(nt)) == bad
    v = np.zeros(2, api.WALL_CLOUD_POINT)
    v["block"] = (0, 3)
    vp = v.ctypes.data_as(C.POINTER(_lib.WallCloudPoint))
    tri = np.zeros((4, 3), np.uint32)
    tp = tri.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle))
    got = C.c_uint64(9)
    assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == _lib.GM_OK and got.value == 0
    assert info.struct_size == C.sizeof(_lib.WallMeshInfo) and (info.quads, info.quads_none, info.wrapped) == (1, 1, 0)
    assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 0, 0.0, None, tp, 4, C.byref(got)) == bad            # NULL info
    assert L.gm_wall_mesh_triangulate(2, 2, None, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad  # NULL rows with a count
    assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 0, 0.0, C.byref(info), None, 4, C.byref(got)) == bad  # NULL triangles with a capacity
    assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 4, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad    # an unknown flag
    for step in (-1.0, float("nan"), float("inf")):
        assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 0, step, C.byref(info), tp, 4, C.byref(got)) == bad
    assert L.gm_wall_mesh_triangulate(2, 1, vp, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad    # block 3 >= NJ NK
    assert L.gm_wall_mesh_triangulate(4097, 4096, vp, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad
    assert L.gm_wall_mesh_triangulate(1, 4097, vp, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad
    for blocks in ((3, 0), (2, 2)):                                                                      # not strictly ascending
        v["block"] = blocks
        assert L.gm_wall_mesh_triangulate(2, 2, vp, 2, 0, 0.0, C.byref(info), tp, 4, C.byref(got)) == bad
    with pytest.raises(_lib.GmError):
        api.wall_mesh_triangulate(2, 2, v)
    # a short capacity: GM_ERR_CAPACITY with the count and the info, nothing written
    full = np.zeros(9, api.WALL_CLOUD_POINT)
    full["block"] = np.arange(9)
    fp = full.ctypes.data_as(C.POINTER(_lib.WallCloudPoint))
    big = np.full((12, 3), 77, np.uint32)
    bp = big.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle))
    assert L.gm_wall_mesh_triangulate(3, 3, fp, 9, 0, 0.0, C.byref(info), bp, 11, C.byref(got)) == _lib.GM_ERR_CAPACITY
    assert got.value == 12 == info.triangles and info.quads_two == 6 and np.all(big == 77)
    assert L.gm_wall_mesh_triangulate(3, 3, fp, 9, 0, 0.0, C.byref(info), None, 0, None) == _lib.GM_OK   # the count query
    assert L.gm_wall_mesh_triangulate(3, 3, fp, 9, 0, 0.0, C.byref(info), bp, 12, C.byref(got)) == _lib.GM_OK and np.all(big < 9)


def verts(NJ, NK, alive, rng=None, mean=None):
    """A vertex list for the alive mask [NJ, NK]: block and mean filled, the rest zero."""
    blocks = np.flatnonzero(np.asarray(alive, bool).reshape(-1))
    v = np.zeros(len(blocks), api.WALL_CLOUD_POINT)
    v["block"] = blocks
    if mean is not None:
        v["mean"] = np.asarray(mean, np.float32).reshape(-1)[blocks]
    elif rng is not None:
        v["mean"] = rng.uniform(-0.1, 0.1, len(blocks)).astype(np.float32)
    return v


def both(NJ, NK, v, flags=0, max_step=0.0):
    """The library and the twin on one vertex list: byte equality, the invariants; returns (info, triangles)."""
    info, tri = api.wall_mesh_triangulate(NJ, NK, v, flags, max_step)
    wtri, winfo = mn.triangles(NJ, NK, v["block"], v["mean"], flags, max_step)
    assert tri.dtype == np.uint32 and tri.shape == wtri.shape and tri.tobytes() == wtri.tobytes()
    assert {k: info[k] for k in mn.INFO_KEYS} == winfo
    assert info["cloud"]["blocks_stations"] == NJ and info["cloud"]["blocks_sectors"] == NK and info["cloud"]["points"] == len(v)
    assert np.all(tri < max(len(v), 1)) and len(tri) == info["triangles"]
    assert info["quads"] == info["quads_two"] + info["quads_one"] + info["quads_none"] == mn.grid(NJ, NK, flags)[2]
    assert info["triangles"] == 2 * info["quads_two"] + info["quads_one"] - info["cut_by_step"]
    assert np.all(tri[:, 0] != tri[:, 1]) and np.all(tri[:, 1] != tri[:, 2]) and np.all(tri[:, 0] != tri[:, 2])
    return info, tri


@pytest.mark.parametrize("NK", (1, 2, 3, 4, 7, 64))
@pytest.mark.parametrize("NJ", (1, 2, 3, 9))
def test_triangulate_equals_the_twin(NJ, NK):
    rng = np.random.default_rng(100 * NJ + NK)
    for flags in FLAGS:
        wrapped = NK >= 3 and not flags & NO_WRAP
        info, tri = both(NJ, NK, verts(NJ, NK, np.ones((NJ, NK)), rng), flags)          # a full grid
        assert info["wrapped"] == int(wrapped) and info["quads"] == (NJ - 1) * (NK if wrapped else NK - 1)
        assert info["triangles"] == 2 * info["quads"] and info["quads_one"] == info["quads_none"] == 0
        for step in (0.0, 0.05):
            both(NJ, NK, verts(NJ, NK, rng.random((NJ, NK)) < 0.5, rng), flags, step)   # random holes
            both(NJ, NK, verts(NJ, NK, rng.random((NJ, NK)) < 0.9, rng), flags, step)
        board = (np.add.outer(np.arange(NJ), np.arange(NK)) % 2) == 0
        info, tri = both(NJ, NK, verts(NJ, NK, board), flags)                            # a checkerboard: no triangle at all
        assert len(tri) == 0 and info["quads_none"] == info["quads"]                     # (two alive corners everywhere, the wrapped column of an odd ring included)
        info, tri = both(NJ, NK, verts(NJ, NK, np.zeros((NJ, NK))), flags)               # no vertex at all
        assert len(tri) == 0 and info["quads_none"] == info["quads"]


def test_the_wrap_starts_at_three_sectors():
    for NK, flags, wrapped, quads in ((1, 0, 0, 0), (2, 0, 0, 1), (3, 0, 1, 3), (3, NO_WRAP, 0, 2), (4, 0, 1, 4)):
        info, tri = both(2, NK, verts(2, NK, np.ones((2, NK))), flags)
        assert (info["wrapped"], info["quads"], len(tri)) == (wrapped, quads, 2 * quads), NK
    info, tri = both(2, 3, verts(2, 3, np.ones((2, 3))))
    # the wrapped quad's corners: A = (0, 2), B = (1, 2), C = (1, 0), D = (0, 0)
    assert tri[-2:].tolist() == [[2, 5, 3], [2, 3, 0]]
    info, tri = both(1, 5, verts(1, 5, np.ones((1, 5))))                                 # NJ = 1: vertices, no triangles
    assert info["quads"] == 0 and len(tri) == 0


def test_each_single_dead_corner_keeps_the_winding():
    """A 2 x 2 grid (one quad, no wrap): blocks A = 0, D = 1, B = 2, C = 3."""
    full = np.ones((2, 2), bool)
    info, tri = both(2, 2, verts(2, 2, full))
    assert tri.tolist() == [[0, 2, 3], [0, 3, 1]]                                        # (A, B, C), (A, C, D)
    info, tri = both(2, 2, verts(2, 2, full), OUTWARD)
    assert tri.tolist() == [[0, 3, 2], [0, 1, 3]]
    # the alive corners in the cyclic order A, B, C, D, as blocks, then as indices into the three-vertex list
    for dead, blocks in ((0, (2, 3, 1)), (2, (0, 3, 1)), (3, (0, 2, 1)), (1, (0, 2, 3))):   # A, B, C, D dead in turn
        alive = full.copy().reshape(-1)
        alive[dead] = False
        v = verts(2, 2, alive.reshape(2, 2))
        index = {int(b): i for i, b in enumerate(v["block"])}
        for flags in (0, OUTWARD):
            info, tri = both(2, 2, v, flags)
            want = [index[b] for b in blocks]
            if flags:
                want = [want[0], want[2], want[1]]
            assert tri.tolist() == [want] and (info["quads_one"], info["quads_two"], info["quads_none"]) == (1, 0, 0)


def test_max_step_cuts_one_triangle_of_a_quad_and_both():
    full = np.ones((2, 2), bool)
    # blocks A = 0, D = 1, B = 2, C = 3
    one = verts(2, 2, full, mean=[0.0, 0.0, 0.5, 0.0])        # B stands out: (A, B, C) goes, (A, C, D) stays
    info, tri = both(2, 2, one, 0, 0.1)
    assert tri.tolist() == [[0, 3, 1]] and (info["cut_by_step"], info["quads_two"]) == (1, 1)
    other = verts(2, 2, full, mean=[0.0, 0.5, 0.0, 0.0])      # D stands out: (A, C, D) goes
    info, tri = both(2, 2, other, 0, 0.1)
    assert tri.tolist() == [[0, 2, 3]] and info["cut_by_step"] == 1
    two = verts(2, 2, full, mean=[0.5, 0.0, 0.0, 0.0])        # A is in both
    info, tri = both(2, 2, two, 0, 0.1)
    assert len(tri) == 0 and (info["cut_by_step"], info["quads_two"], info["triangles"]) == (2, 1, 0)
    info, tri = both(2, 2, two, 0, 0.0)                        # 0 switches the cut off
    assert len(tri) == 2 and info["cut_by_step"] == 0
    info, tri = both(2, 2, two, 0, 0.5)                        # > is strict
    assert len(tri) == 2
    # the comparison is fp32: the step is rounded to fp32 and the difference is one fp32 subtraction
    a, b = np.float32(0.1), np.float32(0.3)
    d = float(np.abs(a - b))
    edge = verts(2, 2, full, mean=[a, a, b, a])
    assert len(both(2, 2, edge, 0, d)[1]) == 2
    assert len(both(2, 2, edge, 0, float(np.nextafter(np.float32(d), np.float32(0))))[1]) == 1
    both(2, 2, edge, 0, 1e300)                                 # a step beyond fp32: nothing is cut
    both(2, 2, edge, 0, 1e-300)                                # a step that rounds to 0: every difference cuts


def test_a_closed_tube_uses_every_interior_edge_twice_in_opposite_directions():
    for NJ, NK in ((2, 3), (5, 8), (9, 33)):
        info, tri = both(NJ, NK, verts(NJ, NK, np.ones((NJ, NK))))
        assert len(tri) == 2 * (NJ - 1) * NK and info["wrapped"] == 1
        e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
        directed = e[:, 0] * (NJ * NK) + e[:, 1]
        assert len(np.unique(directed)) == len(directed)                       # no directed edge twice
        back = e[:, 1] * (NJ * NK) + e[:, 0]
        paired = np.isin(directed, back)
        # the unpaired edges are the two end rings, NK each, along the sectors
        lone = e[~paired]
        assert len(lone) == 2 * NK and np.all(lone // NK == (lone // NK)[:, :1]) and set((lone // NK)[:, 0]) == {0, NJ - 1}
        assert paired.sum() == 3 * len(tri) - 2 * NK


def _raw_constant(n, ns, e, count=4):
    raw = np.zeros((n, ns), wn.RAW_CELL)
    raw["count"] = count
    raw["sum"] = int(round(e * count * 2 ** 20))
    raw["min_key"] = ~wn.ordered(np.float32(e))
    raw["max_key"] = wn.ordered(np.float32(e))
    return raw


@pytest.mark.parametrize("design", (dict(), dict(point=(3.0, -1.0, 0.5), direction=(0.3, 0.2, 0.93), radius=3.1, station_length=0.3)))
def test_the_winding_faces_the_axis(design):
    """A constant-deviation map at g = 0: every vertex on the design cylinder.  (B - A) x (C - A) points toward the axis,
    and away from it with OUTWARD."""
    n, ns = 7, 24
    p = wn.params(n_stations=n, n_sectors=ns, **design)
    raw = _raw_constant(n, ns, 0.02)
    rng = np.random.default_rng(11)
    raw[rng.random((n, ns)) < 0.2] = np.zeros((), wn.RAW_CELL)   # some holes: single triangles, too
    f = wn.design_frame(p)
    for bs, bk in ((1, 1), (2, 5)):
        _, v = cn.cloud(raw, p, 0, None, cn.directions(ns, bk), exaggeration=0.0, block_stations=bs, block_sectors=bk)
        NJ, NK = -(-n // bs), -(-ns // bk)
        xyz = np.stack([v[k] for k in "xyz"], axis=1).astype(np.float64)
        for flags in (0, OUTWARD):
            info, tri = both(NJ, NK, v, flags)
            assert len(tri) > 10 and (bs > 1 or info["quads_one"] > 0)
            A, B, Cc = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
            normal = np.cross(B - A, Cc - A)
            q = (A + B + Cc) / 3.0 - np.asarray(f["o"])
            radial = q - np.outer(q @ np.asarray(f["a"]), np.asarray(f["a"]))
            s = np.einsum("ij,ij->i", normal, radial)
            assert np.all(s > 0) if flags else np.all(s < 0)


def _read_ply(path):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = next(int(ln.split()[2]) for ln in lines if ln.startswith("element vertex"))
    nf = next(int(ln.split()[2]) for ln in lines if ln.startswith("element face"))
    props = [ln.split() for ln in lines if ln.startswith("property")]
    assert props == [["property", "float", k] for k in ("x", "y", "z", "mean", "min", "max")] + [
        ["property", "list", "uchar", "uint", "vertex_indices"]]
    vt = np.dtype([(k, "<f4") for k in ("x", "y", "z", "mean", "min", "max")])
    ft = np.dtype([("n", "u1"), ("v", "<u4", (3,))])
    assert len(body) == nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(body, vt, nv)
    f = np.frombuffer(body, ft, nf, offset=nv * vt.itemsize)
    return v, f


def test_ply_round_trip():
    n, ns = 9, 16
    p = wn.params(n_stations=n, n_sectors=ns)
    rng = np.random.default_rng(3)
    raw = _raw_constant(n, ns, -0.03)
    raw[rng.random((n, ns)) < 0.3] = np.zeros((), wn.RAW_CELL)
    _, v = cn.cloud(raw, p, 0, None, cn.directions(ns, 1))
    _, tri = api.wall_mesh_triangulate(n, ns, v)
    assert len(tri) > 20
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "wall.ply")
        api.wall_mesh_write_ply(path, v, tri)
        pv, pf = _read_ply(path)
        assert len(pv) == len(v) and all(pv[k].tobytes() == v[k].tobytes() for k in pv.dtype.names)
        assert np.all(pf["n"] == 3) and pf["v"].tobytes() == tri.tobytes()
        api.wall_mesh_write_ply(path, v[:0], tri[:0])                       # an empty mesh is a header
        pv, pf = _read_ply(path)
        assert len(pv) == 0 and len(pf) == 0
        with pytest.raises(_lib.GmError) as e:
            api.wall_mesh_write_ply(os.path.join(d, "no", "such", "dir.ply"), v, tri)
        assert e.value.status == _lib.GM_ERR_DEVICE
        with pytest.raises(_lib.GmError) as e:
            api.wall_mesh_write_ply(path, v[:3], tri)                       # an index beyond the vertices
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
    L = _lib.load()
    assert L.gm_wall_mesh_write_ply(None, None, 0, None, 0) == _lib.GM_ERR_INVALID_ARG


def test_twin_mesh_builds_on_the_cloud_twin():
    n, ns = 12, 10
    p = wn.params(n_stations=n, n_sectors=ns)
    raw = _raw_constant(n, ns, 0.01)
    raw[::3, ::2] = np.zeros((), wn.RAW_CELL)
    info, v, tri = mn.mesh(raw, p, 2, 9, cn.directions(ns, 3), block_stations=2, block_sectors=3, flags=NO_WRAP, max_step=0.5)
    winfo, wv = cn.cloud(raw, p, 2, 9, cn.directions(ns, 3), block_stations=2, block_sectors=3)
    assert info["cloud"] == winfo and v.tobytes() == wv.tobytes() and info["wrapped"] == 0
    assert info["quads"] == (5 - 1) * (4 - 1) and len(tri) == info["triangles"]
