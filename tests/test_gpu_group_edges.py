"""The sharded frame (gm_group_process_frame, csrc/gm_group.hip) at slab edges: which rows a rank owns, whether every
owned row sees all of its neighbours through the halo, and how the host merges the ranks' outputs.

The references are the numpy twin of the slab cut (tests/group_cut_np.py), count_exact on the integer tie clouds of
tests/normals_np.py (no floating point), the C oracle, and the single-device frame of the same cloud on a plain
GeometricMapping with the same bound, radius, leaf and flags.  tests/test_group_edges_np.py asserts on every CPU run
that the cases straddle their edges by the ten thousand pairs, that halo-only and mixed tiles occur, and that the checks
used here fail on a narrower halo, a closed upper edge, an edge one float low and a skip that drops mixed tiles.

Per case (assertions 1 to 5 of check_group / test_tie_cloud_over_ranks):
  1  every rank's neighbour counts, in the order of the rows it was sent: the exact count on owned rows, 0 or in
     [1, exact] on halo rows;
  2  the merged cloud is the single-device one, the frame's counters are equal, every rank's valid rows are the rows it
     owns among those the single-device frame kept;
  3  the ranks' normals merged by input row: the single-device NaN pattern, and the f64 oracle's by the rule of
     tests/test_gpu_normals_edges.py (0.98 quantile of the angle below max(1e-5, the f32-faithful oracle's own));
  4  voxel centroids and the 1-NN bit-equal to the single-device frame's, the voxel normals within test_group.py's 1e-5;
  5  the frame again gives the same bytes, and a shorter frame on the same group leaves nothing of the larger one.
Groups are loopback groups on device 0.

Observed on an MI355X (every case passes; printed again by each run with -s).  Rows owned / rows sent per rank, halo
rows that reported count 0 per rank, the worst angle to the f64 oracle over the well-supported rows beside the 0.98
quantile of the f32-faithful oracle's own; straddling pairs and ties are in group_cut_np.TABLE:
  tie_q7  leaf 0.125 R 4  edges 3.625 4.0 4.625   1871 1138 1855 1136 / 2652 2653 3429 1919   0: 515 972 1173 640   0 rad (1.09e-3)
  tie_q7  leaf 0.25  R 3  edges 3.75 4.5          2230 2242 1528 / 3030 3818 2292             0: 570 1037 448       0 rad (1.09e-3)
  tie_q7  leaf 0.5   R 2  edge  4.0               3009 2991 / 3733 3770                       0: 441 520            0 rad (1.09e-3)
  tie_q7  leaf 0.5   R 4  edges 4.0 4.0 5.0       3009 0 2991 0 / 3733 1503 3770 741          0: 441 1503 520 741   0 rad (1.09e-3)
  tie_q14 leaf 0.125 R 4  edges 3.625 4.125 4.5   1935 1521 1172 1514 / 2695 3111 2820 2327   0: 593 1263 1325 704  1.3e-7 rad (1.40e-3)
  tie_q14 leaf 0.25  R 2  edge  4.25              3824 2318 / 4630 3081                       0: 714 586            2.0e-7 rad (1.40e-3)
  planes (20 000-point tunnel + planted rows), leaf 0.5 / 0.3, R 2 / 4: worst angle 1.5e-7 .. 2.1e-7 rad (1.6e-4)
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binning_np as bn  # noqa: E402
import group_cut_np as gc  # noqa: E402
import normals_np as nn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 5.0
RES_KEYS = ("n_in", "n_cropped", "n_valid", "n_voxels")


def ang(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=-1) / np.maximum(np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1), 1e-300)
    return np.arcsin(np.clip(s, 0, 1))


def config(radius, leaf):
    from geometric_mapping_amd import _lib
    return dict(boxFilterBound=BOUND, neighborRadius=radius, voxelGridLeafSize=leaf,
                flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_KEEP_COUNTS | _lib.GM_CFG_NEAREST)


def single_outputs(c, xyz):
    res = c.process_frame(xyz)
    cloud, rows = c.cropped_cloud()
    cen, cnt = c.voxel_centroids()
    return dict(res=res, cloud=cloud, rows=rows, counts=c.neighbor_counts(), normals=c.normals(), cen=cen, cnt=cnt,
                vnrm=c.voxel_normals(), vnn=c.voxel_nearest())


def single_frame(gm, xyz, radius, leaf):
    with gm.GeometricMapping(**config(radius, leaf)) as c:
        return single_outputs(c, xyz)


def group_outputs(g, xyz):
    res = g.process_frame(xyz)
    cloud, rows = g.cropped_cloud()
    cen, cnt = g.voxel_centroids()
    vnrm, vnn = g.voxel_normals(), g.voxel_nearest()
    edges, on_lattice = g.edges()
    ranks = [dict(counts=g.rank_fetch(r, 0, "neighbor_counts"), normals=g.rank_fetch(r, 0, "normals"),
                  xyzw=g.rank_fetch(r, 0, "cropped_xyz")) for r in range(len(g))]
    return dict(res=res, cloud=cloud, rows=rows, cen=cen, cnt=cnt, vnrm=vnrm, vnn=vnn, edges=edges, on_lattice=on_lattice, ranks=ranks)


def same_bytes(a, b, path=""):
    """Two outputs of group_outputs / single_outputs, byte for byte (NaN equal to NaN; the timings aside)."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            if k not in ("stage_ms", "normals_kernel_ms"):
                same_bytes(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_bytes(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, path


@functools.lru_cache(maxsize=None)
def oracle(key):
    """(f64 normals, counts, f32-faithful normals, kept rows) of a registered cloud, once."""
    from oracle import oracle_c as oc
    oc.build()
    xyz, radius = CLOUDS[key]
    n64, cnt = oc.normals(xyz, radius, oc.F64)
    n32, _ = oc.normals(xyz, radius, oc.F32_FAITHFUL)
    return n64, cnt, n32, oc.finite_normals(n64)


CLOUDS = {}          # key -> (xyz, radius) for oracle()


def check_group(xyz, radius, leaf, R, G, S, exact=None, oracle_key=None, tag=""):
    """Assertions 1 to 4 on the outputs G of a group of R ranks against the single-device outputs S of the same cloud.
    Returns what the summary quotes."""
    c = gc.cut(xyz, BOUND, leaf, radius, R)
    # the twin is held to the library
    assert G["on_lattice"] and np.array_equal(G["edges"], c.edges), (tag, G["edges"], c.edges)
    # 1: counts.  The single-device counts are per in-box row, ascending: the same rows by input row
    inside = np.flatnonzero(c.inside)
    assert len(S["counts"]) == S["res"]["n_cropped"] == len(inside), tag
    s_cnt = np.full(len(xyz), -1, np.int32)
    s_cnt[inside] = S["counts"]
    zeros, valid_rows = [], []
    for r, k in enumerate(G["ranks"]):
        rows = gc.sent_inside(c, r)
        assert len(k["counts"]) == len(rows), (tag, "n_cropped of rank", r, len(k["counts"]), len(rows))
        own = c.owned[r][rows]
        zeros.append(gc.check_counts(rows, own, k["counts"], s_cnt, tag=(tag, "single-device counts", r)))
        if exact is not None:
            gc.check_counts(rows, own, k["counts"], exact, tag=(tag, "exact counts", r))
        # 2: the rank's valid cloud, by the .w of its rows (an index into the rows it was sent)
        w = np.ascontiguousarray(k["xyzw"][:, 3]).view(np.int32)
        assert ((w >= 0) & (w < len(c.sent[r]))).all() and len(k["normals"]) == len(w), (tag, r)
        valid_rows.append(c.sent[r][w])
        assert np.array_equal(k["xyzw"][:, :3], xyz[valid_rows[-1]]), (tag, r)
    gc.check_ownership(c, valid_rows, S["rows"], tag=tag)
    for key in RES_KEYS:
        assert G["res"][key] == S["res"][key], (tag, key, G["res"][key], S["res"][key])
    assert np.array_equal(G["rows"], S["rows"]) and np.array_equal(G["cloud"], S["cloud"]), tag
    # 3: normals merged by input row
    merged = np.full((len(xyz), 4), np.nan, np.float32)
    for rows, k in zip(valid_rows, G["ranks"]):
        merged[rows] = k["normals"]
    single = np.full((len(xyz), 4), np.nan, np.float32)
    single[S["rows"]] = S["normals"]
    assert np.array_equal(np.isnan(merged), np.isnan(single)), tag
    q98 = ref_dev = worst = None
    if oracle_key is not None:
        n64, o_cnt, n32, keep = oracle(oracle_key)
        assert np.array_equal(np.flatnonzero(np.isfinite(merged[:, 0])), keep), tag
        if c.inside.all():
            assert np.array_equal(o_cnt, S["counts"]), tag                       # the second reference of the counts
        o, nrm = n64[keep], merged[keep]
        a = ang(nrm[:, :3], o[:, :3])
        well = o_cnt[keep] >= 8
        fin = well & np.isfinite(n32[keep][:, 0])
        assert fin.any(), tag
        ref_dev = float(np.quantile(ang(n32[keep][fin, :3], o[fin, :3]), 0.98))
        q98 = float(np.quantile(a[well], 0.98))
        worst = float(a[well].max())
        curv = float(np.quantile(np.abs(nrm[well, 3] - o[well, 3]) / np.maximum(o[well, 3], 1e-12), 0.999))
        curv32 = float(np.quantile(np.abs(n32[keep][fin, 3] - o[fin, 3]) / np.maximum(o[fin, 3], 1e-12), 0.999))
        assert q98 < max(1e-5, ref_dev), (tag, q98, ref_dev)
        if curv32 < 1e-4:
            assert curv < 1e-4, (tag, curv, curv32)
    # 4: voxels and the 1-NN
    assert np.array_equal(G["cen"], S["cen"]) and np.array_equal(G["cnt"], S["cnt"]), tag
    assert np.array_equal(G["vnn"], S["vnn"]), (tag, np.flatnonzero(G["vnn"] != S["vnn"])[:8])
    assert np.array_equal(np.isnan(G["vnrm"]), np.isnan(S["vnrm"])), tag
    if np.isfinite(S["vnrm"]).any():
        assert np.nanmax(np.abs(G["vnrm"] - S["vnrm"])) < 1e-5, tag
    seen = dict(tag=tag, edges=c.edges[1:-1].tolist(), owned=[int(o.sum()) for o in c.owned], sent=[len(s) for s in c.sent],
                n_valid=[len(v) for v in valid_rows], halo_rows_with_count_0=zeros, angle_q98=q98, angle_max=worst, oracle_own_q98=ref_dev)
    print(seen)
    return seen, c, valid_rows


# ---------------------------------------------------------------- the tie clouds over 2, 3 and 4 ranks

@pytest.mark.parametrize("q,leaf,R", gc.CASES, ids=gc.IDS)
def test_tie_cloud_over_ranks(gm, monkeypatch, q, leaf, R):
    for k in ("GM_NORMALS_ROWS", "GM_NORMALS_IMPL"):
        monkeypatch.delenv(k, raising=False)
    name = f"tie_q{q}"
    xyz, radius = nn.case(name)
    CLOUDS[name] = (xyz, radius)
    P, _ = nn.tie_points(q)
    short = np.ascontiguousarray(xyz[:1500])
    CLOUDS[name + "_short"] = (short, radius)
    with gm.GeometricMapping(**config(radius, leaf)) as c:
        S = single_outputs(c, xyz)
        S_short = single_outputs(c, short)
    with gm.GeometricMappingGroup([0] * R, loopback=True, **config(radius, leaf)) as g:
        G = group_outputs(g, xyz)
        check_group(xyz, radius, leaf, R, G, S, exact=nn.tie_counts(q, False), oracle_key=name, tag=f"{name} leaf {leaf} R {R}")
        # 5: the same frame again, then a shorter one on the same group, then the first again
        same_bytes(group_outputs(g, xyz), G)
        G_short = group_outputs(g, short)
        check_group(short, radius, leaf, R, G_short, S_short, exact=nn.count_exact(P[:1500], nn.TIE_M[q]),
                    oracle_key=name + "_short", tag=f"{name} leaf {leaf} R {R}, 1500 rows")
        same_bytes(group_outputs(g, xyz), G)


# ---------------------------------------------------------------- rows ON the lattice planes and at edge +- halo

@functools.lru_cache(maxsize=None)
def planes_case(leaf, R):
    pl = gc.planes_cloud(nn.tunnel_n(20000, 20000), BOUND, leaf, 0.3, R)
    pl.xyz.setflags(write=False)
    return pl


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("leaf", [0.5, 0.3])
def test_rows_on_the_lattice_planes_and_at_the_halo_limits(gm, monkeypatch, leaf, R):
    for k in ("GM_NORMALS_ROWS", "GM_NORMALS_IMPL"):
        monkeypatch.delenv(k, raising=False)
    radius = 0.3
    pl = planes_case(leaf, R)
    xyz = pl.xyz
    key = f"planes_{leaf}_{R}"
    CLOUDS[key] = (xyz, radius)
    S = single_frame(gm, xyz, radius, leaf)
    with gm.GeometricMappingGroup([0] * R, loopback=True, **config(radius, leaf)) as g:
        G = group_outputs(g, xyz)
    seen, c, valid_rows = check_group(xyz, radius, leaf, R, G, S, oracle_key=key, tag=key)
    assert np.array_equal(c.edges, pl.edges) and all(len(v) > 0 for v in valid_rows)
    # the row ON an edge comes out of the upper rank, the float below it out of the lower one; both are valid rows
    planes = {float(xyz[row, 0]): k for k, row in pl.plane_rows.items()}
    kept = set(S["rows"].tolist())
    assert set(pl.plane_rows.values()) <= kept and set(pl.below_rows.values()) <= kept and set(pl.halo_rows.tolist()) <= kept
    for g_ in range(1, R):
        k = planes[c.edges[g_]]
        assert pl.plane_rows[k] in set(valid_rows[g_].tolist()) and pl.below_rows[k] in set(valid_rows[g_ - 1].tolist()), (key, g_)


def test_rows_on_the_box_bound(gm, monkeypatch):
    """The group's n_cropped comes from the host plan, the single-device frame's from the device crop: rows at exactly
    +-bound (inside) and at the floats just beyond (outside), in every coordinate."""
    for k in ("GM_NORMALS_ROWS", "GM_NORMALS_IMPL"):
        monkeypatch.delenv(k, raising=False)
    from geometric_mapping_amd import synth
    radius, leaf, R = 0.3, 0.5, 4
    base = synth.tunnel_frame(20000, seed=31, outlier_frac=0.01)
    xyz = gc.bound_cloud(base, BOUND)
    inside = gc.inside_box(xyz, BOUND)
    planted = np.arange(len(base), len(xyz))
    assert inside[planted].sum() == len(planted) // 2 and (~inside[:len(base)]).sum() > 100
    S = single_frame(gm, xyz, radius, leaf)
    assert S["res"]["n_cropped"] == inside.sum()
    with gm.GeometricMappingGroup([0] * R, loopback=True, **config(radius, leaf)) as g:
        G = group_outputs(g, xyz)
    assert G["res"]["n_cropped"] == S["res"]["n_cropped"]
    check_group(xyz, radius, leaf, R, G, S, tag="box bound")


# ---------------------------------------------------------------- ranks with nothing

def nothing_clouds():
    a = gc.sheet(2000, 0.3, 0.45, 1)
    bad = np.full((600, 3), np.nan, np.float32)
    bad[200:] = gc.sheet(400, 0.3, 0.45, 2) + np.array([0.0, 6.0, 0.0], np.float32)      # y outside the box
    bad[400:, :] = gc.sheet(200, 5.5, 5.9, 3)                                             # x outside the box
    return {"own_nothing": a, "sent_nothing": a - np.array([0.3, 0, 0], np.float32), "empty": np.zeros((0, 3), np.float32),
            "nan_or_outside": bad}


@pytest.mark.parametrize("which", ["own_nothing", "sent_nothing", "empty", "nan_or_outside"])
def test_ranks_with_nothing(gm, monkeypatch, which):
    for k in ("GM_NORMALS_ROWS", "GM_NORMALS_IMPL"):
        monkeypatch.delenv(k, raising=False)
    radius, leaf, R = 0.3, 0.5, 4
    xyz = nothing_clouds()[which]
    after = nn.tunnel_n(8191, 8191)
    with gm.GeometricMapping(**config(radius, leaf)) as c:
        S = single_outputs(c, xyz)
        S_after = single_outputs(c, after)
    with gm.GeometricMappingGroup([0] * R, loopback=True, **config(radius, leaf)) as g:
        G = group_outputs(g, xyz)
        G_after = group_outputs(g, after)
    for key in RES_KEYS + ("scatter6", "eigenvalues", "eigenvectors", "center_axis"):
        assert np.array_equal(G["res"][key], S["res"][key], equal_nan=True), (which, key, G["res"][key], S["res"][key])
    for key in ("cloud", "rows", "cen", "cnt", "vnn"):
        assert np.array_equal(G[key], S[key]), (which, key)
    assert np.array_equal(G["vnrm"], S["vnrm"], equal_nan=True), which
    if which in ("own_nothing", "sent_nothing"):
        seen, c_, valid_rows = check_group(xyz, radius, leaf, R, G, S, tag=which)
        assert [len(v) for v in valid_rows][1:] == [0, 0, 0] and S["res"]["n_valid"] > 1500
        assert [len(k["counts"]) for k in G["ranks"]] == ([2000] * 4 if which == "own_nothing" else [2000, 0, 0, 0])
    else:
        assert G["res"]["n_valid"] == 0 and G["res"]["n_in"] == len(xyz) and len(G["cloud"]) == 0 and len(G["cen"]) == 0
        assert all(len(k["counts"]) == 0 and len(k["xyzw"]) == 0 for k in G["ranks"])
        assert np.array_equal(G["edges"][1:-1], [0.0] * (R - 1))
    check_group(after, radius, leaf, R, G_after, S_after, tag=which + ", the frame after")


# ---------------------------------------------------------------- a 1-NN tie across an edge

@pytest.mark.parametrize("swapped", [False, True], ids=["lower_first", "upper_first"])
def test_nearest_point_tie_across_an_edge(gm, monkeypatch, swapped):
    for k in ("GM_NORMALS_ROWS", "GM_NORMALS_IMPL"):
        monkeypatch.delenv(k, raising=False)
    t = gc.NN_TIE
    xyz, a, b0, C = gc.nn_tie_cloud(swapped)
    S = single_frame(gm, xyz, t["radius"], t["leaf"])
    with gm.GeometricMappingGroup([0] * t["R"], loopback=True, **config(t["radius"], t["leaf"])) as g:
        G = group_outputs(g, xyz)
    seen, c, valid_rows = check_group(xyz, t["radius"], t["leaf"], t["R"], G, S, tag=f"nn tie, swapped {swapped}")
    # the construction as the device sees it: A and B0 valid, out of different ranks, C a centroid, the fp32 d2 bits equal
    assert a in valid_rows[0] and b0 in valid_rows[1]
    v = int(np.flatnonzero((S["cen"] == C).all(axis=1))[0])
    assert S["cnt"][v] == 3
    brute = bn.nearest_brute(S["cloud"], S["cen"])
    first = min(a, b0)
    assert S["rows"][brute[v]] == first and np.array_equal(S["vnn"], brute)
    assert G["rows"][G["vnn"][v]] == first
    assert np.array_equal(G["vnn"], S["vnn"]) and np.array_equal(G["vnrm"], S["vnrm"], equal_nan=True)
    assert np.array_equal(G["vnrm"][v], S["normals"][brute[v]])


# ---------------------------------------------------------------- the three copies of the ownership test

CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import geometric_mapping_amd as g
from geometric_mapping_amd import _lib
import normals_np as nn
xyz, radius = nn.case('tie_q7')
kw = dict(boxFilterBound=5.0, neighborRadius=radius, voxelGridLeafSize=0.125,
          flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_KEEP_COUNTS | _lib.GM_CFG_NEAREST)
out = {{}}
with g.GeometricMapping(**kw) as c:
    c.process_frame(xyz)
    out['kept'] = c.cropped_cloud()[1]
with g.GeometricMappingGroup([0] * 4, loopback=True, **kw) as grp:
    res = grp.process_frame(xyz)
    out['edges'] = grp.edges()[0]
    out['n_valid'] = np.array(res['n_valid'])
    for r in range(4):
        out['counts%d' % r] = grp.rank_fetch(r, 0, 'neighbor_counts')
        out['xyzw%d' % r] = grp.rank_fetch(r, 0, 'cropped_xyz')
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("impl", ["valu", "mfma0", "rows2"])
def test_every_formulation_owns_the_same_rows(impl):
    """q.x >= own_lo && q.x < own_hi is written in emit_normal and in the halo-only skip of k_normals_valu, k_normals<D>
    and k_normals_m: GM_NORMALS_IMPL / GM_NORMALS_ROWS (read once per process: a fresh child, one at a time) put each of
    them under assertion 1 and the ranks' half of assertion 2 on the tie_q7, leaf 0.125, 4-rank case."""
    q, leaf, R = 7, 0.125, 4
    env = dict(os.environ)
    for k in ("GM_NORMALS_IMPL", "GM_NORMALS_ROWS", "GM_SORT_STAGED", "GM_MX_BAND_SCALE"):
        env.pop(k, None)
    if impl.startswith("rows"):
        env["GM_NORMALS_ROWS"] = impl[4:]
    else:
        env["GM_NORMALS_IMPL"] = impl
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, impl + ".npz")
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")), f], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = dict(np.load(f))
    xyz, radius = nn.case("tie_q7")
    c = gc.cut(xyz, BOUND, leaf, radius, R)
    exact = nn.tie_counts(q, False)
    assert np.array_equal(got["edges"], c.edges)
    valid_rows, zeros = [], []
    for r in range(R):
        rows = gc.sent_inside(c, r)
        zeros.append(gc.check_counts(rows, c.owned[r][rows], got[f"counts{r}"], exact, tag=(impl, r)))
        valid_rows.append(c.sent[r][np.ascontiguousarray(got[f"xyzw{r}"][:, 3]).view(np.int32)])
    gc.check_ownership(c, valid_rows, got["kept"], tag=impl)             # (kept: the child's own single-device frame)
    assert sum(len(v) for v in valid_rows) == int(got["n_valid"]) == len(got["kept"]) and (exact[got["kept"]] >= 3).all()
    print(impl, "halo rows with count 0 per rank:", zeros)
