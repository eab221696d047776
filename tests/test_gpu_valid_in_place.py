"""The NaN-normal compaction works in place (csrc/k_frame.hip, csrc/gm_compact.hpp): the valid cloud is the head of the
cropped cloud's own buffer, the valid normals the head of the per-point normals' buffer.  k_valid_scan counts, finds the
first dropped row and sums getLocalFrame's scatter terms; k_compact<MovePred, MoveEmit> moves the rows behind the first
dropped row down, inside the buffers it reads from.

Exact layer (gm_compact_valid_stage; reference: plain numpy): survivors bit-equal and in order, the count, and scatter6
against the fp64 numpy sum of the same terms with the bound test_gpu_parity.py uses for gm_get_local_frame (5e-7 of the
largest entry).  Every case runs with the default tile (4096 rows) in this process and with GM_VALID_TILE=1024x8 (8192
rows) and 256x8 (2048 rows) in child processes (the variable is read once per process).

Frame layer: clouds of a lattice patch of tunnel wall (dozens of neighbours inside the radius) plus isolated points
farther than two radii from everything, which lose their normal by construction, at input rows 0, 4095, 4096 and n-1; through
gm_get_normals_stage and whole frames, plain, captured (GM_CFG_GRAPH), with a /choppedCloud buffer registered and with two
slots in flight.  Normals against the oracle with test_gpu_parity.py's tolerances (1e-5 rad, 1e-4 relative curvature at the
0.999 quantile).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WF = 0.2
SCATTER_BOUND = 5e-7   # tests/test_gpu_parity.py::test_local_frame_vs_oracle
B, R = 5.0, 0.5


# ------------------------------------------------------------------ exact layer

def make_rows(n, drops, curvature_nan=()):
    """n cloud rows (distinct values, the row index in .w) and n normal rows; `drops` lose their normal: NaN in x only, y
    only, z only, +inf, -inf in turn.  `curvature_nan` rows get a NaN curvature and a finite normal: they stay."""
    i = np.arange(n, dtype=np.int64)
    rows = np.empty((n, 4), np.float32)
    rows[:, 0] = i * 0.25 + 0.125
    rows[:, 1] = -(i * 0.5) - 1.0
    rows[:, 2] = (i % 1021) * 3.0 + 7.0
    rows[:, 3] = i.astype(np.int32).view(np.float32)
    rng = np.random.default_rng(n * 7919 + len(drops))
    nrm = rng.normal(size=(n, 4)).astype(np.float32)
    nrm[:, :3] /= np.maximum(np.linalg.norm(nrm[:, :3], axis=1, keepdims=True), 1e-6)
    nrm[:, 3] = rng.uniform(0.0, 0.3, n).astype(np.float32)
    nrm[:, 0] += (i % 4093).astype(np.float32) * np.float32(1e-5)   # (distinct rows; the direction need not be a unit vector)
    drops = np.asarray(drops, dtype=np.int64)
    for k, d in enumerate(drops):
        kind = k % 5
        if kind < 3:
            nrm[d, kind] = np.nan
        elif kind == 3:
            nrm[d, k % 3] = np.inf
        else:
            nrm[d, k % 3] = -np.inf
    for d in curvature_nan:
        nrm[d, 3] = np.nan
    return rows, nrm


def scatter_ref(nrm, wf):
    """getLocalFrame's sums as the kernels form them: w = float(exp((c + .001/wf)^2)) from doubles, one fp32 product per
    component, exact fp64 products of those, summed in fp64."""
    t = nrm[:, 3].astype(np.float64) + 0.001 / wf
    w = np.exp(t * t).astype(np.float32)
    a = (w * nrm[:, 0]).astype(np.float64)
    b = (w * nrm[:, 1]).astype(np.float64)
    c = (w * nrm[:, 2]).astype(np.float64)
    return np.array([np.sum(a * a), np.sum(a * b), np.sum(a * c), np.sum(b * b), np.sum(b * c), np.sum(c * c)])


def exact_cases(T):
    """(name, n, dropped rows) for tiles of T rows."""
    c = []
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 8192, 12289):
        c.append(("dense_%d" % n, n, []))
    n1 = 3 * T + 17
    for d in (0, n1 - 1, 4095, 4096, 4097, 3 * T):           # 3 T: the first row of the last tile
        c.append(("one_drop_%d_of_%d" % (d, n1), n1, [d]))
    c.append(("one_drop_first_of_last_whole_tile", 3 * T, [2 * T]))
    c.append(("one_drop_last_of_last_whole_tile", 3 * T, [3 * T - 1]))
    c.append(("clean_prefix_then_moving_tile", n1, [2 * T + 5]))
    c.append(("tile_lands_in_the_tile_before", 3 * T, list(range(T, 2 * T))))
    c.append(("one_drop_per_tile", 3 * T, [7, T + 100, 3 * T - 1]))
    c.append(("every_second_row_four_tiles", 4 * T, list(range(0, 4 * T, 2))))
    c.append(("all_dropped", 2 * T + 3, list(range(2 * T + 3))))
    c.append(("all_but_the_last_dropped", 2 * T + 3, list(range(2 * T + 2))))
    c.append(("empty", 0, []))
    rng = np.random.default_rng(20240)
    c.append(("forty_tiles_one_percent", 163840, sorted(rng.choice(163840, 1638, replace=False).tolist())))
    return c


def check_exact(ctx, n, drops, curvature_nan=()):
    rows, nrm = make_rows(n, drops, curvature_nan)
    mask = np.isfinite(nrm[:, :3]).all(axis=1)
    assert int((~mask).sum()) == len(drops)
    out, on, sc = ctx.compactValid(WF, rows, nrm)
    assert out.shape[0] == int(mask.sum()) and on.shape[0] == int(mask.sum())
    # bit-equal, order included (compared as integers: NaN payloads count)
    assert np.array_equal(out.view(np.uint32), rows[mask].view(np.uint32))
    assert np.array_equal(on.view(np.uint32), nrm[mask].view(np.uint32))
    if len(curvature_nan):
        assert np.isnan(sc).any()
    else:
        ref = scatter_ref(nrm[mask], WF)
        assert np.abs(sc - ref).max() <= SCATTER_BOUND * np.abs(ref).max()
    return out, on, sc


@pytest.fixture(scope="module")
def ctx(gm):
    c = gm.GeometricMapping(boxFilterBound=B, neighborRadius=R, weightingFactor=WF)
    yield c
    c.close()


_CASES = exact_cases(4096)


@pytest.mark.parametrize("name,n,drops", _CASES, ids=[c[0] for c in _CASES])
def test_exact_default_tile(ctx, name, n, drops):
    check_exact(ctx, n, drops)


def test_exact_curvature_nan_keeps_the_row(ctx):
    check_exact(ctx, 4096 + 300, [5, 4100], curvature_nan=[0, 6, 4095, 4096, 4395])


def check_sequence(make_ctx, T):
    """Stale rows, records, ticket words or counters of a call would show in the next one: each call of a dropping, dense,
    dropping sequence on one context equals the same call on a fresh context, bit for bit."""
    seq = [(3 * T + 17, list(range(3, 3 * T, 11))), (3 * T + 17, []), (2 * T + 1, [T - 1, T, 2 * T])]
    with make_ctx() as one:
        got = [check_exact(one, n, d) for n, d in seq]
    for (n, d), g in zip(seq, got):
        with make_ctx() as fresh:
            f = check_exact(fresh, n, d)
        assert np.array_equal(g[0].view(np.uint32), f[0].view(np.uint32))
        assert np.array_equal(g[1].view(np.uint32), f[1].view(np.uint32))
        assert np.array_equal(g[2], f[2])


def test_exact_dropping_dense_dropping_on_one_context(gm):
    check_sequence(lambda: gm.GeometricMapping(weightingFactor=WF), 4096)


def child_main(tile_rows):
    """Runs in a child process (GM_VALID_TILE set by the parent): every exact case, on one context."""
    import geometric_mapping_amd as g
    g.load_library()
    with g.GeometricMapping(weightingFactor=WF) as c:
        for name, n, drops in exact_cases(int(tile_rows)):
            check_exact(c, n, drops)
            print("ok", name, flush=True)
        check_exact(c, 4096 + 300, [5, 4100], curvature_nan=[0, 6, 4095, 4096, 4395])
    check_sequence(lambda: g.GeometricMapping(weightingFactor=WF), int(tile_rows))
    print("all ok", flush=True)


@pytest.mark.parametrize("tile,tile_rows", [("1024x8", 8192), ("256x8", 2048)])
def test_exact_other_tiles_in_a_child_process(gm, tile, tile_rows):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_valid_in_place as t; "
            "t.child_main(sys.argv[1])" % (os.path.dirname(here), here))
    env = dict(os.environ)
    env["GM_VALID_TILE"] = tile
    r = subprocess.run([sys.executable, "-c", code, str(tile_rows)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "all ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ frame layer

ISO = np.array([[-1.5, 0.0, 0.5], [0.0, 0.0, 0.5], [1.5, 0.0, 0.5], [0.0, 0.0, 2.0]], np.float32)   # > 2 R from everything


def lattice(n):
    """n points of a tunnel wall patch (radius 2.5 m about the x axis), 0.05 m apart along x and along the arc: ~300
    neighbours inside R = 0.5, curvature as on the tunnel frames the tolerances were set on; all inside the crop box."""
    k = np.arange(n)
    x = -1.8 + 0.05 * (k // 72)
    th = -2.3 + 0.02 * (k % 72)
    return np.stack([x, 2.5 * np.cos(th), 2.5 * np.sin(th)], axis=1).astype(np.float32)


def frame(n, iso_rows):
    """n input rows: lattice points, with isolated points at the given input rows."""
    xyz = lattice(n)
    for k, r in enumerate(iso_rows):
        xyz[r] = ISO[k]
    mask = np.ones(n, bool)
    mask[list(iso_rows)] = False
    return xyz, mask


N_FRAME = 72 * 72 + 4   # 5188 rows: two tiles of 4096
FRAMES = [("dense", []), ("row_0", [0]), ("row_last", [N_FRAME - 1]), ("rows_4095_4096", [4095, 4096]),
          ("all_four", [0, 4095, 4096, N_FRAME - 1])]


@pytest.fixture(scope="module")
def refs(oc):
    """Oracle normals of each frame, computed once and left alone."""
    out = {}
    for name, iso in FRAMES:
        xyz, mask = frame(N_FRAME, iso)
        o_n, _ = oc.normals(xyz, R, oc.F64)
        assert np.array_equal(oc.finite_normals(o_n), np.flatnonzero(mask))   # the construction holds
        o_n.setflags(write=False)
        out[name] = (xyz, mask, o_n[mask])
    return out


def ang(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    return np.arcsin(np.clip(s, 0, 1))


def check_normals(nrm, o):
    assert nrm.shape == o.shape
    assert np.isfinite(nrm[:, :3]).all()
    assert np.quantile(ang(nrm[:, :3], o[:, :3]), 0.999) < 1e-5
    rel = np.abs(nrm[:, 3] - o[:, 3]) / np.maximum(o[:, 3], 1e-12)
    assert np.quantile(rel, 0.999) < 1e-4


def check_frame(c, slot, res, xyz, mask, o_n):
    assert res["n_cropped"] == len(xyz) and res["n_valid"] == int(mask.sum())
    cloud, rows = c.cropped_cloud(slot)
    assert np.array_equal(rows, np.flatnonzero(mask))          # input rows in .w
    assert np.array_equal(cloud.view(np.uint32), xyz[mask].view(np.uint32))
    check_normals(c.normals(slot), o_n)
    return cloud, rows


@pytest.mark.parametrize("name", [f[0] for f in FRAMES])
def test_normals_stage(ctx, refs, name):
    xyz, mask, o_n = refs[name]
    nrm, cloud, rows = ctx.getNormals(R, xyz)
    assert np.array_equal(rows, np.flatnonzero(mask))
    assert np.array_equal(cloud.view(np.uint32), xyz[mask].view(np.uint32))
    check_normals(nrm, o_n)


@pytest.mark.parametrize("name", [f[0] for f in FRAMES])
def test_whole_frame(ctx, refs, name):
    xyz, mask, o_n = refs[name]
    res = ctx.process_frame(xyz)
    cloud, rows = check_frame(ctx, 0, res, xyz, mask, o_n)
    if name == "dense":
        assert res["n_valid"] == res["n_cropped"]
        chopped, kept = ctx.chopCloud(B, xyz)                  # the crop alone
        assert np.array_equal(cloud.view(np.uint32), chopped.view(np.uint32)) and np.array_equal(rows, kept)


def test_whole_frames_through_one_capture(gm, refs):
    from geometric_mapping_amd import _lib
    with gm.GeometricMapping(boxFilterBound=B, neighborRadius=R, weightingFactor=WF,
                             flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_GRAPH) as c:
        for name in ("dense", "all_four", "dense", "rows_4095_4096", "row_0"):
            xyz, mask, o_n = refs[name]
            check_frame(c, 0, c.process_frame(xyz), xyz, mask, o_n)


@pytest.mark.parametrize("graph", [False, True])
def test_cloud_output_buffer(gm, refs, graph):
    """The page-locked /choppedCloud rows: a dropping frame (the head left with the crop, the moved tail re-sent), then a
    dense frame (nothing re-sent), then another dropping one."""
    from geometric_mapping_amd import _lib
    with gm.GeometricMapping(boxFilterBound=B, neighborRadius=R, weightingFactor=WF,
                             flags=_lib.GM_CFG_DEFAULT | (_lib.GM_CFG_GRAPH if graph else 0)) as c:
        buf = c.cloud_output(0, N_FRAME + 100)
        for name in ("all_four", "dense", "rows_4095_4096"):
            xyz, mask, o_n = refs[name]
            res = c.process_frame(xyz)
            got = buf[:res["n_valid"]].copy()
            cloud, rows = check_frame(c, 0, res, xyz, mask, o_n)
            assert np.array_equal(got[:, :3].view(np.uint32), cloud.view(np.uint32))
            assert np.array_equal(got[:, 3].copy().view(np.int32), rows)


def test_two_slots_in_flight(gm, refs):
    with gm.GeometricMapping(boxFilterBound=B, neighborRadius=R, weightingFactor=WF, n_slots=2) as c:
        order = ["all_four", "dense", "row_last", "rows_4095_4096"]
        c.submit_frame(0, refs[order[0]][0])
        for i in range(1, len(order) + 1):
            if i < len(order):
                c.submit_frame(i % 2, refs[order[i]][0])
            xyz, mask, o_n = refs[order[i - 1]]
            check_frame(c, (i - 1) % 2, c.wait_frame((i - 1) % 2), xyz, mask, o_n)
