"""k_normals and its tile cutter (csrc/k_normals.hip) at row, chunk and radius-band edges, through whole frames.

Every case is a cloud of tests/normals_np.py's table: the plan twin there says which mechanism the cloud reaches (the
cutter's backwards walk over several 4096-position steps, row starts on and around a cutter block's first position,
64-chunks cut again at cell groups, tiles of 1 .. 64 queries on the matrix-core path, the candidate stream's octet and
128-slot edges, the thin / matrix-core switch at 64 candidates, exact ties and near-ties inside the error band, the
fine-row instantiation), and tests/test_normals_reference.py asserts those claims on every CPU run.  Here the frame runs
on the GPU and must give
  * the C oracle's neighbour counts, bit for bit, every point -- and on the integer tie clouds count_exact's, which uses
    no floating point;
  * n_cropped = n (every point lies inside the box: counts come back in input order), the oracle's kept rows;
  * normals by the project's rule (tests/test_gpu_fuzz.py): the 0.98 quantile of the angle to the f64 oracle below
    max(1e-5, the f32-faithful oracle's own), relative curvature at quantile 0.999 below 1e-4 where the f32-faithful mode
    itself is.
The frame's grid depends on (bound, radius), which a context fixes: the r = 0.1 and r = 0.3 cases run back to back on two
module-scoped contexts each -- n_slots = 1 (tiles filed by cost class) and n_slots = 2 (position order) -- so that a small
frame follows a larger one's row table, tile lists and scan records; a tie cloud has a radius of its own and a short-lived
pair of contexts.  The last test writes what the cases saw to build/normals_edges_observed.json (git-ignored) and asserts
that every mechanism key of the table was reached by a case that ran.
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_np as nn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"classes": 1, "position": 2}          # n_slots
OBSERVED = {"cases": {}, "band_scale": {}}
SHARED = {(5.0, nn.R01), (5.0, 0.3)}             # (bound, radius) groups that share a context per shape
N_EDGE = [name for name in nn.CASES if name.startswith("tunnel_n")]


def ang(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=-1) / np.maximum(np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1), 1e-300)
    return np.arcsin(np.clip(s, 0, 1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's view of a case, computed once: f64 normals and counts, kept rows, the f32-faithful normals."""
    from oracle import oracle_c as oc
    oc.build()
    xyz, radius = nn.case(name)
    n64, cnt = oc.normals(xyz, radius, oc.F64)
    n32, _ = oc.normals(xyz, radius, oc.F32_FAITHFUL)
    keep = oc.finite_normals(n64)
    for a in (n64, cnt, n32, keep):
        a.setflags(write=False)
    return n64, cnt, n32, keep


def flags(gm, graph=False):
    from geometric_mapping_amd import _lib
    return _lib.GM_CFG_DEFAULT | _lib.GM_CFG_KEEP_COUNTS | (_lib.GM_CFG_GRAPH if graph else 0)


@pytest.fixture(scope="module")
def shared(gm):
    made = {}

    def get(shape, bound, radius):
        key = (shape, bound, radius)
        if key not in made:
            made[key] = gm.GeometricMapping(boxFilterBound=bound, neighborRadius=radius, n_slots=SHAPES[shape], flags=flags(gm))
        return made[key]

    yield get
    for c in made.values():
        c.close()


def check_frame(ctx, name, tag, rows=None, frames=1):
    """One case on one context; `frames`: how often the frame is sent (the last one is checked)."""
    c = nn.CASES[name]
    xyz, radius = nn.case(name)
    n64, o_cnt, n32, keep = reference(name)
    for _ in range(frames):
        res = ctx.process_frame(xyz)
    cnt = ctx.neighbor_counts()
    nrm = ctx.normals()
    cloud, crows = ctx.cropped_cloud()
    assert res["n_cropped"] == len(xyz), name
    bad = np.flatnonzero(cnt != o_cnt)
    assert len(bad) == 0, (name, tag, len(bad), bad[:8], cnt[bad[:8]], o_cnt[bad[:8]])
    if c.tie is not None:
        assert np.array_equal(cnt, nn.tie_counts(*c.tie)), (name, tag)
    assert np.array_equal(crows, keep) and np.array_equal(cloud, xyz[keep]), (name, tag)
    assert res["n_valid"] == len(keep) == len(nrm)
    assert (o_cnt[keep] >= 3).all() and len(keep) > 0
    o = n64[keep]
    a = ang(nrm[:, :3], o[:, :3])
    well = o_cnt[keep] >= 8
    fin = well & np.isfinite(n32[keep][:, 0])
    assert fin.any(), name
    ref_dev = float(np.quantile(ang(n32[keep][fin, :3], o[fin, :3]), 0.98))
    q98 = float(np.quantile(a[well], 0.98))
    curv = float(np.quantile(np.abs(nrm[well, 3] - o[well, 3]) / np.maximum(o[well, 3], 1e-12), 0.999))
    curv32 = float(np.quantile(np.abs(n32[keep][fin, 3] - o[fin, 3]) / np.maximum(o[fin, 3], 1e-12), 0.999))
    p, s = nn.case_plan(name, rows)
    census = nn.case_census(name)
    OBSERVED["cases"][f"{name}/{tag}"] = dict(
        n=len(xyz), D=s["D"], tiles=s["tiles"], chunks=s["chunks"], thin_tiles=s["thin_tiles"],
        tie_pairs=census[0] if census else 0, in_band_pairs=census[1] if census else 0, angle_q98=q98, ref_dev_q98=ref_dev,
        curvature_rel_q999=curv, curvature_rel_q999_f32=curv32, reached=sorted(nn.reached(name, rows)))
    print(name, tag, OBSERVED["cases"][f"{name}/{tag}"])
    assert q98 < max(1e-5, ref_dev), (name, tag, q98, ref_dev)
    if curv32 < 1e-4:
        assert curv < 1e-4, (name, tag, curv, curv32)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(nn.CASES))
def test_case_matches_oracle(gm, shared, monkeypatch, name, shape):
    monkeypatch.delenv("GM_NORMALS_ROWS", raising=False)
    c = nn.CASES[name]
    radius = nn.case(name)[1]
    if (c.bound, radius) in SHARED:
        check_frame(shared(shape, c.bound, radius), name, shape)
    else:
        with gm.GeometricMapping(boxFilterBound=c.bound, neighborRadius=radius, n_slots=SHAPES[shape], flags=flags(gm)) as ctx:
            check_frame(ctx, name, shape)


@pytest.mark.parametrize("name", N_EDGE)
def test_frame_that_fills_its_context(gm, monkeypatch, name):
    """n on and around the cutter's 4096-position blocks on a context whose capacity is n: nothing behind the frame."""
    monkeypatch.delenv("GM_NORMALS_ROWS", raising=False)
    c = nn.CASES[name]
    with gm.GeometricMapping(boxFilterBound=c.bound, neighborRadius=c.radius, max_points=len(nn.case(name)[0]), flags=flags(gm)) as ctx:
        check_frame(ctx, name, "full")


@pytest.mark.parametrize("name,rows", nn.FINE_VARIANTS)
def test_fine_rows(gm, monkeypatch, name, rows):
    """k_normals<true> forced onto the case (GM_NORMALS_ROWS, read when the frame's grid is made)."""
    monkeypatch.setenv("GM_NORMALS_ROWS", str(rows))
    c = nn.CASES[name]
    assert nn.case_plan(name, rows)[1]["D"] == rows
    with gm.GeometricMapping(boxFilterBound=c.bound, neighborRadius=nn.case(name)[1], flags=flags(gm)) as ctx:
        check_frame(ctx, name, f"rows{rows}", rows=rows)


@pytest.mark.parametrize("name", nn.GRAPH_VARIANTS)
def test_replayed_from_a_graph(gm, monkeypatch, name):
    monkeypatch.delenv("GM_NORMALS_ROWS", raising=False)
    c = nn.CASES[name]
    with gm.GeometricMapping(boxFilterBound=c.bound, neighborRadius=nn.case(name)[1], flags=flags(gm, graph=True)) as ctx:
        check_frame(ctx, name, "graph", frames=2)          # the second frame of a context is the replayed one


BAND_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import geometric_mapping_amd as g
from geometric_mapping_amd import _lib
import normals_np as nn
out = {{}}
for name in sys.argv[2:]:
    xyz, radius = nn.case(name)
    with g.GeometricMapping(boxFilterBound=nn.CASES[name].bound, neighborRadius=radius, flags=_lib.GM_CFG_DEFAULT | _lib.GM_CFG_KEEP_COUNTS) as c:
        c.process_frame(xyz)
        out[name] = c.neighbor_counts()
np.savez(sys.argv[1], **out)
"""
BAND_CASES = ["tie_q7", "tie_q12", "tie_q14", "tie_q7_up", "tie_q12_up", "tie_q14_up", "tie_q10", "tie_q10_up"]


def test_tie_clouds_need_the_band():
    """The teeth of the tie cases.  GM_MX_BAND_SCALE=0.001 (the experiment switch, read once per process: a child) puts
    the band below one ulp of r2, so no pair is re-evaluated and the distance product's own rounding decides the pairs at
    and beside the threshold.  Measured: the q = 7, 10 and 12 clouds still match count_exact, every point -- on
    lattices of up to 12 bits every term of the product (offsets from the tile origin below 1, their squares multiples of
    2^-24 below 1) and every partial sum is an fp32 of its own, so the product is exact and a tie comes out as 0, which is
    "not a neighbour" (DESIGN.md par. 5).  The strengthened cloud is tie_q14: a 2^-14 lattice, where the offsets' squares
    round, with pairs planted at and within two steps of the threshold.  Its counts must DIFFER from count_exact without
    the band -- under the default band test_case_matches_oracle holds all of them equal.  The others are on record."""
    code = BAND_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    env = dict(os.environ)
    env.pop("GM_NORMALS_ROWS", None)
    env.pop("GM_NORMALS_IMPL", None)
    env["GM_MX_BAND_SCALE"] = "0.001"
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "counts.npz")
        r = subprocess.run([sys.executable, "-c", code, f] + BAND_CASES, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = dict(np.load(f))
    for name in BAND_CASES:
        OBSERVED["band_scale"][name] = int((got[name] != nn.tie_counts(*nn.CASES[name].tie)).sum())
    print("points whose count differs without the band:", OBSERVED["band_scale"])
    assert OBSERVED["band_scale"]["tie_q14"] > 0, OBSERVED["band_scale"]


def test_zz_write_what_the_cases_observed():
    """On record (runs last: the file's order), and every mechanism key of the table was reached by a case that ran."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", "normals_edges_observed.json"), "w") as f:
        json.dump(OBSERVED, f, indent=1, sort_keys=True)
    for shape in SHAPES:
        got = set().union(*(o["reached"] for k, o in OBSERVED["cases"].items() if k.endswith("/" + shape)))
        assert got >= set(nn.ALL_MECH) - {"fine_D2", "fine_D4", "fine_passes_3", "fine_pieces_4"}, (shape, sorted(set(nn.ALL_MECH) - got))
    got = set().union(*(o["reached"] for o in OBSERVED["cases"].values()))
    assert got >= set(nn.ALL_MECH), sorted(set(nn.ALL_MECH) - got)
    for name in N_EDGE:
        assert f"{name}/full" in OBSERVED["cases"]
    assert all(f"{name}/graph" in OBSERVED["cases"] for name in nn.GRAPH_VARIANTS)
    assert {"tie_q7", "tie_q12", "tie_q14"} <= set(OBSERVED["band_scale"])
