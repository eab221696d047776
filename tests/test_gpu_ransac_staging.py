"""The in-frame RANSAC (csrc/k_ransac.hip) through every shape its launchers take: staged scoring, the folded radix
select and k_select_topk, the replicated counters, the label pass.

Every case is an ordinary frame.  run_case reads back the device's own valid cloud, normals and labels and rebuilds the
frame's RANSAC on them in two layers:

  exact        the frame's hypotheses are taken from the stage calls (plane_hypotheses / cylinder_hypotheses run the same
               kernels with the same seeds on the same inputs), tests/ransac_np.staged_best runs the staging over the C
               restatement's fp32 scorers, and the reported rows, inlier counts and labels must equal it bit for bit.
  independent  the finalists' device counts and the winner's reported count lie in the fp64 interval
               [certain, certain + near] of tests/ransac_np.py, and every label outside the winner's near set equals the
               fp64 decision.  The near sets must be as thin as tests/test_ransac_reference.py pins them (NEAR_SHARE_*):
               a condition on the inputs.

The last test writes what the cases saw (n_valid, winners, near shares, ties at the cuts and at the top) to
build/ransac_staging_observed.json (git-ignored).
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, R, LEAF, WF = 5.0, 0.5, 0.5, 0.2
OUTSIDE = 9.0            # a coordinate beyond the crop box
OBSERVED = {}            # case name -> what run_case saw


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def stage(gm):
    """A context for the stage calls only: they upload into their slot, so the frame under test keeps its own."""
    c = gm.GeometricMapping()
    yield c
    c.close()


def frame_context(gm, H, tau, seed=7, plane=True):
    from geometric_mapping_amd import _lib
    flags = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_CYLINDER | (_lib.GM_CFG_RANSAC_PLANE if plane else 0)
    return gm.GeometricMapping(flags=flags, ransac_hypotheses=H, ransac_threshold=tau, ransac_seed=seed)


def run_case(gm, oc, stage, name, xyz, H, tau, seed=7, plane=True, ctx=None, n_valid=None):
    """One frame, both layers (module docstring).  Returns dict(res, lab, n, plane=..., cylinder=...) with, per model,
    hyp (the frame's hypotheses), best, info (staged_best's)."""
    c = ctx if ctx is not None else frame_context(gm, H, tau, seed, plane)
    try:
        res = c.process_frame(xyz)
        cloud, _ = c.cropped_cloud()
        nrm = c.normals()
        lab = c.labels()
        n = len(cloud)
        assert res["n_valid"] == n == len(lab) == len(nrm)
        if n_valid is not None:
            assert res["n_valid"] == n_valid
        out = dict(res=res, lab=lab, n=n)
        obs = OBSERVED[name] = dict(n_valid=n, H=H, tau=tau)
        labels = np.zeros(n, np.uint8)           # the restatement's running labels
        for model in ((0, 1) if plane else (1,)):
            key = ("plane", "cylinder")[model]
            elig = None if (model == 0 or not plane) else labels.copy()     # the first model of a frame sees every point
            n_el = n if elig is None else int((elig == 0).sum())
            if model == 0:
                hyp = stage.plane_hypotheses(cloud, seed, H, None, 0)
                score, label, interval, decide = oc.score_planes, oc.label_plane, rn.plane_interval, rn.plane_decide
            else:
                hyp = stage.cylinder_hypotheses(cloud, nrm, seed + 1, H, elig, 0)
                score, label, interval, decide = oc.score_cylinders, oc.label_cylinder, rn.cyl_interval, rn.cyl_decide
            row, cnt = res[key], int(res[key + "_inliers"])
            best, nbest, info = rn.staged_best(score, cloud, hyp, elig, tau)
            # ---- exact layer
            assert same_bits(row, hyp[best]), (name, key, best, row, hyp[best])
            assert cnt == nbest, (name, key, cnt, nbest)
            if np.isnan(hyp).all():              # nothing could be drawn: index 0, no inlier, the NaN row reported
                assert best == 0 and cnt == 0 and np.isnan(row).all()
            assert label(cloud, labels, 0, model + 1, row, tau) == cnt
            # ---- independent layer
            fin = info["finalists"]
            certain, near = interval(cloud, hyp[fin], tau, elig, 0)
            k = int(np.flatnonzero(fin == best)[0])
            assert certain[k] <= cnt <= certain[k] + near[k], (name, key, cnt, certain[k], near[k])
            staged = rn.check_interval(info["final_counts"], certain, near, n_el)
            dev = c.score_frame(model, hyp[fin], tau)                       # exhaustive scorer, every point of the frame
            c_all, n_all = (certain, near) if elig is None else interval(cloud, hyp[fin], tau)
            whole = rn.check_interval(dev, c_all, n_all, n)
            assert staged["violations"] == 0 and whole["violations"] == 0, (name, key, staged, whole)
            if elig is None:
                assert np.array_equal(dev, info["final_counts"])
            for got in (staged, whole):
                assert got["near_all"] <= rn.NEAR_SHARE_ALL and got["near_hyp"] <= rn.NEAR_SHARE_HYP, (name, key, got)
            inl, nr = decide(cloud, row[None], tau)
            sure = ~nr[0] if model == 0 else ~nr[0] & (lab != 1)
            assert np.array_equal(lab[sure] == model + 1, inl[0][sure]), (name, key)
            out[key] = dict(hyp=hyp, best=best, info=info)
            obs[key] = dict(winner=best, inliers=cnt, finalists=fin.tolist(), top_ties=info["top_ties"],
                            nan_hypotheses=int(np.isnan(hyp[:, 0]).sum()),
                            cuts=[dict(keep=s["keep"], cut=s["cut"], above=s["above"], at_cut=s["at_cut"]) for s in info["stages"]],
                            near_all=max(staged["near_all"], whole["near_all"]), near_hyp=max(staged["near_hyp"], whole["near_hyp"]),
                            winner_near=int(nr.sum()))
            if model == 1:
                obs[key]["r_below_tau"] = float((hyp[:, 6] < tau).mean())
        assert np.array_equal(lab, labels), name                            # byte for byte
        assert int((lab == 1).sum()) == res["plane_inliers"] and int((lab == 2).sum()) == res["cylinder_inliers"]
        if not plane:
            assert res["plane_inliers"] == 0 and np.isnan(res["plane"]).all()
        return out
    finally:
        if ctx is None:
            c.close()


def index_order_decides(info):
    """At every cut more candidates sit ON the cut count than the selection may take from them."""
    return all(s["at_cut"] > s["keep"] - s["above"] for s in info["stages"])


# ---- inputs ------------------------------------------------------------------------------------------------------------

def padded(xyz, rows):
    """xyz spread evenly over `rows` input rows; the others lie outside the crop box."""
    out = np.full((rows, 3), OUTSIDE, np.float32)
    out[np.linspace(0, rows - 1, len(xyz)).astype(np.int64)] = xyz
    return out


def frame_with_n_valid(oc, target):
    """Input rows whose valid cloud (inside the box, three or more neighbours within R: a finite normal) has exactly
    `target` points by the C restatement, among rows outside the box."""
    from geometric_mapping_amd import synth
    if target == 0:
        pts = np.zeros((0, 3), np.float32)
    elif target == 1:      # the middle point sees three points, the outer two see two
        pts = np.array([[0, 0, 0], [0.4, 0.02, 0], [-0.4, 0, 0.03]], np.float32)
    elif target == 2:      # a and b see each other and one more each; c and d see two
        pts = np.array([[0, 0, 0], [0.1, 0.03, 0], [-0.45, 0, 0.02], [0.55, 0, -0.02]], np.float32)
    elif target == 30:     # two parallel sheets, 24 + 6 points: every triple of a sheet spans the same plane, so finalists tie
        xy = np.random.default_rng(30).uniform(-0.3, 0.3, (30, 2))
        pts = np.concatenate([xy, np.where(np.arange(30) % 5 == 2, 0.1, -0.1)[:, None]], axis=1).astype(np.float32)
    else:
        pts = None
        for seed, m in ((s, m) for s in range(9, 14) for m in range(target, target + 8)):
            cand = synth.tunnel_frame(m, seed=seed, radius=0.3, length=0.8) if target < 200 else rn.scene_small_tunnel(m, seed)[0]
            if oc.process_frame(cand, B, R, LEAF, WF, oc.F64)["n_valid"] == target:
                pts = cand
                break
        assert pts is not None, target
    xyz = padded(pts, len(pts) + 300)
    assert oc.process_frame(xyz, B, R, LEAF, WF, oc.F64)["n_valid"] == target
    return xyz


@pytest.fixture(scope="module")
def tunnel20k():
    return rn.scene_tunnel(24000)      # ~20 k of them inside the box


# ---- cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 8, 9, 128, 129, 512, 513, 2048, 2049, 4097, 8192])
def test_every_shape_of_the_staging_plane_then_cylinder(gm, oc, stage, tunnel20k, H):
    """Exhaustive (H <= 8), two stages (<= 128), three; a second row of hypothesis blocks from 513; all 8 keys per thread
    of the folded select at 2048; k_select_topk and the memset of the replicated counters from 2049; hypothesis index
    8191, the last the 13-bit key field holds, at 8192."""
    xyz, tau = tunnel20k
    out = run_case(gm, oc, stage, f"tunnel_H{H}", xyz, H, tau)
    assert 18000 < out["n"] < 22000
    if H >= 128:
        assert out["res"]["plane_inliers"] > 4000 and out["res"]["cylinder_inliers"] > 4000


@pytest.mark.parametrize("H", [129, 2048, 2049, 8192])
def test_cylinder_as_the_first_model(gm, oc, stage, tunnel20k, H):
    """GM_CFG_RANSAC_CYLINDER alone: labels == nullptr through the scorers and init = 1 in the cylinder's label pass."""
    xyz, tau = tunnel20k
    out = run_case(gm, oc, stage, f"tunnel_cylinder_only_H{H}", xyz, H, tau, plane=False)
    assert out["res"]["cylinder_inliers"] > 4000


@pytest.mark.parametrize("H", [129, 2049])
@pytest.mark.parametrize("scene", ["tilted", "pipe"])
def test_tilted_tunnel_and_thin_pipe(gm, oc, stage, scene, H):
    """Nothing axis-aligned; and a pipe thinner than tau, whose hypotheses carry the lo2 = -1 band through k_score,
    k_score_sel, k_score_stream and k_label."""
    xyz, tau = (rn.scene_tilted if scene == "tilted" else rn.scene_pipe)(20000)
    # (a plane with tau = 0.3 through the pipe's axis would take the whole pipe: the pipe runs the cylinder alone)
    out = run_case(gm, oc, stage, f"{scene}_H{H}", xyz, H, tau, plane=scene == "tilted")
    if scene == "pipe":
        hyp = out["cylinder"]["hyp"]
        assert (hyp[:, 6] < tau).mean() >= 0.10
        assert hyp[out["cylinder"]["info"]["finalists"], 6].min() < tau      # and such a band reaches the last stage
    else:
        assert out["res"]["cylinder_inliers"] > 4000 and abs(out["res"]["cylinder"][6] - 1.1) < 0.05


@pytest.mark.parametrize("n_valid", [63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097])
def test_n_valid_around_the_tiles(gm, oc, stage, n_valid):
    """One subsampled point (n_valid <= 64); the 32-point stage-1 tile (2048 / 64); the 256-point block of
    k_score_sel<*, 64> (4096 / 16); the 1024-point span of k_score_stream."""
    run_case(gm, oc, stage, f"n_valid_{n_valid}", frame_with_n_valid(oc, n_valid), 2049, 0.03, n_valid=n_valid)


@pytest.mark.parametrize("H", [9, 2049])
@pytest.mark.parametrize("n_valid", [0, 1, 2, 5, 30])
def test_nearly_empty_frames(gm, oc, stage, n_valid, H):
    """No hypothesis can be drawn (winner = index 0, no inlier, labels all 0, NaN rows reported: run_case), then a
    handful of points, where the finalists tie on the full count."""
    out = run_case(gm, oc, stage, f"n_valid_{n_valid}_H{H}", frame_with_n_valid(oc, n_valid), H, 0.03, n_valid=n_valid)
    if n_valid <= 1:
        assert np.isnan(out["plane"]["hyp"]).all() and np.isnan(out["cylinder"]["hyp"]).all()
        assert not out["lab"].any() and np.isnan(out["res"]["plane"]).all() and np.isnan(out["res"]["cylinder"]).all()
    if n_valid == 30:
        assert out["plane"]["info"]["top_ties"] >= 2


@pytest.mark.parametrize("H", [2048, 2049, 8192])
@pytest.mark.parametrize("n", [700, 2500])
def test_ties_at_both_cuts(gm, oc, stage, n, H):
    """Small frames: a stage sees 11 / 44 or 40 / 157 points, counts tie by the dozen and index order decides who
    passes a cut -- in the folded radix select (2048) and in k_select_topk (2049, 8192)."""
    xyz, tau = rn.scene_small_tunnel(n)
    out = run_case(gm, oc, stage, f"small_tunnel_{n}_H{H}", xyz, H, tau)
    for key in ("plane", "cylinder"):
        info = out[key]["info"]
        assert len(info["stages"]) == 2 and index_order_decides(info), (key, info["stages"])


def test_floor_dominated_frame(gm, oc, stage):
    """A 20 k-point floor and a 1 k-point tunnel: after the plane most draws of a cylinder hypothesis land on label 1, so
    hypotheses that ran out of draws (NaN rows) go through the select beside finite ones."""
    from geometric_mapping_amd import synth
    floor = synth.plane_patch(20000, seed=6, normal=(0, 0, 1), offset=-1.2, half=4.5, sigma=0.01)
    xyz = np.concatenate([floor, rn.scene_small_tunnel(1000)[0]])
    xyz = xyz[np.random.default_rng(1).permutation(len(xyz))]
    out = run_case(gm, oc, stage, "floor_dominated_H2049", xyz, 2049, 0.03)
    nan = np.isnan(out["cylinder"]["hyp"][:, 0])
    assert 100 < nan.sum() < 1949, int(nan.sum())
    assert out["res"]["plane_inliers"] > 15000


@pytest.fixture(scope="module")
def inflated():
    xyz, tau = rn.scene_tunnel(30000, seed=12)     # ~25 k inside the box
    return padded(xyz, 4_300_000), tau


@pytest.mark.parametrize("H", [1024, 8192])
def test_grids_far_larger_than_the_frame(gm, oc, stage, inflated, H):
    """~25 k valid points among 4.3 M input rows: every grid is sized for 4.5 M points (the 256-point stage-1 tile,
    k_score_sel<*, 256> at K = 128, the 2048-block cap and grid-stride loop of k_score_stream, the caps of k_label) and
    nearly every block is empty -- and still has to report to the done-counter."""
    xyz, tau = inflated
    out = run_case(gm, oc, stage, f"inflated_H{H}", xyz, H, tau)
    assert out["res"]["n_in"] == 4_300_000 and 23000 < out["n"] < 27000
    assert out["res"]["plane_inliers"] > 4000 and out["res"]["cylinder_inliers"] > 4000


@pytest.mark.parametrize("H", [2048, 8192])
def test_one_context_frames_of_different_grids(gm, oc, stage, tunnel20k, H):
    """Big, small, big on one context: the counters, the done word and the replicated counts are left clean."""
    big, tau = tunnel20k
    small, _ = rn.scene_small_tunnel(700)
    with frame_context(gm, H, tau) as c:
        a = run_case(gm, oc, stage, f"reuse_H{H}_big", big, H, tau, ctx=c)
        run_case(gm, oc, stage, f"reuse_H{H}_small", small, H, tau, ctx=c)
        b = run_case(gm, oc, stage, f"reuse_H{H}_big_again", big, H, tau, ctx=c)
    for key in ("plane", "cylinder"):
        assert same_bits(a["res"][key], b["res"][key]) and a["res"][key + "_inliers"] == b["res"][key + "_inliers"]
    assert np.array_equal(a["lab"], b["lab"])


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import geometric_mapping_amd as g
from geometric_mapping_amd import _lib
import ransac_np as rn
out = {}
both = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER
for name, (xyz, tau) in (("tunnel", rn.scene_tunnel(24000)), ("pipe", rn.scene_pipe(20000)), ("small", rn.scene_small_tunnel(700))):
    flags = both & ~_lib.GM_CFG_RANSAC_PLANE if name == "pipe" else both     # (a tau = 0.3 plane would take the whole pipe)
    with g.GeometricMapping(flags=flags, ransac_hypotheses=2048, ransac_threshold=tau, ransac_seed=7) as c:
        res = c.process_frame(xyz)
        out[name + "_labels"] = c.labels()
    for k in ("plane", "cylinder", "plane_refit", "cylinder_axis_refit"):
        out[name + "_" + k] = res[k]
    out[name + "_counts"] = np.array([res["n_valid"], res["plane_inliers"], res["cylinder_inliers"]])
np.savez(sys.argv[1], **out)
"""
SWITCHES = ("GM_RANSAC_SELECT", "GM_RANSAC_FINAL", "GM_LABEL_MASKS")


def run_child(path, **env_set):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def default_child():
    with tempfile.TemporaryDirectory() as d:
        return run_child(os.path.join(d, "default.npz"))


@pytest.mark.parametrize("switch", ["GM_RANSAC_SELECT=kernel", "GM_RANSAC_FINAL=sel", "GM_LABEL_MASKS=1"])
def test_documented_switches_change_no_bit(default_child, switch):
    """The environment switches of DESIGN.md (read once per process -> child processes, one at a time): selections in
    launches of their own at H = 2048, the last stage in the lane <-> hypothesis shape (k_score_sel split for K <= 32),
    and the streaming stage's inlier masks with the by-mask label pass.  A 20 k tunnel, the thin pipe and a 700-point
    frame (ties at the cuts): rows, counts, labels and refits equal the default process's bit for bit."""
    k, v = switch.split("=")
    with tempfile.TemporaryDirectory() as d:
        got = run_child(os.path.join(d, "switch.npz"), **{k: v})
    assert sorted(got) == sorted(default_child)
    for name, a in default_child.items():
        b = got[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (switch, name)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (switch, name, a, b)
    assert default_child["tunnel_counts"][1] > 4000 and default_child["small_counts"][0] == 700


def test_zz_write_what_the_cases_observed():
    """The numbers behind the caps and the tie / r < tau conditions, on record (runs last: the file's order)."""
    def plain(o):
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        return o.item() if isinstance(o, np.generic) else o
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", "ransac_staging_observed.json"), "w") as f:
        json.dump(dict(near_share_caps=dict(all_pairs=rn.NEAR_SHARE_ALL, per_hypothesis=rn.NEAR_SHARE_HYP), cases=plain(OBSERVED)),
                  f, indent=1, sort_keys=True)
    for name, obs in OBSERVED.items():
        for key in ("plane", "cylinder"):
            if key in obs:
                assert obs[key]["near_all"] <= rn.NEAR_SHARE_ALL and obs[key]["near_hyp"] <= rn.NEAR_SHARE_HYP, (name, key)
