"""The fp64 statements of "inlier" (tests/ransac_np.py) against the C restatement's fp32 counts, on the CPU: the oracle's
count of every hypothesis must lie in [certain, certain + near], and the near sets must stay as thin as the GPU tests
assume (ransac_np.NEAR_SHARE_ALL / NEAR_SHARE_HYP).  2048 oracle hypotheses of both models on three scenes: the
radius-2 tunnel with a floor, a tilted off-centre tunnel, and a pipe thinner than the threshold (lo2 = -1 bands)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_np as rn  # noqa: E402

B, R, LEAF, WF = 5.0, 0.5, 0.5, 0.2
H = 2048


@pytest.mark.parametrize("scene", ["tunnel", "tilted", "pipe"])
def test_fp32_counts_lie_in_the_fp64_interval(oc, scene):
    xyz, tau = dict(tunnel=rn.scene_tunnel, tilted=rn.scene_tilted, pipe=rn.scene_pipe)[scene](7000)
    ref = oc.process_frame(xyz, B, R, LEAF, WF, oc.F64)
    cloud, nrm = ref["xyz"], ref["normals"]
    assert len(cloud) > 5000   # (the box crops the 12 m tunnel)
    labels = (np.arange(len(cloud)) % 3 == 0).astype(np.uint8)
    hp = oc.plane_hypotheses(cloud, 11, H)
    hc = oc.cylinder_hypotheses(cloud, nrm, 12, H)
    if scene == "pipe":
        assert (hc[:, 6] < tau).mean() > 0.25           # the lo2 = -1 branch carries a large part of this scene
    for lab, want in ((None, 0), (labels, 0)):
        n_el = len(cloud) if lab is None else int((lab == want).sum())
        for interval, score, hyp in ((rn.plane_interval, oc.score_planes, hp), (rn.cyl_interval, oc.score_cylinders, hc)):
            certain, near = interval(cloud, hyp, tau, lab, want)
            got = rn.check_interval(score(cloud, hyp, tau, lab, want), certain, near, n_el)
            print(scene, interval.__name__, "labels" if lab is not None else "all", got)
            assert got["violations"] == 0
            assert got["near_all"] <= rn.NEAR_SHARE_ALL and got["near_hyp"] <= rn.NEAR_SHARE_HYP
    nan = np.full((2, 7), np.nan, np.float32)
    assert rn.cyl_interval(cloud, nan, tau)[0].tolist() == [0, 0] and rn.cyl_interval(cloud, nan, tau)[1].tolist() == [0, 0]
    assert rn.plane_interval(cloud, nan[:, :4], tau)[0].tolist() == [0, 0] and rn.plane_interval(cloud, nan[:, :4], tau)[1].tolist() == [0, 0]


def test_staged_best_reports_ties(oc):
    """staged_best on a scorer with known counts: the selections take count descending, index ascending."""
    counts = np.array([5, 9, 9, 7, 7, 7, 7, 3, 7, 7, 1, 9], np.int32)     # 12 hypotheses -> one selection (keep 8)
    hyp = np.arange(12, dtype=np.float32).reshape(-1, 1)
    score = lambda cloud, h, tau, labels, want: counts[h[:, 0].astype(int)]
    best, n, info = rn.staged_best(score, np.zeros((40, 3), np.float32), hyp, None, 0.03)
    assert (best, n) == (1, 9) and info["top_ties"] == 3
    st, = info["stages"]
    assert (st["stride"], st["keep"], st["cut"], st["above"], st["at_cut"]) == (16, 8, 7, 3, 6)
    assert st["kept"].tolist() == [1, 2, 3, 4, 5, 6, 8, 11] and info["finalists"].tolist() == st["kept"].tolist()
