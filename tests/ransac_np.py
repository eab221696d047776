"""Plain numpy references of the in-frame RANSAC (csrc/k_ransac.hip): no GPU, none of the code under test.

staged_best restates the staging of launch_score_preemptive over any exhaustive scorer and reports what the selections
had to decide (ties at the cuts and at the top).  plane_interval / cyl_interval state "inlier" in fp64 and return, per
hypothesis, how many eligible points are inliers beyond doubt (`certain`) and how many lie so close to the band edge that
an fp32 evaluation may decide either way (`near`): a correct fp32 count lies in [certain, certain + near].

The margins (U = 2^-24, the unit roundoff of fp32):
  cylinder  q = fma(-t, t, vv), vv = fma(vx, vx, fma(vy, vy, vz * vz)), t = fma(vx, dx, fma(vy, dy, vz * dz)): the
            three-term chains round three times each and q once more; every intermediate is bounded by |v|^2 or t^2, the
            band edges (fp32 roundings of lo^2 / hi^2) by hi^2.  near: |q - edge| <= 4 U (|v|^2 + t^2 + hi^2).
  plane     dist = fma(a, x, fma(b, y, fma(c, z, d))): the two inner roundings are bounded by the sum of the absolute
            terms (the last one rounds a value near tau, far smaller).  near: ||dist| - tau| <= 2 U (|ax| + |by| + |cz| + |d|).
tests/test_ransac_reference.py checks them against the C restatement's fp32 counts on every CPU run.
"""
import numpy as np

U = 2.0 ** -24
STAGES = ((64, 128), (16, 8))      # (point stride, hypotheses kept): kPre1* / kPre2* of csrc/k_ransac.hip
NEAR_SHARE_ALL = 5e-4              # conditions on a test's INPUTS (not measurements): near pairs / all pairs ...
NEAR_SHARE_HYP = 0.02              # ... and near points / points for any single hypothesis


def staged_best(score_fn, cloud, hyp, labels, tau, want=0):
    """The in-frame RANSAC's staged scoring (csrc/k_ransac.hip launch_score_preemptive), restated with an exhaustive
    scorer score_fn(cloud, hyp, tau, labels, want) -> counts: all hypotheses on every 64th point -> 128 best (count
    desc, index asc) -> those on every 16th point -> 8 best -> those on every point -> best full count (lowest index on
    ties).  H <= 128 starts at the second stage, H <= 8 is exhaustive.  labels None: every point is eligible.

    Returns (winner id, winner count, info).  info["stages"] has one dict per selection that ran: stride, keep, kept
    (sorted ids), cut (the count of the last candidate kept), above (candidates with a larger count) and at_cut
    (candidates with exactly that count: index order decides keep - above of them).  info["finalists"] /
    info["final_counts"] are the last stage's ids (ascending) and full counts, info["top_ties"] the number of finalists
    that share the winning count."""
    cloud = np.asarray(cloud)
    ids = np.arange(len(hyp))
    stages = []
    for stride, keep in STAGES:
        if len(ids) > keep:
            c = score_fn(cloud[::stride], hyp[ids], tau, None if labels is None else labels[::stride], want)
            order = np.lexsort((ids, -c))
            cut = int(c[order[keep - 1]])
            stages.append(dict(stride=stride, keep=keep, cut=cut, above=int((c > cut).sum()), at_cut=int((c == cut).sum()),
                               kept=np.sort(ids[order[:keep]])))
            ids = ids[order[:keep]]
    ids = np.sort(ids)
    c = score_fn(cloud, hyp[ids], tau, labels, want)
    k = np.lexsort((ids, -c))[0]
    info = dict(stages=stages, finalists=ids, final_counts=np.asarray(c).copy(), top_ties=int((c == c[k]).sum()))
    return int(ids[k]), int(c[k]), info


def _eligible(n, labels, want):
    return np.ones(n, bool) if labels is None else (np.asarray(labels) == want)


def plane_decide(cloud, hyp4, tau):
    """fp64 decision of every (hypothesis, point) pair: (inlier [H, n] bool, near [H, n] bool).  Non-finite rows: False."""
    p = np.asarray(cloud, np.float64)
    h = np.asarray(hyp4, np.float32).reshape(-1, 4).astype(np.float64)
    t32 = float(np.float32(tau))
    with np.errstate(invalid="ignore"):
        ax, by, cz = h[:, 0:1] * p[:, 0], h[:, 1:2] * p[:, 1], h[:, 2:3] * p[:, 2]
        dist = np.abs(ax + by + cz + h[:, 3:4])
        mag = np.abs(ax) + np.abs(by) + np.abs(cz) + np.abs(h[:, 3:4])
        near = np.abs(dist - t32) <= 2 * U * mag
        inl = dist < t32
    ok = np.isfinite(h).all(axis=1)[:, None]
    return inl & ok, near & ok


def cyl_decide(cloud, hyp7, tau):
    """fp64 decision of every (hypothesis, point) pair: (inlier [H, n] bool, near [H, n] bool).  Non-finite rows: False."""
    p = np.asarray(cloud, np.float64)
    h = np.asarray(hyp7, np.float32).reshape(-1, 7).astype(np.float64)
    r = h[:, 6:7]
    lo, hi = r - float(tau), r + float(tau)
    with np.errstate(invalid="ignore"):
        lo2 = np.where(lo > 0, lo * lo, -1.0)
        hi2 = hi * hi
        vx, vy, vz = p[:, 0] - h[:, 0:1], p[:, 1] - h[:, 1:2], p[:, 2] - h[:, 2:3]
        t = vx * h[:, 3:4] + vy * h[:, 4:5] + vz * h[:, 5:6]
        vv = vx * vx + vy * vy + vz * vz
        q = vv - t * t
        m = 4 * U * (vv + t * t + hi2)
        near = (np.abs(q - lo2) <= m) | (np.abs(q - hi2) <= m)
        inl = (q > lo2) & (q < hi2)
    ok = np.isfinite(h).all(axis=1)[:, None]
    return inl & ok, near & ok


def _interval(decide, cloud, hyp, tau, labels, want, chunk):
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    hyp = np.asarray(hyp, np.float32)
    hyp = hyp.reshape(-1, hyp.shape[-1])
    el = _eligible(len(cloud), labels, want)
    pts = cloud[el]
    certain = np.zeros(len(hyp), np.int64)
    near = np.zeros(len(hyp), np.int64)
    step = max(1, chunk // max(len(pts), 1))
    for s in range(0, len(hyp), step):
        i, nr = decide(pts, hyp[s:s + step], tau)
        certain[s:s + step] = (i & ~nr).sum(axis=1)
        near[s:s + step] = nr.sum(axis=1)
    return certain, near


def plane_interval(cloud, hyp4, tau, labels=None, want=0, chunk=1 << 21):
    """(certain, near) per plane hypothesis over the points with labels == want (all when labels is None)."""
    return _interval(plane_decide, cloud, hyp4, tau, labels, want, chunk)


def cyl_interval(cloud, hyp7, tau, labels=None, want=0, chunk=1 << 21):
    """(certain, near) per cylinder hypothesis over the points with labels == want (all when labels is None)."""
    return _interval(cyl_decide, cloud, hyp7, tau, labels, want, chunk)


def check_interval(counts, certain, near, n_eligible):
    """What every comparison against an interval reports: violations (counts outside [certain, certain + near]), the
    overall near share and the largest per-hypothesis near share."""
    counts = np.asarray(counts, np.int64)
    bad = int(((counts < certain) | (counts > certain + near)).sum())
    n = max(int(n_eligible), 1)
    return dict(violations=bad, near_all=float(near.sum()) / (n * max(len(near), 1)), near_hyp=float(near.max(initial=0)) / n)


# ---- the scenes the references are pinned on (and the GPU cases run): (input rows, tau) ----------------------------------

def scene_tunnel(n, seed=2):
    """Tunnel r = 2 along x through the origin, floor at z = -1.2, 1 % outliers; tau = 0.03."""
    from geometric_mapping_amd import synth
    return synth.tunnel_frame(n, seed=seed, floor_z=-1.2, outlier_frac=0.01), 0.03


def scene_tilted(n, seed=3):
    """Nothing axis-aligned: tunnel r = 1.1 along (0.3, 1, 0.4) through (0.4, -0.3, 0.5), 2 % outliers; tau = 0.03."""
    from geometric_mapping_amd import synth
    xyz = synth.tunnel_frame(n, seed=seed, radius=1.1, length=9.0, axis=(0.3, 1.0, 0.4), outlier_frac=0.02)
    return xyz + np.array([0.4, -0.3, 0.5], np.float32), 0.03


def scene_pipe(n, seed=4):
    """A pipe thinner than the threshold: r = 0.2 along x, tau = 0.3, so a hypothesis near the truth has r - tau < 0 and
    its band is the whole disc (cyl_band's lo2 = -1); 5 % outliers."""
    from geometric_mapping_amd import synth
    return synth.tunnel_frame(n, seed=seed, radius=0.2, length=8.0, sigma=0.005, outlier_frac=0.05), 0.3


def scene_small_tunnel(n, seed=5):
    """A short narrow tunnel for frames of a few hundred to a few thousand points (dense enough for normals at the
    default 0.5 search radius): r = 1, length 3.5, floor at z = -0.6; tau = 0.03."""
    from geometric_mapping_amd import synth
    return synth.tunnel_frame(n, seed=seed, radius=1.0, length=3.5, floor_z=-0.6), 0.03
