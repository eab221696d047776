"""GPU tests of the wall-map align (gm_wall_map_align_*, csrc/k_wall_align.hip + gm_wall_slot.hip): the table, the counts and
the info integers against the exact twin (tests/wall_align_np.py) fed the device's own (cell, e) pairs and read_raw, at every
frame size where the bin kernel takes another path and at the edges of the score kernel; the table's independence of the
block shape; the truth of shifted poses; the ambiguity on a smooth wall; what an align is for (the check it repairs); the
frame path against the stage path over every pipeline path, the ordering rule and the scratch."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_align_np as an  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
KW = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)
# The bin kernel runs the add's grid (1024 threads, two points per thread and trip): one block up to 2048 points, then one
# per 2048 up to 48 blocks.  63 .. 65: a wave's edge; 1023 .. 1025: the block's edge, the second wave-trip slot of the
# unroll; 2047 .. 2049: the unroll's edge, then the second block; 98304, 98305: 48 blocks full, then their second trip.
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 98304, 98305)
NST, NS, DS, RADIUS = 96, 32, 0.25, 2.0
P = wn.params(n_stations=NST, n_sectors=NS, station_length=DS, radius=RADIUS)
TEX = dict(seed=5, amplitude=0.04, length=24.0)
SIGMA = 0.005
SWEEP_KW = dict(half_patch_stations=12)   # 3 m of a frame's 5 m of reach: the far points are outside the patch
AMBIGUOUS_CAP = 0.02      # (the fp64 twin alone on the sweep's inputs: at most 0.5 % of a frame's points ambiguous)
DTH = 2 * np.pi / NS
WHOLE = ((3, 2), (-2, -1), (0, 0), (5, 0))
FRACTIONAL = ((1.3, -0.4), (-2.25, 1.7), (0.4, 0.3))
# The fp64 twin's worst errors over the three frames and FRACTIONAL (align() of the twin, scratch run on the CPU):
# 0.070 cell of chainage, 0.044 cell of roll.  Five times that, never more than half a cell.
TWIN_WORST_STATION, TWIN_WORST_SECTOR = 0.070, 0.044
BOUND_STATION, BOUND_SECTOR = min(5 * TWIN_WORST_STATION, 0.5), min(5 * TWIN_WORST_SECTOR, 0.5)


def survey_raw(texture=TEX, n=200_000, seed=1, p=P):
    """Twin-made raw cells of a wall surveyed at the identity pose: n points over the whole map, 5 mm noise, the texture."""
    rng = np.random.default_rng(seed)
    nst, ns = p["n_stations"], p["n_sectors"]
    t = rng.uniform(0.0, nst * p["station_length"], n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    rr = RADIUS + rng.normal(0.0, SIGMA, n)
    if texture is not None:
        rr = rr + synth.wall_texture(t, phi, **texture)
    world = np.stack([t, -rr * np.sin(phi), rr * np.cos(phi)], axis=1).astype(np.float32)
    r = wn.points(world, None, wn.add_frame(wn.design_frame(p), p, np.eye(4)[:3]), p)
    return wn.cells_from(r["e"].astype(np.float32), r["cell"], nst * ns).reshape(nst, ns)


def drive(n_points=20_000, texture=TEX):
    """Three frames 3.5 m apart on the textured wall, 5 m of reach: (cloud, true pose)."""
    return synth.tunnel_drive(3, n_points, seed=7, length=24.0, start=8.0, step=3.5, reach=5.0, sigma=SIGMA, patches=(),
                              texture=texture)["frames"]


def moved(pose, sa, sb, p=P):
    """The pose a caller would hold whose chainage is sa stations short and whose roll is sb sectors short of `pose`."""
    return an.compose(wn.design_frame(p), pose, -sa * p["station_length"], -sb * 2 * np.pi / p["n_sectors"])


def _map_state(m):
    i = m.info()
    return m.read_raw().tobytes(), tuple(i[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))


def against_twin(m, p, xyz, lab, pose, raw=None, per_point=True, **kw):
    """One stage call against the twin: the table, the counts and the info integers byte for byte from the device's own
    (cell, e) pairs and read_raw; e and cell against the fp64 chain outside the ambiguity mask.  Returns (info, table, twin
    patch (sum, count), ambiguous fraction)."""
    ap = an.prm(**kw)
    ns = p["n_sectors"]
    n = len(xyz)
    info, tab, res, cell = m.align_points(xyz, pose, labels=lab, **kw)
    raw = m.read_raw() if raw is None else raw
    labs = np.zeros(n, np.uint8) if lab is None else lab
    assert info["n_points"] == n and len(res) == len(cell) == n
    assert (info["half_patch_stations"], info["max_station_shift"], info["max_sector_shift"]) == (
        ap["half_patch_stations"], ap["max_station_shift"], ap["max_sector_shift"])
    # the classes from the device's pairs
    plane = labs == 1
    gate = np.float32(ap["gate"])
    with np.errstate(invalid="ignore"):
        beyond = ~plane & ~(np.abs(res) <= gate)
    binned = cell >= 0
    assert not np.any(binned & (plane | beyond)) and np.all(np.isnan(res[plane]))
    assert np.all(cell[binned] < 2 * ap["half_patch_stations"] * ns)
    want = dict(plane=int(plane.sum()), beyond_gate=int(beyond.sum()), binned=int(binned.sum()))
    want["outside_patch"] = n - sum(want.values())
    assert {k: info[k] for k in an.CLASSES} == want
    # the patch, the table and the selection
    psum, pcnt = an.patch_from(res, cell, 2 * ap["half_patch_stations"] * ns)
    assert info["patch_cells_usable"] == int((pcnt >= ap["min_frame_count"]).sum())
    twin = an.table(psum, pcnt, raw, info["anchor_station"], ns, ap)
    assert tab.tobytes() == twin.tobytes()
    sel = an.select(twin, p, pose, ap)
    for k in ("status", "anchor_station", "overlap", "best_station", "best_sector"):
        assert info[k] == sel[k], (k, info[k], sel[k])
    for k in ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction"):
        assert np.isclose(info[k], sel[k], rtol=1e-14, atol=0.0, equal_nan=True), (k, info[k], sel[k])
    assert np.allclose(info["pose"], sel["pose"], rtol=0.0, atol=1e-12, equal_nan=True)
    if info["status"] & _lib.GM_ALIGN_FAILED_MASK:
        assert np.all(np.isnan(info["pose"]))
    else:
        assert wn.pose_ok(info["pose"])
    frac = 0.0
    if per_point and n:
        add = info["add"]
        assert add["gate"] == gate and add["anchor_station"] == info["anchor_station"]
        t = an.points(xyz, lab, add, p, ap)
        amb = t["ambiguous"]
        frac = float(amb.mean())
        assert np.array_equal(cell[~amb], t["cell"][~amb])
        assert np.array_equal(np.isnan(res), np.isnan(t["e"]))
        live = ~np.isnan(res) & np.isfinite(t["e"])
        assert np.abs(res[live].astype(np.float64) - t["e"][live]).max(initial=0.0) <= 2e-6
    return info, tab, (psum, pcnt), frac


# ---- twin parity over the frame sizes ----

def sweep_cases():
    """(n, xyz, labels, pose) per size: the points of a textured frame truncated or tiled to n, every seventh a plane
    point, every eleventh pushed a quarter further from the sensor (beyond the gate), under a pose one station and one
    sector off."""
    frames = drive()
    cases = []
    for k, n in enumerate(SIZES):
        cloud, pose = frames[k % 3]
        xyz = np.ascontiguousarray(np.tile(cloud, ((n + len(cloud) - 1) // len(cloud) or 1, 1))[:n])
        xyz[np.arange(n) % 11 == 3] *= np.float32(1.25)
        cases.append((n, xyz, (np.arange(n) % 7 == 0).astype(np.uint8), moved(pose, 1, -1)))
    return cases


def test_the_twin_alone_stays_under_the_ambiguity_cap():
    """No device: the fp64 chain's own mask on the sweep's inputs."""
    design = wn.design_frame(P)
    worst = 0.0
    for n, xyz, lab, pose in sweep_cases():
        if n:
            ap = an.prm(**SWEEP_KW)
            worst = max(worst, float(an.points(xyz, lab, wn.add_frame(design, P, pose), P, ap)["ambiguous"].mean()))
    print("worst ambiguous fraction:", worst)
    assert worst <= AMBIGUOUS_CAP


def test_sizes_against_the_twin(gm):
    raw = survey_raw()
    seen = dict.fromkeys(an.CLASSES, 0)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**P)
        m.add_raw(raw)
        before = _map_state(m)
        assert m.read_raw().tobytes() == raw.tobytes()
        for n, xyz, lab, pose in sweep_cases():
            info, tab, _, frac = against_twin(m, P, xyz, lab, pose, raw=raw, **SWEEP_KW)
            print(f"n={n}: status={info['status']:#x} best=({info['best_station']}, {info['best_sector']}) "
                  f"distinction={info['distinction']:.2f} overlap={info['overlap']} ambiguous={frac:.4f}",
                  {k: info[k] for k in an.CLASSES})
            assert frac <= AMBIGUOUS_CAP
            for k in an.CLASSES:
                seen[k] += info[k]
            if n < 64:
                assert info["status"] == _lib.GM_ALIGN_NO_OVERLAP and np.all(np.isnan(info["pose"]))
            if n >= 98304:     # the frame tiled five times, every patch cell well above min_frame_count: the shift is found
                assert (info["status"], info["best_station"], info["best_sector"]) == (_lib.GM_ALIGN_OK, 1, -1)
        assert _map_state(m) == before                      # the map is not changed
    assert all(seen[k] > 0 for k in an.CLASSES), seen


# ---- the score kernel's edges ----

def random_raw(p, seed, mean_count=10.0, block=None):
    """Twin-made raw cells with counts around min_count (some below, some empty) and sums of both signs; block: a
    (j0, j1, k0, k1) window of cells moved 0.5 m off."""
    rng = np.random.default_rng(seed)
    nst, ns = p["n_stations"], p["n_sectors"]
    nc = nst * ns
    cell = rng.integers(0, nc, int(mean_count * nc))
    base = rng.normal(0.0, 0.03, nc)
    if block:
        j0, j1, k0, k1 = block
        b = np.zeros((nst, ns))
        b[j0:j1, k0:k1] = 0.5
        base = base + b.reshape(-1)
    e = (base[cell] + rng.normal(0.0, 0.01, len(cell))).astype(np.float32)
    return wn.cells_from(e, cell, nc).reshape(nst, ns)


def random_cloud(p, ap, pose, n, seed):
    """About n points around the sensor of `pose` (no rotation): stations beyond the patch on both sides, every sector,
    residuals of both signs, a few beyond the gate, every ninth a plane point; the cells of every fifth station and every
    third sector keep one point in seven, so that some patch cells stay below min_frame_count."""
    rng = np.random.default_rng(seed)
    ds, ns = p["station_length"], p["n_sectors"]
    reach = (ap["half_patch_stations"] + 2) * ds
    s = pose[0, 3]
    t = rng.uniform(s - reach, s + reach, n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    tex = 0.03 * np.sin(7.0 * t / (reach + 1.0)) * np.cos(3.0 * phi)
    rr = RADIUS + tex + rng.normal(0.0, 0.01, n) + np.where(rng.random(n) < 0.01, 0.4, 0.0)
    thin = (np.floor(t / ds).astype(np.int64) % 5 == 0) & (np.floor(phi / (2 * np.pi / ns)).astype(np.int64) % 3 == 0)
    keep = ~thin | (rng.random(n) < 1.0 / 7.0)
    t, phi, rr, n = t[keep], phi[keep], rr[keep], int(keep.sum())
    world = np.stack([t, -rr * np.sin(phi), rr * np.cos(phi)], axis=1)
    sensor = (world - pose[:, 3]) @ pose[:, :3]
    return np.ascontiguousarray(sensor, np.float32), (np.arange(n) % 9 == 0).astype(np.uint8)


EDGES = {
    # name: (map keywords, sensor chainage, points, align keywords)
    "one_shift": (dict(), 12.1, 20_000, dict(max_station_shift=0, max_sector_shift=0)),
    "full_wrap_33": (dict(n_sectors=33), 12.1, 20_000, dict(max_sector_shift=16, max_station_shift=3)),
    "one_sector": (dict(n_sectors=1), 12.1, 2_000, dict(max_sector_shift=0, min_overlap=8)),
    "ninety_sectors": (dict(n_sectors=90), 12.1, 40_000, dict()),
    "largest_patch": (dict(n_sectors=64, n_stations=400, station_length=0.05), 10.02, 80_000,
                      dict(half_patch_stations=64, max_station_shift=8, max_sector_shift=4)),
    "most_shifts": (dict(), 12.1, 20_000, dict(max_station_shift=64, max_sector_shift=15)),
    "low_end": (dict(), 1.3, 20_000, dict()),             # j_f = 5 < P + A: patch and map rows below station 0
    "high_end": (dict(), 22.9, 20_000, dict()),           # j_f = 91 > n_stations - P - A
    "clamped_block": (dict(), 12.1, 20_000, dict()),      # cells 0.5 m off saturate the clamp
    "thin_counts": (dict(), 12.1, 6_000, dict(min_count=12, min_frame_count=6, min_overlap=16)),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_score_edges_against_the_twin(gm, name):
    mk, s, n, kw = EDGES[name]
    p = wn.params(**dict(P, **mk))
    ap = an.prm(**kw)
    ns = p["n_sectors"]
    block = (40, 56, 3, 9) if name == "clamped_block" else None
    raw = random_raw(p, seed=11, block=block)
    pose = synth.pose_matrix((s, 0.0625, -0.03125))
    xyz, lab = random_cloud(p, ap, pose, n, seed=12)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        m.add_raw(raw)
        before = _map_state(m)
        info, tab, (psum, pcnt), _ = against_twin(m, p, xyz, lab, pose, raw=raw, per_point=False, **kw)
        assert _map_state(m) == before
    print(name, f"status={info['status']:#x} best=({info['best_station']}, {info['best_sector']}) overlap={info['overlap']}",
          {k: info[k] for k in an.CLASSES}, "usable", info["patch_cells_usable"])
    # the case holds what it is there for
    assert all(info[k] > 0 for k in an.CLASSES)
    used_p, used_m = pcnt >= ap["min_frame_count"], raw["count"] >= ap["min_count"]
    assert np.any((pcnt > 0) & ~used_p) and np.any(used_p) and np.any((raw["count"] > 0) & ~used_m) and np.any(used_m)
    rem = lambda s_, c_, u: np.any(u & (s_ < 0) & (np.abs(s_) % np.maximum(c_, 1) != 0))  # noqa: E731
    assert rem(psum, pcnt, used_p) and rem(raw["sum"].astype(np.int64), raw["count"].astype(np.int64), used_m)
    assert tab["n"].max() <= 2 * ap["half_patch_stations"] * ns and np.all(tab["reserved"] == 0)
    if name in ("low_end", "high_end"):
        A, Pp = ap["max_station_shift"], ap["half_patch_stations"]
        jf = info["anchor_station"]
        assert (jf < Pp + A) if name == "low_end" else (jf > p["n_stations"] - Pp - A)
        # the rows outside the map never overlap: fewer cells at the shifts that push the patch further out
        col = tab["n"][:, ap["max_sector_shift"]].astype(np.int64)
        assert (col[0] < col[-1]) if name == "low_end" else (col[0] > col[-1])
    if name == "clamped_block":
        Cq = int(np.rint(ap["clip"] * 2.0 ** 20))
        f = an.values(psum, pcnt, ap["min_frame_count"]).reshape(-1, ns)
        mi = an.map_image(raw, info["anchor_station"], ns, ap["half_patch_stations"], ap["max_station_shift"], ap["min_count"])
        mid = mi[ap["max_station_shift"]:ap["max_station_shift"] + f.shape[0]]
        both = (f != an.NONE) & (mid != an.NONE)
        assert int((np.abs(f - mid)[both] > Cq).sum()) > 20
    if name in ("one_shift",):
        assert tab.shape == (1, 1) and info["distinction"] == np.inf and not info["status"] & _lib.GM_ALIGN_AT_BORDER
    if name == "full_wrap_33":
        assert tab.shape == (7, 33)
        # every sector shift of the ring once: at a = 0 each patch cell meets each sector of its station at some b
    if name == "largest_patch":
        assert 2 * ap["half_patch_stations"] * ns == _lib.GM_WALL_ALIGN_MAX_PATCH_CELLS and info["patch_cells_usable"] > 4000
    if name == "most_shifts":
        assert tab.size == 129 * 31


def test_an_anchor_far_outside_the_map(gm):
    raw = survey_raw()
    cloud, pose = drive()[0]
    far = pose.copy()
    far[0, 3] += 5000 * DS
    with gm.GeometricMapping() as c:
        m = c.wall_map(**P)
        m.add_raw(raw)
        before = _map_state(m)
        info, tab, _, _ = against_twin(m, P, cloud, None, far, raw=raw)
        assert info["anchor_station"] > 5000 and info["binned"] > 10_000 and info["patch_cells_usable"] > 1000
        assert info["status"] == _lib.GM_ALIGN_NO_OVERLAP and np.all(np.isnan(info["pose"])) and info["overlap"] == 0
        assert np.isnan(info["shift_m"]) and np.isnan(info["roll"]) and not tab["n"].any() and not tab["ssd"].any()
        # the other side, and a pose the conversion to a station would overflow on
        near = pose.copy()
        near[0, 3] -= 3000 * DS
        info, tab, _, _ = against_twin(m, P, cloud, None, near, raw=raw)
        assert info["anchor_station"] < -2900 and info["status"] == _lib.GM_ALIGN_NO_OVERLAP and not tab["n"].any()
        gone = pose.copy()
        gone[0, 3] = 1e300
        with pytest.raises(gm.GmError) as e:
            m.align_points(cloud, gone)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        assert _map_state(m) == before


# ---- the table does not depend on the block shape ----

_CHILD = """
import hashlib, sys
sys.path.insert(0, {tests!r})
import geometric_mapping_amd as gm
import test_gpu_wall_align as t
raw = t.survey_raw()
cloud, pose = t.drive()[1]
with gm.GeometricMapping() as c:
    m = c.wall_map(**t.P)
    m.add_raw(raw)
    info, tab, _, _ = m.align_points(cloud, t.moved(pose, -2, 3), outputs=False)
print("TABLE", hashlib.sha256(tab.tobytes()).hexdigest(), hashlib.sha256(info["bytes"]).hexdigest())
"""


def test_table_does_not_depend_on_the_rows_per_block():
    """GM_WALL_ALIGN_ROWS is read at gm_wall_map_create: two shapes (one patch row per block; 7, which does not divide
    the 40 rows) in fresh child processes, and the twin's table from the same inputs."""
    got = {}
    for rows in ("1", "7"):
        env = dict(os.environ, GM_WALL_ALIGN_ROWS=rows)
        r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(ROOT, "tests"))], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got[rows] = [ln for ln in r.stdout.splitlines() if ln.startswith("TABLE")][0]
    assert got["1"] == got["7"]
    cloud, pose = drive()[1]
    want, tab = an.align(cloud, None, P, moved(pose, -2, 3), survey_raw(), an.prm())
    assert (want["best_station"], want["best_sector"]) == (-2, 3)
    print(got["1"], hashlib.sha256(tab.tobytes()).hexdigest())


# ---- truth ----

def test_truth_of_shifted_poses(gm):
    """Whole-cell shifts are found exactly with the flags clear; fractional shifts to within BOUND_STATION / BOUND_SECTOR
    of a cell: five times the fp64 twin's worst on these inputs (0.070 and 0.044 cell), never more than half a cell.  The
    twin's distinction on them: at least 15 at the whole-cell shifts, at least 4.0 at the fractional ones."""
    raw = survey_raw()
    worst = [0.0, 0.0]
    least = np.inf
    with gm.GeometricMapping() as c:
        m = c.wall_map(**P)
        m.add_raw(raw)
        for cloud, true in drive():
            for sa, sb in WHOLE + FRACTIONAL:
                info, _tab, _, _ = m.align_points(cloud, moved(true, sa, sb), outputs=False)
                ea = info["shift_m"] / DS - sa
                eb = info["roll"] / DTH - sb
                print(f"shift ({sa}, {sb}): best ({info['best_station']}, {info['best_sector']}) + ({info['frac_station']:.3f}, "
                      f"{info['frac_sector']:.3f}) error ({ea:.3f}, {eb:.3f}) cells, distinction {info['distinction']:.2f}, "
                      f"overlap {info['overlap']}, status {info['status']:#x}")
                assert info["status"] == _lib.GM_ALIGN_OK and wn.pose_ok(info["pose"])
                least = min(least, info["distinction"])
                if (sa, sb) in WHOLE:
                    assert (info["best_station"], info["best_sector"]) == (sa, sb)
                    assert abs(ea) <= BOUND_STATION and abs(eb) <= BOUND_SECTOR
                else:
                    worst = [max(worst[0], abs(ea)), max(worst[1], abs(eb))]
                    assert abs(ea) <= BOUND_STATION and abs(eb) <= BOUND_SECTOR
                a = wn.design_frame(P)["a"]
                assert abs((info["pose"][:, 3] - true[:, 3]) @ a - ea * DS) <= 1e-9
    print("worst fractional error (cells):", worst, "least distinction:", least)


def test_a_smooth_wall_is_ambiguous(gm):
    """The same frames against a map of a smooth wall: the costs differ by noise only (the twin: 1.0005 .. 1.003)."""
    raw = survey_raw(texture=None)
    with gm.GeometricMapping() as c:
        m = c.wall_map(**P)
        m.add_raw(raw)
        for cloud, true in drive():
            info, _tab, _, _ = m.align_points(cloud, moved(true, 3, 2), outputs=False)
            print(f"smooth map: distinction {info['distinction']:.4f} best ({info['best_station']}, {info['best_sector']})")
            assert info["status"] & _lib.GM_ALIGN_AMBIGUOUS and not info["status"] & _lib.GM_ALIGN_FAILED_MASK
            assert info["distinction"] < an.DEFAULTS["min_distinction"] and wn.pose_ok(info["pose"])
        # a smooth frame against the smooth map as well
        cloud, true = drive(texture=None)[0]
        info, _tab, _, _ = m.align_points(cloud, true, outputs=False)
        assert info["status"] & _lib.GM_ALIGN_AMBIGUOUS


# ---- what it is for ----

CHECK = dict(threshold=0.03, min_count=8)
# The twin on these inputs (wall_check_np.classify on the fp64 chain of the three frames): 1 changed point under the true
# poses, 847 under the poses 3 stations off (164, 316, 367), 1 under the twin's own aligned poses.  The twin's margin over
# the true poses' count is 0; 5 points are allowed for the device's fp32 binning of points at cell edges.  "Many times":
# at least half the twin's 847, and 50 times the true poses' count.
PURPOSE_MARGIN = 5


def test_an_aligned_pose_clears_the_check(gm):
    raw = survey_raw()
    n_true = n_off = n_aligned = 0
    with gm.GeometricMapping() as c:
        m = c.wall_map(**P)
        m.add_raw(raw)
        for cloud, true in drive():
            off = moved(true, 3, 0)
            info, _tab, _, _ = m.align_points(cloud, off, outputs=False)
            assert info["status"] == _lib.GM_ALIGN_OK and info["best_station"] == 3
            changed = []
            for pose in (true, off, info["pose"]):
                i, _, _ = m.check_points(cloud, pose, outputs=False, **CHECK)
                changed.append(i["changed_pos"] + i["changed_neg"])
                assert i["unchanged"] + changed[-1] > 15_000
            print("changed under the true / the shifted / the aligned pose:", changed)
            n_true, n_off, n_aligned = n_true + changed[0], n_off + changed[1], n_aligned + changed[2]
    assert n_off >= 50 * max(n_true, 1) and n_off > 423
    assert n_aligned <= n_true + PURPOSE_MARGIN


# ---- failures ----

def test_failures(gm):
    frames = drive(5_000)
    (cloud, pose), (cloud1, pose1) = frames[0], frames[1]
    L = _lib.load()
    info = _lib.WallAlignInfo()
    got = C.c_uint32(7)
    dp = np.ascontiguousarray(pose).ctypes.data_as(C.POINTER(C.c_double))
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(5_000)) as c, gm.GeometricMapping() as other:
        m = c.wall_map(**P)
        before = _map_state(m)
        assert L.gm_wall_map_get_align(m._map, 0, C.byref(info), None, 0, C.byref(got)) == _lib.GM_ERR_NOT_READY and got.value == 0
        assert L.gm_wall_map_align_frame(m._map, c._ctx, 1, dp, None, None) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_align_frame(m._map, other._ctx, 0, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_align_frame(m._map, c._ctx, 7, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_align(m._map, 7, C.byref(info), None, 0, None) == _lib.GM_ERR_INVALID_ARG
        c.process_frame(cloud1)
        nan = pose1.copy()
        nan[1, 3] = np.nan
        for bad in (nan, pose1 * 1.01):
            with pytest.raises(gm.GmError) as e:
                m.align_frame(0, bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        for kw in (dict(half_patch_stations=0), dict(half_patch_stations=129), dict(max_station_shift=65), dict(max_sector_shift=16),
                   dict(min_count=0), dict(min_frame_count=0), dict(min_overlap=0), dict(gate=0.0), dict(gate=8.5), dict(clip=0.0),
                   dict(clip=9.0), dict(min_distinction=0.5)):
            with pytest.raises(gm.GmError) as e:
                m.align_frame(0, pose1, **kw)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG, kw
            with pytest.raises(gm.GmError) as e:
                m.align_points(cloud, pose, **kw)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG, kw
        assert L.gm_wall_map_get_align(m._map, 0, C.byref(info), None, 0, None) == _lib.GM_ERR_NOT_READY
        # an align on an empty map: the frame is binned, nothing overlaps
        add = m.align_frame(0, pose1)
        r, tab = m.align_result(0)
        assert add["anchor_station"] == r["anchor_station"] and add["gate"] == np.float32(0.25)
        assert r["n_points"] > 1000 and r["binned"] > 1000 and r["status"] == _lib.GM_ALIGN_NO_OVERLAP
        assert np.all(np.isnan(r["pose"])) and tab.shape == (17, 9) and not tab["n"].any()
        assert m.align_result(0)[0]["bytes"] == r["bytes"]                     # readable again
        # the count query, a short buffer, NULL scores with a capacity
        assert L.gm_wall_map_get_align(m._map, 0, None, None, 0, C.byref(got)) == _lib.GM_OK and got.value == 153
        buf = (_lib.WallAlignScore * 152)()
        assert L.gm_wall_map_get_align(m._map, 0, C.byref(info), buf, 152, C.byref(got)) == _lib.GM_ERR_CAPACITY
        assert L.gm_wall_map_get_align(m._map, 0, C.byref(info), None, 5, C.byref(got)) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_align(m._map, 1, C.byref(info), None, 0, None) == _lib.GM_ERR_NOT_READY
        # a frame whose n_valid is 0
        res0 = c.process_frame(np.full((100, 3), 50.0, np.float32))
        assert res0["n_valid"] == 0
        m.align_frame(0, pose1)
        r, tab = m.align_result(0)
        assert r["n_points"] == 0 and r["status"] == _lib.GM_ALIGN_NO_OVERLAP and not tab["n"].any()
        assert all(r[k] == 0 for k in an.CLASSES) and r["patch_cells_usable"] == 0
        assert _map_state(m) == before
        # a map destroyed with an align outstanding frees cleanly; so does the context with one
        c.submit_frame(1, cloud1)
        m.align_frame(1, pose1)
        m.close()
        c.wait_frame(1)
        m2 = c.wall_map(**P)
        c.submit_frame(0, cloud1)
        m2.align_frame(0, pose1)


# ---- frame path = stage path ----

N_FRAME = 20_000


@pytest.mark.parametrize("graph", (False, True))
def test_frame_path_equals_stage_path(gm, graph):
    raw = survey_raw()
    frames = drive(N_FRAME)
    clouds = [f[0] for f in frames]
    poses = [moved(f[1], 2, -1) for f in frames]
    flags = PLANE | (_lib.GM_CFG_GRAPH if graph else 0)
    wide = dict(max_station_shift=12, half_patch_stations=16)
    L = _lib.load()
    live = L.gm_debug_live_buffers()
    with gm.GeometricMapping(flags=flags, n_slots=2, neighborRadius=synth.fixed_k_radius(N_FRAME), **KW) as c:
        m = c.wall_map(**P)
        idle = c.wall_map(**P)                                # a map that never aligns
        m.add_raw(raw)
        idle.add_raw(raw)
        c.process_frame(clouds[0])
        idle.check_frame(0, poses[0])
        idle.check_result(0)
        with_adds = L.gm_debug_live_buffers()
        before = _map_state(m)
        for k in range(2):
            c.submit_frame(0, clouds[k])                      # right behind the submit
            m.align_frame(0, poses[k])
            streamed, stab = m.align_result(0)
            if k == 0:   # the align's scratch of (m, slot 0), allocated on first use: four blocks; `idle` holds none
                assert L.gm_debug_live_buffers() == with_adds + 4
            c.wait_frame(0)
            again, atab = m.align_result(0)
            assert again["bytes"] == streamed["bytes"] and atab.tobytes() == stab.tobytes()
            m.align_frame(0, poses[k])                        # after the wait
            waited, wtab = m.align_result(0)
            m.align_frame(0, poses[k], **wide)
            other, otab = m.align_result(0)
            xyz, _rows = c.cropped_cloud(0)
            lab = c.labels(0)
            assert streamed["status"] == _lib.GM_ALIGN_OK and streamed["n_points"] == len(xyz) > 10_000
            assert (streamed["best_station"], streamed["best_sector"]) == (2, -1)
            assert streamed["plane"] == int((lab == 1).sum())
            staged, ttab, _, _ = m.align_points(xyz, poses[k], labels=lab, outputs=False)
            assert staged["bytes"] == streamed["bytes"] == waited["bytes"], k
            assert ttab.tobytes() == stab.tobytes() == wtab.tobytes(), k
            staged, ttab, _, _ = m.align_points(xyz, poses[k], labels=lab, outputs=False, **wide)
            assert staged["bytes"] == other["bytes"] != streamed["bytes"], k
            assert ttab.tobytes() == otab.tobytes() and otab.shape == (25, 9), k
            if k == 0:
                kept = L.gm_debug_live_buffers()
        assert L.gm_debug_live_buffers() == kept              # grow-only: the second frame's aligns allocate nothing
        assert _map_state(m) == before and _map_state(idle) == before
        idle.close()
        m.close()
        assert L.gm_debug_live_buffers() < with_adds
    assert L.gm_debug_live_buffers() == live


def test_ordering_across_slots(gm):
    """An add enqueued on slot 1 before the align on slot 0 is seen; one enqueued after it is not."""
    (cloud0, pose0), (cloud1, pose1), _ = drive(N_FRAME)              # (3.5 m apart: the frames overlap)
    pin = moved(pose0, 1, 1)
    ak = dict(min_count=1, min_overlap=16)
    kw = dict(n_slots=2, neighborRadius=synth.fixed_k_radius(N_FRAME))
    with gm.GeometricMapping(**kw) as c:
        held = c.wall_map(**P)                                        # a map that already holds frame 1
        c.process_frame(cloud1)
        held.add_frame(0, pose1)
        held.sync()
        c.process_frame(cloud0)
        held.align_frame(0, pin, **ak)
        want, wtab = held.align_result(0)
        assert not want["status"] & _lib.GM_ALIGN_FAILED_MASK and want["overlap"] > 100
        assert (want["best_station"], want["best_sector"]) == (1, 1)
        m = c.wall_map(**P)                                           # an empty map, nothing waited for in between
        c.submit_frame(1, cloud1)
        m.add_frame(1, pose1)
        c.submit_frame(0, cloud0)
        m.align_frame(0, pin, **ak)
        c.wait_frame(1)
        c.submit_frame(1, cloud0)
        m.add_frame(1, pose0)                                         # enqueued after the align: not seen
        got, gtab = m.align_result(0)
        c.wait_frame(0)
        c.wait_frame(1)
        m.sync()
        assert got["bytes"] == want["bytes"] and gtab.tobytes() == wtab.tobytes()
        assert m.info()["frames"] == 2
