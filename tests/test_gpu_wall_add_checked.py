"""GPU tests of the add less the check's changed rows (gm_wall_map_add_*_checked, csrc/k_wall_add_checked.hip, the masked
instantiation of k_wall_add, gm_wall_add_checked.hip).  The defining property everywhere: the map's raw cells and totals
after a checked add are, byte for byte, those of gm_wall_map_add_points of the cloud with the twin's skipped indices
(tests/wall_add_checked_np.py) deleted; the call's counts are the twin's.  Sizes and mask-word edges, none / all selected,
the selection parameters, stale mask bits, the frame path against the stage path over every pipeline path, the ordering
against a check on another slot, readiness and failures, independence of the chainage."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_add_checked_np as an  # noqa: E402
import wall_check_np as kn  # noqa: E402
import wall_np as wn  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = dict(n_stations=160, n_sectors=90)
ROW_KEYS = an.ROW_NAMES
POINT_KEYS = ("skipped", "plane", "beyond_gate", "outside", "mapped")


def _map_state(m):
    i = m.info()
    return m.read_raw().tobytes(), tuple(i[k] for k in ("frames", "mapped", "outside", "beyond_gate", "plane", "cells_hit"))


def _copy(c, p, raw):
    m = c.wall_map(**p)
    m.add_raw(raw)
    return m


def _sum_rules(info):
    assert sum(info[k] for k in ROW_KEYS) == info["n_rows"]
    assert sum(info[k] for k in POINT_KEYS) == info["n_points"]


def _same_info(info, want):
    for k in want:
        assert info[k] == want[k], (k, info[k], want[k])
    _sum_rules(info)


def _survey(c, p, frames):
    m = c.wall_map(**p)
    for cloud, pose in frames:
        m.add_points(cloud, pose, outputs=False)
    return m


def _checked_vs_plain(c, p, raw, scratch, xyz, pose, lab, rows, **prm):
    """One add_points_checked on a copy of the map against the filtered plain add on another copy: bytes, totals, the
    counts and the per-point outputs.  Returns (info, row classes, skipped indices, the checked copy's raw bytes)."""
    n = len(xyz)
    a, b = _copy(c, p, raw), _copy(c, p, raw)
    info, res, cell = a.add_points_checked(xyz, pose, rows, labels=lab, **prm)
    cls, skipped = an.select(rows, n, **prm)
    keep = an.keep(n, skipped)
    ainfo, e, cl = b.add_points(xyz[keep], pose, labels=None if lab is None else lab[keep])
    state = _map_state(a)
    assert state == _map_state(b)
    # the counts: the twin on the plain add's own per-point pairs, put back at their indices
    e_full, cell_full = np.full(n, np.nan, np.float32), np.full(n, -1, np.int64)
    e_full[keep], cell_full[keep] = e, cl
    want = an.info(rows, e_full, cell_full, p["gate"], labels=lab, status=ainfo["status"], **prm)
    _same_info(info, want)
    for f in ("o", "a", "u", "v", "R", "station_length", "sector_angle", "gate"):
        assert np.array_equal(np.asarray(info["add"][f]).view(np.uint32), np.asarray(ainfo[f]).view(np.uint32)), f
    # the per-point outputs: the plain add's for the points that stay; e of the add's chain and -1 for a skipped one
    _, e_all, _ = scratch.add_points(xyz, pose, labels=lab)
    assert np.array_equal(res.view(np.uint32), e_all.view(np.uint32))
    assert np.array_equal(cell[keep], cl) and np.all(cell[~keep] == -1)
    a.close()
    b.close()
    return info, cls, skipped, state[0]


SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8193, 20_000)


def test_sizes_and_mask_edges_byte_for_byte(gm):
    survey = synth.tunnel_drive(4, 20_000, seed=3, patches=())
    drive = synth.tunnel_drive(4, 20_000, seed=3)          # the same poses; the wall moved inside the patches
    p = wn.params(**dict(drive["design"], **GRID))
    ck = dict(threshold=0.004, min_count=2)                # 0.4 sigma: about two points in three are rows, of both signs
    tot = dict(neg=0, pos=0, kept=0, skipped=0, both_ends=0)
    with gm.GeometricMapping() as c:
        m = _survey(c, p, survey["frames"])
        raw = m.read_raw()
        before = _map_state(m)
        scratch = c.wall_map(**p)
        for k, n in enumerate(SIZES):
            cloud, pose = drive["frames"][k % 4]
            xyz = cloud[:n]
            lab = (np.arange(n) % 7 == 0).astype(np.uint8)
            _, rows, _ = m.check_points(xyz, pose, labels=lab, outputs=False, **ck)
            for prm in (dict(), dict(min_delta=0.012)):    # every row selected; the rows below 1.2 sigma kept
                info, cls, skipped, _ = _checked_vs_plain(c, p, raw, scratch, xyz, pose, lab, rows, **prm)
                print(f"n={n} {prm}: " + " ".join(f"{k_}={info[k_]}" for k_ in ROW_KEYS + POINT_KEYS))
                assert info["n_points"] == n and info["n_rows"] == len(rows) and info["rows_rejected"] == 0
                tot["neg"] += info["rows_neg"]
                tot["pos"] += info["rows_pos"]
                tot["kept"] += info["rows_kept"]
                tot["skipped"] += info["skipped"]
                if n > 1 and len(skipped) and skipped[0] == 1 and skipped[-1] == n - 1:
                    tot["both_ends"] += 1
            # Index 0 carries label 1 under these labels, and a check never lists a plane point: its own rows reach index
            # 1 and n - 1 at most.  So the same rows once more with hand-made ones behind them (any order, duplicates
            # allowed) that name both ends of every mask word the size has, and index n, which is rejected
            ends = np.array(sorted({i for i in (0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, n - 2, n - 1) if 0 <= i < n} | {n}), np.uint32)
            extra = np.zeros(len(ends), kn.POINT)
            extra["index"], extra["delta"] = ends, np.where(ends % 2 == 0, 1.0, -1.0)
            info, cls, skipped, _ = _checked_vs_plain(c, p, raw, scratch, xyz, pose, lab, np.concatenate([rows, extra]))
            assert info["rows_rejected"] == 1 and set(ends[:-1].tolist()) <= set(skipped.tolist())
            assert info["plane"] == int(lab.sum()) - int(lab[skipped].sum())   # a skipped plane point is skipped, not plane
        print(tot)
        # without these the test proves nothing
        assert tot["neg"] > 0 and tot["pos"] > 0 and tot["kept"] > 0 and tot["skipped"] > 100 and tot["both_ends"] > 0
        assert _map_state(m) == before                     # the checked map itself was only read


def test_none_and_all(gm):
    n = 10_000
    survey = synth.tunnel_drive(4, 20_000, seed=8, radius=2.05, patches=())
    drive = synth.tunnel_drive(4, n, seed=9, patches=())
    p = wn.params(**dict(drive["design"], n_stations=160, radius=2.0))
    with gm.GeometricMapping() as c:
        m = _survey(c, p, survey["frames"])                # the surveyed wall lies 0.05 m outside the design
        raw = m.read_raw()
        scratch = c.wall_map(**p)
        cloud, pose = drive["frames"][1]
        # none: no rows, the plain add's bytes, nothing of the mark in the counters
        i0, rows, _ = m.check_points(cloud, pose, threshold=8.0, gate=8.0, outputs=False)
        assert len(rows) == 0
        info, _, skipped, got = _checked_vs_plain(c, p, raw, scratch, cloud, pose, None, rows)
        assert info["skipped"] == 0 and len(skipped) == 0 and info["n_rows"] == 0 and all(info[k] == 0 for k in ROW_KEYS)
        plain = _copy(c, p, raw)
        plain.add_points(cloud, pose, outputs=False)
        assert plain.read_raw().tobytes() == got
        # all: every usable point is a row and is skipped; the usable cells keep their bytes
        i1, rows, out = m.check_points(cloud, pose, threshold=2.0 ** -20, min_count=1)
        usable = n - i1["plane"] - i1["beyond_gate"] - i1["outside"] - i1["unsurveyed"]
        assert usable > 2 * 4096 and len(rows) == usable
        info, _, skipped, got = _checked_vs_plain(c, p, raw, scratch, cloud, pose, None, rows)
        assert info["skipped"] == usable == len(skipped) and info["rows_kept"] == 0
        after = np.frombuffer(got, wn.RAW_CELL).reshape(raw.shape)
        surveyed = raw["count"] > 0
        assert after[surveyed].tobytes() == raw[surveyed].tobytes()
        assert info["mapped"] == int(after["count"][~surveyed].sum()) == i1["unsurveyed"]


def test_selection(gm):
    survey = synth.tunnel_drive(4, 20_000, seed=3, patches=())
    drive = synth.tunnel_drive(4, 20_000, seed=3)
    p = wn.params(**dict(drive["design"], **GRID))
    with gm.GeometricMapping() as c:
        m = _survey(c, p, survey["frames"])
        raw = m.read_raw()
        scratch = c.wall_map(**p)
        cloud, pose = drive["frames"][1]
        xyz = cloud[:8193]
        _, rows, _ = m.check_points(xyz, pose, threshold=0.015, min_count=2, outputs=False)
        neg, pos = int((rows["delta"] < 0).sum()), int((rows["delta"] > 0).sum())
        assert neg > 50 and pos > 50
        states = {}
        for skip in (1, 2, 3):
            info, cls, skipped, states[skip] = _checked_vs_plain(c, p, raw, scratch, xyz, pose, None, rows, skip=skip)
            assert info["rows_neg"] == (neg if skip & 1 else 0) and info["rows_pos"] == (pos if skip & 2 else 0)
            assert info["rows_kept"] == len(rows) - info["rows_neg"] - info["rows_pos"]
        assert len(set(states.values())) == 3
        # min_delta at one row's |delta| exactly: S == |dq|, the row is selected; one unit of 2^-20 above it, the row is kept
        r = int(np.argsort(np.abs(rows["delta"]))[len(rows) // 2])
        d = np.abs(rows["delta"][r])
        dq = int(abs(kn.fix(rows["delta"][r:r + 1])[0]))
        assert float(d) * 2.0 ** 20 == dq                  # exact for a check's row
        info, cls, skipped, _ = _checked_vs_plain(c, p, raw, scratch, xyz, pose, None, rows, min_delta=float(d))
        assert info["min_delta_q"] == dq and cls[r] <= an.POS and rows["index"][r] in skipped
        info, cls, skipped, _ = _checked_vs_plain(c, p, raw, scratch, xyz, pose, None, rows, min_delta=(dq + 1) * 2.0 ** -20)
        assert info["min_delta_q"] == dq + 1 and cls[r] == an.KEPT and rows["index"][r] not in skipped
        # the next fp32 above |delta|: S = rint(min_delta 2^20) by the rule, whatever that is for this delta (an fp32 ulp
        # is below 2^-20 for every |delta| < 8, so S stays |dq| and the row stays selected): the twin decides
        up = float(np.nextafter(d, np.float32(np.inf)))
        info, cls, skipped, _ = _checked_vs_plain(c, p, raw, scratch, xyz, pose, None, rows, min_delta=up)
        assert info["min_delta_q"] == an.min_delta_q(up) and (cls[r] == an.KEPT) == (an.min_delta_q(up) > dq)


def test_stale_bits(gm):
    """Many selected rows, then few at other indices, through the same mask: the stage call's and one slot's."""
    n = 12_000
    survey = synth.tunnel_drive(6, 20_000, seed=5, patches=())
    drive = synth.tunnel_drive(6, n, seed=5)
    p = wn.params(**dict(drive["design"], **GRID))
    many, few = dict(threshold=0.004, min_count=2), dict(threshold=0.03, min_count=2)   # 0.4 and 3 sigma
    kw = dict(neighborRadius=synth.fixed_k_radius(n))
    with gm.GeometricMapping(**kw) as c:
        m = _survey(c, p, survey["frames"])
        raw = m.read_raw()
        a, b = _copy(c, p, raw), _copy(c, p, raw)
        # the stage call
        counts = []
        for (cloud, pose), ck in ((drive["frames"][1], many), (drive["frames"][4], few)):
            _, rows, _ = m.check_points(cloud, pose, outputs=False, **ck)
            info, _, _ = a.add_points_checked(cloud, pose, rows, outputs=False)
            _, skipped = an.select(rows, n)
            assert info["skipped"] == len(skipped) == len(rows)
            b.add_points(cloud[an.keep(n, skipped)], pose, outputs=False)
            counts.append(info["skipped"])
        assert counts[0] > 5000 and 0 < counts[1] < 500
        assert _map_state(a) == _map_state(b)
        # one slot of the frame path: the checks run against the map the adds go into
        f, g = _copy(c, p, raw), _copy(c, p, raw)
        seen = []
        for (cloud, pose), ck in ((drive["frames"][1], many), (drive["frames"][4], few)):
            c.process_frame(cloud)
            f.check_frame(0, pose, **ck)
            f.add_frame_checked(0, pose)
            xyz, _ = c.cropped_cloud()
            seen.append((xyz, pose, f.check_result(0)[1], f.add_checked_result(0)))
        f.sync()
        for xyz, pose, rows, info in seen:
            _, skipped = an.select(rows, len(xyz))
            assert info["skipped"] == len(skipped) == len(rows) and info["n_points"] == len(xyz)
            g.add_points(xyz[an.keep(len(xyz), skipped)], pose, outputs=False)
        assert len(seen[0][2]) > 5000 and 0 < len(seen[1][2]) < 500
        assert _map_state(f) == _map_state(g)


# ---- frame path = stage path ----

N_FRAME = 20_000
CK = dict(threshold=0.02, min_count=4)
AC = dict(min_delta=0.03)
PLANE = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE
RANSAC = dict(ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=7)


def _collect(c, m, slot, flags):
    xyz, _ = c.cropped_cloud(slot)
    lab = c.labels(slot) if flags & _lib.GM_CFG_RANSAC_PLANE else None
    return xyz, lab, m.check_result(slot)[1], m.add_checked_result(slot)


def _replay(gm, p, baseline, seen, poses):
    """The stage path on what the frame path saw: per frame the info, and the final map."""
    infos = []
    with gm.GeometricMapping() as c:
        m = _copy(c, p, baseline)
        for (xyz, lab, rows, _), pose in zip(seen, poses):
            info, _, _ = m.add_points_checked(xyz, pose, rows, labels=lab, outputs=False, **AC)
            info.pop("add")
            infos.append(info)
        return infos, _map_state(m)


def test_frame_path_equals_stage_path(gm):
    survey = synth.tunnel_drive(8, N_FRAME, seed=31, patches=())
    drive = synth.tunnel_drive(8, N_FRAME, seed=31)
    clouds, poses = [f[0] for f in drive["frames"]], [f[1] for f in drive["frames"]]
    p = wn.params(n_stations=192, **drive["design"])
    with gm.GeometricMapping() as c:
        baseline = _survey(c, p, survey["frames"]).read_raw()
    kw = dict(neighborRadius=synth.fixed_k_radius(N_FRAME))

    def blocking(flags, n, kw_):
        seen = []
        with gm.GeometricMapping(flags=flags, **kw_) as c:
            m = _copy(c, p, baseline)
            for k in range(n):
                c.process_frame(clouds[k])
                m.check_frame(0, poses[k], **CK)
                m.add_frame_checked(0, poses[k], **AC)
                seen.append(_collect(c, m, 0, flags))
            return seen, _map_state(m)

    def compare(seen, state, n):
        infos, want = _replay(gm, p, baseline, seen, poses[:n])
        for k, ((_, _, rows, info), w) in enumerate(zip(seen, infos)):
            assert info == w, (k, info, w)
            _sum_rules(info)
            assert info["n_rows"] == len(rows)
        assert state == want
        return infos

    seen, part = blocking(_lib.GM_CFG_DEFAULT, 4, kw)
    infos = compare(seen, part, 4)
    assert sum(i["skipped"] for i in infos) > 100 and sum(i["rows_kept"] for i in infos) > 100
    gseen, gpart = blocking(_lib.GM_CFG_DEFAULT | _lib.GM_CFG_GRAPH, 4, kw)
    compare(gseen, gpart, 4)
    assert gpart == part
    # the plane RANSAC's labels
    pseen, ppart = blocking(PLANE, 3, dict(kw, **RANSAC))
    pinfos = compare(pseen, ppart, 3)
    assert all(i["plane"] > 0 for i in pinfos)
    # four streaming slots, check and checked add right behind each submit, slots reused, no sync until the end: adds from
    # several streams interleave in the map.  The checks see other maps' states than the blocking run's, so the reference is
    # the stage path replayed on these rows; two runs of it agree with each other as well
    finals = []
    for _ in range(2):
        with gm.GeometricMapping(n_slots=4, **kw) as c:
            m = _copy(c, p, baseline)
            sseen = []
            for k in range(8):
                if k >= 4:
                    c.wait_frame(k % 4)
                    sseen.append(_collect(c, m, k % 4, 0))         # frame k - 4's, before the slot's next calls replace them
                c.submit_frame(k % 4, clouds[k])
                m.check_frame(k % 4, poses[k], **CK)
                m.add_frame_checked(k % 4, poses[k], **AC)
            for k in range(4, 8):
                c.wait_frame(k % 4)
                sseen.append(_collect(c, m, k % 4, 0))
            m.sync()
            state = _map_state(m)
        compare(sseen, state, 8)
        finals.append((state, [s[2].tobytes() for s in sseen]))
    assert finals[0] == finals[1]
    # a check sees every earlier frame's checked add: the first four frames' rows are the blocking run's
    assert [s[2].tobytes() for s in sseen[:4]] == [s[2].tobytes() for s in seen]


def test_ordering_against_a_check_on_another_slot(gm):
    n = 12_000
    survey = synth.tunnel_drive(4, 20_000, seed=13, patches=())
    drive = synth.tunnel_drive(4, n, seed=13, step=1.0)   # neighbouring frames overlap almost wholly
    p = wn.params(**dict(drive["design"], **GRID))
    (ca, pa), (cb, pb) = drive["frames"][1], drive["frames"][2]
    ck = dict(threshold=0.02, min_count=2, reference=kn.ENVELOPE)
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(n)) as c:
        baseline = _survey(c, p, survey["frames"][:1]).read_raw()  # a thin survey: the add of A widens many envelopes
        m = _copy(c, p, baseline)
        c.submit_frame(0, ca)
        m.check_frame(0, pa, **ck)
        m.add_frame_checked(0, pa)
        c.submit_frame(1, cb)
        m.check_frame(1, pb, **ck)
        c.wait_frame(0)
        c.wait_frame(1)
        xa, _ = c.cropped_cloud(0)
        xb, padb = c.cropped_cloud(1)
        rows_a, (info_b, rows_b) = m.check_result(0)[1], m.check_result(1)
        ainfo = m.add_checked_result(0)
        m.sync()
        # the map the check on B must have seen: the filtered plain add of A, and nothing of the skipped points
        _, skipped = an.select(rows_a, len(xa))
        assert ainfo["skipped"] == len(skipped) > 100
        ref = _copy(c, p, baseline)
        ref.add_points(xa[an.keep(len(xa), skipped)], pa, outputs=False)
        assert _map_state(m)[0] == _map_state(ref)[0]
        winfo, wrows, _ = ref.check_points(xb, pb, outputs=False, **ck)
        wrows["row"] = padb.view(np.uint32)[wrows["index"]]
        winfo.pop("add")
        assert info_b == winfo and rows_b.tobytes() == wrows.tobytes()
        # and it differs from what a check sees before A's add and after a plain add of all of A
        early = _copy(c, p, baseline)
        full = _copy(c, p, baseline)
        full.add_points(xa, pa, outputs=False)
        for other in (early, full):
            assert not np.array_equal(other.check_points(xb, pb, outputs=False, **ck)[1]["delta"], wrows["delta"])


def test_readiness_and_failures(gm):
    drive = synth.tunnel_drive(3, 5_000, seed=2)
    (cloud, pose), (cloud1, pose1), (cloud2, pose2) = drive["frames"]
    big = synth.tunnel_drive(2, 20_000, seed=4)["frames"][1][0]
    p = wn.params(n_stations=80, **drive["design"])
    L = _lib.load()
    info = _lib.WallAddCheckedInfo()
    dp = np.ascontiguousarray(pose1).ctypes.data_as(C.POINTER(C.c_double))
    with gm.GeometricMapping(n_slots=2, neighborRadius=synth.fixed_k_radius(5_000)) as c, gm.GeometricMapping() as other:
        m = c.wall_map(**p)
        m2 = c.wall_map(**p)
        m.add_points(cloud, pose, outputs=False)
        m2.add_points(cloud, pose, outputs=False)
        # before any call; NULL info; a bad slot
        assert L.gm_wall_map_get_add_checked(m._map, 0, C.byref(info)) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_get_add_checked(m._map, 0, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_get_add_checked(m._map, 7, C.byref(info)) == _lib.GM_ERR_INVALID_ARG
        # a slot without a frame; the wrong context; a bad slot
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 1, dp, None, None) == _lib.GM_ERR_NOT_READY
        assert L.gm_wall_map_add_frame_checked(m._map, other._ctx, 0, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 7, dp, None, None) == _lib.GM_ERR_INVALID_ARG
        c.process_frame(cloud1)
        # a frame, no check on (map, slot): none at all, then one on another map only
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 0, dp, None, None) == _lib.GM_ERR_NOT_READY
        m2.check_frame(0, pose1, threshold=0.03, min_count=1)
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 0, dp, None, None) == _lib.GM_ERR_NOT_READY
        m.check_frame(0, pose1, threshold=0.03, min_count=1)
        # a bad pose; bad params
        nan = pose1.copy()
        nan[1, 3] = np.nan
        for bad in (nan, pose1 * 1.01):
            with pytest.raises(gm.GmError) as e:
                m.add_frame_checked(0, bad)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        for prm in (dict(skip=0), dict(skip=4), dict(min_delta=-1.0), dict(min_delta=8.5), dict(min_delta=float("nan"))):
            with pytest.raises(gm.GmError) as e:
                m.add_frame_checked(0, pose1, **prm)
            assert e.value.status == _lib.GM_ERR_INVALID_ARG
        before = _map_state(m)
        assert before[1][0] == 1 and L.gm_wall_map_get_add_checked(m._map, 0, C.byref(info)) == _lib.GM_ERR_NOT_READY
        # the call; the check stays readable, with the same bytes; the pose need not be the check's
        i1, r1 = m.check_result(0)
        m.add_frame_checked(0, pose1)
        got = m.add_checked_result(0)
        assert got == m.add_checked_result(0) and got["n_rows"] == len(r1) > 1 and got["skipped"] == len(r1)
        assert info.struct_size == 0 and L.gm_wall_map_get_add_checked(m._map, 0, C.byref(info)) == _lib.GM_OK
        assert info.struct_size == C.sizeof(_lib.WallAddCheckedInfo) and info.reserved == 0
        i1b, r1b = m.check_result(0)
        assert i1b == i1 and r1b.tobytes() == r1.tobytes()
        moved = pose1.copy()
        moved[0, 3] += 0.5
        m.add_frame_checked(0, moved)                              # the same check again, another pose
        assert m.add_checked_result(0)["skipped"] == len(r1) and m.info()["frames"] == 3
        assert L.gm_wall_map_get_add_checked(m._map, 1, C.byref(info)) == _lib.GM_ERR_NOT_READY
        # a second submit to the slot since the check: refused, not applied to another cloud's indices
        c.process_frame(cloud2)
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 0, dp, None, None) == _lib.GM_ERR_NOT_READY
        assert m.add_checked_result(0)["skipped"] == len(r1)       # the last call's counts stay readable
        # a slot reused by a stage call holds no frame
        m.check_frame(0, pose2)
        m.add_points(cloud, pose, outputs=False)
        assert L.gm_wall_map_add_frame_checked(m._map, c._ctx, 0, dp, None, None) == _lib.GM_ERR_NOT_READY
        # the stage call: NULL rows with a count, bad params; it leaves slot 0's stored check alone
        c.process_frame(cloud2)
        m.check_frame(0, pose2, threshold=0.03, min_count=1)
        i2, r2 = m.check_result(0)
        xyz2, _ = c.cropped_cloud()
        xp = np.ascontiguousarray(cloud).ctypes.data_as(C.POINTER(C.c_float))
        assert L.gm_wall_map_add_points_checked(m._map, xp, 10, None, dp, None, None, 3, None, None, None, None) == _lib.GM_ERR_INVALID_ARG
        with pytest.raises(gm.GmError) as e:
            m2.add_points_checked(cloud, pose, r2[:0], skip=0)
        assert e.value.status == _lib.GM_ERR_INVALID_ARG
        other_rows = np.zeros(3, kn.POINT)
        other_rows["delta"], other_rows["index"] = 1.0, (0, 1, 2)
        assert m2.add_points_checked(cloud, pose, other_rows, outputs=False)[0]["skipped"] == 3
        i2b, r2b = m.check_result(0)
        assert i2b == i2 and r2b.tobytes() == r2.tobytes()
        # a regrow of the check's staging right behind a checked add: a larger frame on the same slot, nothing waited for
        c.process_frame(cloud2)
        m.check_frame(0, pose2, threshold=0.03, min_count=1)
        state = m.read_raw()
        ra = m.check_result(0)[1]
        m.add_frame_checked(0, pose2)
        c.submit_frame(0, big)
        m.check_frame(0, pose2, threshold=0.03, min_count=1)       # frees and regrows the rows the mark reads
        m.add_frame_checked(0, pose2)
        c.wait_frame(0)
        xb, _ = c.cropped_cloud(0)
        rb, ib = m.check_result(0)[1], m.add_checked_result(0)
        m.sync()
        ref = _copy(c, p, state)
        _, ska = an.select(ra, len(xyz2))
        assert len(ska) == len(ra) > 1
        ref.add_points(xyz2[an.keep(len(xyz2), ska)], pose2, outputs=False)
        assert ib["n_points"] == len(xb) > 10_000 and ib["skipped"] == len(rb)
        _, skb = an.select(rb, len(xb))
        ref.add_points(xb[an.keep(len(xb), skb)], pose2, outputs=False)
        assert m.read_raw().tobytes() == ref.read_raw().tobytes()
        # a frame whose n_valid is 0
        res = c.process_frame(np.full((100, 3), 50.0, np.float32))
        assert res["n_valid"] == 0
        m.check_frame(0, pose1)
        m.add_frame_checked(0, pose1)
        i0 = m.add_checked_result(0)
        assert i0["n_points"] == 0 and i0["n_rows"] == 0 and sum(i0[k] for k in ROW_KEYS + POINT_KEYS) == 0
        # a map destroyed with a checked add outstanding frees cleanly; so does the context with one
        c.submit_frame(1, cloud1)
        m.check_frame(1, pose1)
        m.add_frame_checked(1, pose1)
        m.close()
        c.wait_frame(1)
        c.submit_frame(0, cloud1)
        m2.check_frame(0, pose1)
        m2.add_frame_checked(0, pose1)


def _wall_seen_from(p, pose, n, seed, dr=0.0):
    rng = np.random.default_rng(seed)
    D = wn.design_frame(p)
    s = (pose[:, 3] - D["o"]) @ D["a"]
    t, phi = rng.uniform(s - 6.0, s + 6.0, n), rng.uniform(0.0, 2 * np.pi, n)
    rr = D["R"] + dr * (phi < 1.0) + rng.normal(0.0, 0.01, n)
    world = D["o"] + t[:, None] * D["a"] + (rr * np.cos(phi))[:, None] * D["u"] + (rr * np.sin(phi))[:, None] * D["v"]
    cloud = ((world - pose[:, 3]) @ pose[:, :3]).astype(np.float32)
    return np.ascontiguousarray(cloud[np.all(np.abs(cloud) <= 5.0, axis=1)])


def test_chainage(gm):
    shift = 20000
    p, p0, p1 = wn.chainage_pair(shift)
    survey = _wall_seen_from(p, p0, 60_000, seed=41)
    cloud = _wall_seen_from(p, p0, 20_000, seed=42, dr=0.1)     # a sixth of the ring moved out by 0.1 m
    with gm.GeometricMapping() as c:
        m = c.wall_map(**p)
        _, _, cell = m.add_points(survey, p0)
        _, _, ccell = c.wall_map(**p).add_points(cloud, p0)
        cells = np.concatenate([cell[cell >= 0], ccell[ccell >= 0]])
        j0 = int(cells.min()) // 90
        n = int(cells.max()) // 90 - j0 + 1
        m.add_raw(m.read_raw(j0, n), station0=j0 + shift)       # the same cells, 20 000 stations on
        _, r0, _ = m.check_points(cloud, p0, min_count=4, threshold=0.015, outputs=False)
        _, r1, _ = m.check_points(cloud, p1, min_count=4, threshold=0.015, outputs=False)
        assert len(r0) == len(r1) > 2000
        i0, e0, c0 = m.add_points_checked(cloud, p0, r0, min_delta=0.05)
        i1, e1, c1 = m.add_points_checked(cloud, p1, r1, min_delta=0.05)
        assert i1.pop("add")["anchor_station"] - i0.pop("add")["anchor_station"] == shift
        assert i0 == i1 and i0["skipped"] > 1000 and i0["rows_kept"] > 500 and i0["mapped"] > 5000
        _sum_rules(i0)
        assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
        assert np.array_equal(np.where(c0 >= 0, c0.astype(np.int64) + shift * 90, -1), c1)
        assert m.read_raw(j0, n).tobytes() == m.read_raw(j0 + shift, n).tobytes()
