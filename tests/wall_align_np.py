"""Twin of the wall-map align (gm_wall_map_align_*, csrc/k_wall_align.hip + gm_wall_slot.hip; include/gm_hip.h states the rule).

Everything from a point's residual on is integer, so this twin is exact: patch_from() bins the device's own per-point
(e, cell) pairs as wall_np.cells_from does for the add, values() and table() are the integer rule in numpy int64 (every
intermediate stays below 2^60), select() is the host rule with the 128-bit comparison in Python integers and the rest in
fp64, compose() the pose.  points() is the per-point chain in fp64 on the frame the device REPORTED, with wall_np.points'
ambiguity mask (a bin coordinate within 1e-3 of an edge, |e| within 1e-5 m of the gate).
"""
import numpy as np

import wall_np as wn

OK, NO_OVERLAP, FAILED_MASK, AMBIGUOUS, AT_BORDER = 0, 2, 0xFF, 1 << 8, 1 << 9
MAX_PATCH_CELLS, MAX_SHIFT, MAX_SHIFTS = 8192, 64, 4096
NONE = -2 ** 31            # the value of an unusable cell
SAT = 2 ** 30              # |m| saturates here
CLASSES = ("plane", "beyond_gate", "outside_patch", "binned")
SCORE = np.dtype([("ssd", "<u8"), ("sum_d", "<i8"), ("n", "<u4"), ("reserved", "<u4")])
DEFAULTS = dict(half_patch_stations=20, max_station_shift=8, max_sector_shift=4, min_count=8, min_frame_count=4,
                min_overlap=64, gate=0.25, clip=0.05, min_distinction=1.5)


def prm(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_ok(ap, n_sectors):
    """gm_wall_align_check_params' rule."""
    P, A, B = ap["half_patch_stations"], ap["max_station_shift"], ap["max_sector_shift"]
    return bool(1 <= n_sectors <= 4096 and P >= 1 and 2 * P * n_sectors <= MAX_PATCH_CELLS and 0 <= A <= MAX_SHIFT
                and 0 <= B <= MAX_SHIFT and 2 * B + 1 <= n_sectors and (2 * A + 1) * (2 * B + 1) <= MAX_SHIFTS
                and ap["min_count"] >= 1 and ap["min_frame_count"] >= 1 and ap["min_overlap"] >= 1
                and 0.0 < ap["gate"] <= 8.0 and 0.0 < ap["clip"] <= 8.0 and np.rint(ap["clip"] * 2.0 ** 20) >= 1
                and ap["min_distinction"] >= 1.0 and np.isfinite(ap["min_distinction"]))


def fix(e):
    """(int64) rint(e 2^20) of fp32 residuals, the integer the add sums."""
    return np.rint(np.asarray(e, np.float32) * np.float32(2.0 ** 20)).astype(np.int64)


def patch_from(e, cell, n_cells):
    """(sum int64 [n_cells], count int64 [n_cells]) of the per-point (e fp32, patch cell or -1) pairs."""
    cell = np.asarray(cell, np.int64)
    m = cell >= 0
    s = np.zeros(n_cells, np.int64)
    np.add.at(s, cell[m], fix(np.asarray(e, np.float32)[m]))
    return s, np.bincount(cell[m], minlength=n_cells).astype(np.int64)


def _div(s, c):
    """sum / (int64) count by C integer division (toward zero); 0 where count is 0."""
    s = np.asarray(s, np.int64)
    c = np.maximum(np.asarray(c, np.int64), 1)
    return np.sign(s) * (np.abs(s) // c)


def values(s, c, least, saturate=False):
    """The int64 image of (sum, count): sum / count where count >= least, else NONE."""
    v = _div(s, c)
    if saturate:
        v = np.clip(v, -SAT, SAT)
    return np.where(np.asarray(c, np.int64) >= least, v, NONE)


def map_image(raw, anchor, n_sectors, P, A, min_count):
    """The map's value image of stations [anchor - P - A, anchor + P + A): (2P + 2A, n_sectors) int64, NONE outside the
    map and where a cell is not usable.  raw: RAW_CELL (n_stations, n_sectors), gm_wall_map_read_raw's."""
    raw = np.asarray(raw).reshape(-1, n_sectors)
    nst = raw.shape[0]
    out = np.full((2 * P + 2 * A, n_sectors), NONE, np.int64)
    j = anchor - P - A + np.arange(2 * P + 2 * A, dtype=object)      # (an anchor near 4e18 must not wrap)
    inside = np.array([0 <= int(x) < nst for x in j], bool)
    rows = np.array([int(x) for x in j[inside]], np.int64)
    out[inside] = values(raw["sum"][rows], raw["count"][rows], min_count, saturate=True)
    return out


def table(psum, pcnt, raw, anchor, n_sectors, ap):
    """The score table, SCORE shaped (2A + 1, 2B + 1), of a patch (sum, count [2P n_sectors]) against raw map cells."""
    P, A, B = ap["half_patch_stations"], ap["max_station_shift"], ap["max_sector_shift"]
    C = int(np.rint(ap["clip"] * 2.0 ** 20))
    f = values(psum, pcnt, ap["min_frame_count"]).reshape(2 * P, n_sectors)
    m = map_image(raw, anchor, n_sectors, P, A, ap["min_count"])
    out = np.zeros((2 * A + 1, 2 * B + 1), SCORE)
    fu = f != NONE
    for ia in range(2 * A + 1):
        rows = m[ia:ia + 2 * P]                                      # patch row jr against image row jr + a + A
        for ib in range(2 * B + 1):
            mb = np.roll(rows, -(ib - B), axis=1)                    # mb[:, k] = rows[:, (k + b) mod n_sectors]
            ok = fu & (mb != NONE)
            d = np.clip(np.where(ok, f - mb, 0), -C, C)
            out[ia, ib] = (int((d * d).sum()), int(d.sum()), int(ok.sum()), 0)
    return out


def compose(design, pose, shift_m, roll):
    """Rm' = Q Rm, tr' = o + Q (tr - o) + shift_m a, Q the rotation by `roll` about the design axis (Rodrigues)."""
    m = np.asarray(pose, np.float64)[:3]
    a, o = design["a"], design["o"]
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    Q = np.cos(roll) * np.eye(3) + np.sin(roll) * K + (1.0 - np.cos(roll)) * np.outer(a, a)
    return np.concatenate([Q @ m[:, :3], (o + Q @ (m[:, 3] - o) + shift_m * a).reshape(3, 1)], axis=1)


def select(tab, p, pose, ap):
    """The host rule on a SCORE table: dict(status, anchor_station, overlap, best_station, best_sector, frac_station,
    frac_sector, shift_m, roll, bias_m, rms_best, rms_runner, distinction, pose (3, 4))."""
    A, B = ap["max_station_shift"], ap["max_sector_shift"]
    nb = 2 * B + 1
    t = np.asarray(tab, SCORE).reshape(-1)
    assert len(t) == (2 * A + 1) * nb
    design = wn.design_frame(p)
    ds = float(p["station_length"])
    tr = np.asarray(pose, np.float64)[:3, 3]
    out = dict(anchor_station=int(np.floor(((tr - design["o"]) @ design["a"] - p["t_min"]) / ds)))
    ssd, n = [int(x) for x in t["ssd"]], [int(x) for x in t["n"]]
    valid = [x >= ap["min_overlap"] for x in n]
    cheb = lambda i, a0=0, b0=0: max(abs(i // nb - A - a0), abs(i % nb - B - b0))  # noqa: E731
    best = -1
    for i in range(len(t)):
        if not valid[i]:
            continue
        if best >= 0:
            lhs, rhs = ssd[i] * n[best], ssd[best] * n[i]            # exact: Python integers
            if lhs > rhs or (lhs == rhs and cheb(i) >= cheb(best)):
                continue
        best = i
    if best < 0:
        nan = float("nan")
        out.update(status=NO_OVERLAP, overlap=0, best_station=0, best_sector=0, frac_station=nan, frac_sector=nan, shift_m=nan,
                   roll=nan, bias_m=nan, rms_best=nan, rms_runner=nan, distinction=nan, pose=np.full((3, 4), nan))
        return out
    cost = lambda i: float(ssd[i]) / float(n[i])  # noqa: E731
    ia, ib = best // nb, best % nb
    sa, sb = ia - A, ib - B
    c0 = cost(best)

    def fraction(lo, hi, have):
        if not have or not valid[lo] or not valid[hi]:
            return 0.0
        cm, cp = cost(lo), cost(hi)
        den = cm - 2.0 * c0 + cp
        if not den > 0.0:
            return 0.0
        return float(min(0.5, max(-0.5, 0.5 * (cm - cp) / den)))

    fa = fraction(best - nb, best + nb, 0 < ia < 2 * A)
    fb = fraction(best - 1, best + 1, 0 < ib < 2 * B)
    run = [cost(i) for i in range(len(t)) if valid[i] and cheb(i, sa, sb) > 1]
    cr = min(run) if run else float("inf")
    dist = float("inf") if (c0 == 0.0 or not run) else cr / c0
    status = OK
    if dist < ap["min_distinction"]:
        status |= AMBIGUOUS
    if (A > 0 and abs(sa) == A) or (B > 0 and abs(sb) == B):
        status |= AT_BORDER
    shift_m = (sa + fa) * ds
    roll = (sb + fb) * (2 * np.pi / p["n_sectors"])
    out.update(status=status, overlap=n[best], best_station=sa, best_sector=sb, frac_station=fa, frac_sector=fb,
               shift_m=shift_m, roll=roll, bias_m=(float(int(t["sum_d"][best])) * 2.0 ** -20) / float(n[best]),
               rms_best=np.sqrt(c0) * 2.0 ** -20, rms_runner=(np.sqrt(cr) * 2.0 ** -20 if run else float("nan")),
               distinction=dist, pose=compose(design, pose, shift_m, roll))
    return out


def points(xyz, labels, frame, p, ap):
    """Per point in fp64 on the reported add info `frame`: dict(e (NaN for plane points), cell (jr n_sectors + k of a
    binned point, else -1), cls (index into CLASSES), ambiguous)."""
    P, ns = ap["half_patch_stations"], int(p["n_sectors"])
    r = wn.points(xyz, labels, frame, dict(p, gate=ap["gate"]))
    gate = float(np.float32(ap["gate"]))
    ds = float(np.float32(p["station_length"]))
    dth = float(np.float32(2 * np.pi / ns))
    e = r["e"]
    plane = np.isnan(e) & (np.zeros(len(e), bool) if labels is None else np.asarray(labels) == 1)
    with np.errstate(invalid="ignore"):
        beyond = ~plane & ~(np.abs(e) <= gate)
        jl = np.floor(r["t"] / ds)
        k = np.minimum(np.floor(r["phi"] / dth), ns - 1)
        outside = ~plane & ~beyond & ~((jl >= -P) & (jl < P))
    binned = ~plane & ~beyond & ~outside
    cls = np.full(len(e), 3, np.int8)
    cls[plane], cls[beyond], cls[outside] = 0, 1, 2
    cell = np.full(len(e), -1, np.int64)
    cell[binned] = (jl[binned].astype(np.int64) + P) * ns + k[binned].astype(np.int64)
    return dict(e=e, cell=cell, cls=cls, ambiguous=r["ambiguous"])


def align(xyz, labels, p, pose, raw, ap):
    """The whole align in fp64 + integers (the frame rounded to fp32 once, as the device does): (select() dict with the
    class counts, table).  Its patch is the twin's own binning, so it may differ from the device's in ambiguous points."""
    design = wn.design_frame(p)
    frame = wn.add_frame(design, p, pose)
    r = points(xyz, labels, frame, p, ap)
    ns, P = int(p["n_sectors"]), ap["half_patch_stations"]
    e32 = np.where(np.isnan(r["e"]), 0.0, r["e"]).astype(np.float32)
    psum, pcnt = patch_from(e32, r["cell"], 2 * P * ns)
    tab = table(psum, pcnt, raw, frame["anchor"], ns, ap)
    out = select(tab, p, pose, ap)
    out.update({q: int((r["cls"] == i).sum()) for i, q in enumerate(CLASSES)})
    out["patch_cells_usable"] = int((pcnt >= ap["min_frame_count"]).sum())
    return out, tab
