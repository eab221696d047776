"""The twin of the checked add alone (tests/wall_add_checked_np.py): no GPU, no library.  A hand-built frame of 12 points
and 13 rows that hold every edge of the rule of include/gm_hip.h: |dq| == S and S - 1, a zero and a NaN delta, an infinite
one, index == n, a duplicate index, both signs under each skip value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wall_add_checked_np as an  # noqa: E402
import wall_check_np as wk  # noqa: E402

N = 12
S = 1 << 19   # min_delta = 0.5
Q = np.float32(2.0 ** -20)


def _rows():
    # (index, delta): the delta is exact in fp32 for every |dq| <= 2^24
    spec = [(0, S * Q),                 # 0  |dq| == S, positive: selected by POS
            (1, -(S * Q)),              # 1  |dq| == S, negative: selected by NEG
            (2, (S - 1) * Q),           # 2  S - 1: kept
            (3, -((S - 1) * Q)),        # 3  S - 1: kept
            (4, np.float32(0.0)),       # 4  zero: rejected
            (5, np.float32("nan")),     # 5  NaN: rejected
            (6, np.float32("inf")),     # 6  not finite: rejected
            (N, np.float32(1.0)),       # 7  index == n: rejected
            (7, np.float32(1.0)),       # 8  selected by POS
            (7, np.float32(2.0)),       # 9  the same point again
            (11, np.float32(-3.0)),     # 10 the last point, NEG
            (7, np.float32(-1.0)),      # 11 the duplicated point, the other sign
            (9, np.float32(2.0 ** -21))]   # 12 rounds to dq == 0 (nearest even): rejected
    r = np.zeros(len(spec), wk.POINT)
    r["index"] = [s[0] for s in spec]
    r["delta"] = np.array([s[1] for s in spec], np.float32)
    r["cell"] = 5
    return r


WANT = {
    3: ([an.POS, an.NEG, an.KEPT, an.KEPT, an.REJECTED, an.REJECTED, an.REJECTED, an.REJECTED, an.POS, an.POS, an.NEG, an.NEG,
         an.REJECTED], [0, 1, 7, 11]),
    1: ([an.KEPT, an.NEG, an.KEPT, an.KEPT, an.REJECTED, an.REJECTED, an.REJECTED, an.REJECTED, an.KEPT, an.KEPT, an.NEG, an.NEG,
         an.REJECTED], [1, 7, 11]),
    2: ([an.POS, an.KEPT, an.KEPT, an.KEPT, an.REJECTED, an.REJECTED, an.REJECTED, an.REJECTED, an.POS, an.POS, an.KEPT, an.KEPT,
         an.REJECTED], [0, 7]),
}


@pytest.mark.parametrize("skip", [1, 2, 3])
def test_row_classes_and_skipped_set(skip):
    assert an.min_delta_q(0.5) == S
    cls, skipped = an.select(_rows(), N, skip=skip, min_delta=0.5)
    want_cls, want_skipped = WANT[skip]
    assert cls.tolist() == want_cls
    assert skipped.tolist() == want_skipped and skipped.dtype == np.int64
    # the order of the rows does not matter
    perm = np.random.default_rng(skip).permutation(len(cls))
    cls2, skipped2 = an.select(_rows()[perm], N, skip=skip, min_delta=0.5)
    assert cls2.tolist() == cls[perm].tolist() and skipped2.tolist() == want_skipped


def test_min_delta_zero_selects_every_usable_row():
    cls, skipped = an.select(_rows(), N)
    assert (cls == an.KEPT).sum() == 0 and (cls == an.REJECTED).sum() == 5
    assert skipped.tolist() == [0, 1, 2, 3, 7, 11]


def test_info_counts_and_sum_rules():
    rows = _rows()
    # the add's per-point outputs of the whole cloud: point 8 plane, 10 beyond the gate, 6 outside, 7 (skipped) outside too
    e = np.full(N, 0.01, np.float32)
    cell = np.arange(N, dtype=np.int64)
    labels = np.zeros(N, np.uint8)
    labels[8] = 1
    e[8] = np.nan
    cell[8] = -1
    e[10] = 0.3
    cell[10] = -1
    cell[6] = -1
    cell[7] = -1
    labels[11] = 1   # a skipped plane point is skipped, not plane
    e[11] = np.nan
    cell[11] = -1
    d = an.info(rows, e, cell, 0.25, labels, status=256, skip=3, min_delta=0.5)
    assert d == dict(status=256, min_delta_q=S, n_points=N, n_rows=13, reserved=0, rows_neg=3, rows_pos=3, rows_kept=2,
                     rows_rejected=5, skipped=4, plane=1, beyond_gate=1, outside=1, mapped=5)
    assert d["rows_neg"] + d["rows_pos"] + d["rows_kept"] + d["rows_rejected"] == d["n_rows"]
    assert d["skipped"] + d["plane"] + d["beyond_gate"] + d["outside"] + d["mapped"] == d["n_points"]
    assert an.keep(N, [0, 1, 7, 11]).tolist() == [i not in (0, 1, 7, 11) for i in range(N)]


def test_no_rows_and_params():
    cls, skipped = an.select(np.zeros(0, wk.POINT), 5)
    assert len(cls) == 0 and len(skipped) == 0
    d = an.info(np.zeros(0, wk.POINT), np.zeros(3, np.float32), np.array([1, -1, 2]), 0.25)
    assert (d["skipped"], d["mapped"], d["outside"], d["n_rows"]) == (0, 2, 1, 0)
    assert an.params_ok(1, 0.0) and an.params_ok(3, 8.0) and not an.params_ok(0, 0.0) and not an.params_ok(4, 0.0)
    assert not an.params_ok(3, -1e-9) and not an.params_ok(3, 8.1) and not an.params_ok(3, float("nan"))
    with pytest.raises(TypeError):
        an.params(threshold=1.0)
