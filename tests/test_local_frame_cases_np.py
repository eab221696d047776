"""CPU tests of tests/local_frame_cases.py and of the references the GPU tests of the local frame hold the device to
(tests/test_gpu_local_frame_edges.py).

Every case is what it claims: M an integer matrix below 2^24, M q_i == lambda_i q_i in integer arithmetic for the known
spectra, and for the cases whose reference is numpy.linalg.eigh every eigenvalue bracketed, within 2^-44 of the largest,
by a sign change of the exact integer characteristic polynomial (simple roots: the spectrum is in the class the case is
filed under).  The oracle returns exactly the integer M in both of its modes, which makes its f32-faithful solve a valid
sign reference on these inputs.  gm_solve_local_frame, the host compile of the code under test, meets every bound of the
GPU tests against the exact references on every case and has the oracle's column signs on every separated one (of the
sweep: every draw with its gaps at least 2^-18 of the largest eigenvalue, all but 46 of 2000),
the recorded contraction-sensitive indices included: the references stay inside the bounds."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_frame_cases as lf  # noqa: E402


@functools.lru_cache(maxsize=None)
def known():
    return tuple(lf.known_cases())


@functools.lru_cache(maxsize=None)
def structured():
    return tuple(lf.structured_cases())


@functools.lru_cache(maxsize=None)
def sweep():
    return tuple(lf.sweep_cases())


def signed_cases():
    """The cases whose eigenvector signs are compared: every separated one, the sweep's included."""
    return [c for c in known() + structured() + sweep() if c.cls == lf.SEPARATED]


# ------------------------------------------------------------------ the cases are what they claim

def test_every_case_is_an_integer_matrix_below_2_24():
    cases = known() + structured() + sweep()
    assert len(sweep()) == lf.SWEEP_N and len(set(c.name for c in cases)) == len(cases)
    for c in cases:
        assert c.M.dtype == np.int64 and np.abs(c.M).max() < lf.LIMIT, c.name
        assert np.array_equal(c.M, c.M.T)
        assert np.array_equal(c.normals[:, :3].astype(np.int64), c.rows) and np.all(c.normals[:, 3] == 0), c.name
        assert np.array_equal(c.M.astype(np.float32).astype(np.int64), c.M)


def test_known_spectra_hold_in_integer_arithmetic():
    seen = set()
    for c in known():
        seen.add(c.cls)
        if c.cls == lf.ZERO:
            assert not c.M.any()
            continue
        lam, vec = c.lam_int, c.vec_int
        assert np.array_equal(c.M @ vec, vec * lam[None, :]), c.name                     # M q_i == lambda_i q_i
        d2 = int(vec[:, 0] @ vec[:, 0])
        assert np.array_equal(vec.T @ vec, d2 * np.eye(3, dtype=np.int64)), c.name       # orthogonal, equal lengths
        assert np.all(np.diff(lam) >= 0) and np.array_equal(c.lam, lam.astype(np.float64))
        l0, l1, l2 = (int(v) for v in lam)
        want = {lf.SEPARATED: 0 < l0 < l1 < l2, lf.DOUBLE_LOW: 0 < l0 == l1 < l2, lf.DOUBLE_HIGH: 0 < l0 < l1 == l2,
                lf.TRIPLE: 0 < l0 == l1 == l2, lf.RANK2: 0 == l0 < l1 <= l2, lf.RANK1: 0 == l0 == l1 < l2}[c.cls]
        assert want, (c.name, lam)
    assert seen == {lf.SEPARATED} | set(lf.DEGENERATE)
    # ratios from about one half down to 1e-6
    sep = [c for c in known() if c.cls == lf.SEPARATED]
    assert max(c.lam[0] / c.lam[1] for c in sep) > 0.45 and min(c.lam[0] / c.lam[2] for c in sep) <= 1.0e-6


def test_diagonal_and_branch_cases():
    diag = [c for c in known() if c.name.startswith("diag_") and c.cls == lf.SEPARATED]
    orders = set(tuple(np.argsort(np.diag(c.M))) for c in diag)
    assert len(orders) == 6 and all(not (c.M - np.diag(np.diag(c.M))).any() for c in diag)
    by = {c.name: c.M for c in structured()}
    for n in ("a20_zero_a10_pos", "a20_zero_a10_neg", "a20_zero_a10_neg_large"):
        assert by[n][2, 0] == 0 and by[n][1, 0] != 0 and by[n][2, 1] != 0       # no reflection, yet QR steps to do
    assert by["a20_zero_a10_pos"][1, 0] > 0 > by["a20_zero_a10_neg"][1, 0]
    for n, s10, s20 in (("a10_pos_a20_pos", 1, 1), ("a10_pos_a20_neg", 1, -1), ("a10_neg_a20_pos", -1, 1),
                        ("a10_neg_a20_neg", -1, -1)):
        assert np.sign(by[n][1, 0]) == s10 and np.sign(by[n][2, 0]) == s20
    for n in ("offdiag_all_negative", "offdiag_all_negative_large"):
        assert by[n][1, 0] < 0 and by[n][2, 0] < 0 and by[n][2, 1] < 0
    # the known spectra reach both Householder signs too
    sep = [c.M for c in known() if c.cls == lf.SEPARATED]
    assert any(M[1, 0] > 0 and M[2, 0] != 0 for M in sep) and any(M[1, 0] < 0 and M[2, 0] != 0 for M in sep)
    assert any(M[1, 0] < 0 and M[2, 0] < 0 and M[2, 1] < 0 for M in sep)


def test_eigh_references_are_bracketed_by_the_exact_characteristic_polynomial():
    from fractions import Fraction
    for c in structured() + sweep():
        if c.cls == lf.ZERO:
            assert not c.M.any()
            continue
        lmax = c.lam[2]
        # every pair by residual and orthonormality: the spectrum of M is within the residual of lam, multiplicities included
        res = np.abs(c.M.astype(np.float64) @ c.V - c.V * c.lam[None, :]).max()
        assert res <= 2.0 ** -44 * lmax and np.abs(c.V.T @ c.V - np.eye(3)).max() <= 2.0 ** -44, c.name
        if c.cls == lf.CLOSE:
            assert c.gap.min() < lf.SIGN_MIN_GAP * lmax, c.name
            continue
        assert c.cls == lf.SEPARATED and np.all(c.gap >= lf.SIGN_MIN_GAP * lmax), c.name
        p = lf.charpoly(c.M)
        delta = Fraction(float(lmax)) / (1 << 44)
        for i in range(3):
            lo, hi = p(Fraction(float(c.lam[i])) - delta), p(Fraction(float(c.lam[i])) + delta)
            assert lo * hi < 0, (c.name, i)                                      # a root inside: three simple eigenvalues


def test_sweep_classes_and_the_recorded_indices():
    sw = sweep()
    assert all(c.cls == lf.SEPARATED for c in structured())
    assert sorted(set(len(c.rows) for c in sw)) == [3, 4, 5, 6, 7, 8]
    assert sum(lf.well_separated(c.lam) for c in sw) > lf.SWEEP_N // 2
    assert min(c.lam[0] / c.lam[2] for c in sw) < 1e-6 and max(c.lam[0] / c.lam[2] for c in sw) > 0.25
    # how many draws the sign comparison leaves out, and that the eigenpair bounds keep them
    assert sum(c.cls != lf.SEPARATED for c in sw) == lf.SWEEP_CLOSE and set(c.cls for c in sw) <= {lf.SEPARATED, lf.CLOSE, lf.ZERO}
    idx = lf.CONTRACTION_SENSITIVE
    assert len(set(idx)) == len(idx) and all(0 <= i < lf.SWEEP_N and sw[i].cls == lf.SEPARATED for i in idx)
    assert sum(lf.well_separated(sw[i].lam) for i in idx) >= 10


def test_rule_rows_and_sums():
    for k, (p, q, r) in enumerate(lf.RULES):
        rows = lf.rule_rows(1000, k)
        assert rows.dtype == np.float32 and np.all(rows[:, 3] == 0) and np.all(rows == np.rint(rows))
        assert np.abs(rows).max() <= 6
        i = 777
        assert tuple(rows[i, :3]) == (i % p - p // 2, i % q - q // 2, i % r - r // 2)
        assert np.array_equal(lf.rule_rows(10, k, start=990), rows[990:])
    # the first rule repeats only every 105 rows
    rows = lf.rule_rows(210)[:, :3]
    assert all(not np.array_equal(rows[0], rows[j]) for j in range(1, 105)) and np.array_equal(rows[:105], rows[105:])
    # any two rules differ on every prefix the sequence test uses
    for n in (257, 16385):
        sums = [tuple(lf.rule_sum(n, k)) for k in range(len(lf.RULES))]
        assert len(set(sums)) == len(sums)
    # the largest exact sum is far below 2^53
    assert 36 * (4194304 + 4097) < 2 ** 53


# ------------------------------------------------------------------ the oracle on these inputs

def test_oracle_returns_the_integer_scatter_matrix_in_both_modes(oc):
    """The f32-faithful mode, the sign reference, stores the weight to float as the library does: exactly M at wf = 1000.
    The f64 mode keeps the weight in double, where exp(1e-12) = 1 + 1e-12 is not 1: it returns exactly M from wf = 1e9 on
    (t^2 = 1e-24 < 2^-53), and at wf = 1000 M scaled by that weight's square, 2e-12, to a few fp64 roundings."""
    for c in signed_cases() + [c for c in known() if c.cls != lf.SEPARATED]:
        Mx = c.M.astype(np.float64)
        _, _, M = oc.local_frame(c.normals, lf.WF_EXACT, oc.F32_FAITHFUL)
        assert np.array_equal(M, Mx), c.name
        _, _, M = oc.local_frame(c.normals, 1.0e9, oc.F64)
        assert np.array_equal(M, Mx), c.name
        _, _, M = oc.local_frame(c.normals, lf.WF_EXACT, oc.F64)
        assert np.all(np.abs(M - Mx * np.exp(2.0e-12)) <= 2.0 ** -49 * np.abs(c.M).max()), c.name


def test_weight_is_one_at_curvature_zero_and_wf_1000():
    t = np.float64(np.float32(0.0)) + 0.001 / lf.WF_EXACT
    assert np.float32(np.exp(t * t)) == np.float32(1.0) and np.exp(t * t) - 1.0 < 2.0 ** -24


# ------------------------------------------------------------------ the host compile of the code under test

def test_host_solve_meets_the_eigenpair_bounds(gm):
    worst = [0.0, 0.0, 0.0]
    for c in known() + structured() + sweep():
        ev, V = gm.solve_local_frame(lf.six(c.M).astype(np.float64))
        f = lf.check_eigenpairs(c, ev, V)
        worst = [max(a, b) for a, b in zip(worst, f)]
    print("host solve: eigenvalue error / bound %.3f, angle / bound %.3f, |V^T V - I| %.3g (bound %.3g)"
          % (worst[0], worst[1], worst[2], lf.ORTHO))


def test_host_solve_has_the_oracle_signs(gm, oc):
    low = 1.0
    for c in signed_cases():
        ev, V = gm.solve_local_frame(lf.six(c.M).astype(np.float64))
        _, oV, _ = oc.local_frame(c.normals, lf.WF_EXACT, oc.F32_FAITHFUL)
        d = lf.column_dots(V, oV)
        assert np.all(d > lf.SIGN_DOT), (c.name, d)
        low = min(low, float(d.min()))
    print("host solve against the f32-faithful oracle: smallest column dot %.9f" % low)


def test_host_solve_has_the_oracle_signs_on_the_contraction_sensitive_indices(gm, oc):
    sw = sweep()
    for i in lf.CONTRACTION_SENSITIVE:
        c = sw[i]
        ev, V = gm.solve_local_frame(lf.six(c.M).astype(np.float64))
        _, oV, _ = oc.local_frame(c.normals, lf.WF_EXACT, oc.F32_FAITHFUL)
        assert np.all(lf.column_dots(V, oV) > lf.SIGN_DOT), (i, lf.column_dots(V, oV))
