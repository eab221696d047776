"""Case builders and exact references for the local frame's closing step (csrc/k_frame.hip: k_scatter_partials and
k_valid_scan; csrc/gm_device.hpp: frame_finalize_block, eig3_sym_eigen_signs).  numpy only.

Exact rows.  The device forms w = float(exp((c + .001/wf)^2)) with the inner arithmetic in double.  With curvature c = 0
and wf = 1000, t = 1e-6 and exp(t^2) - 1 = 1e-12 < 2^-24, so w == 1.0f exactly.  Rows (a, b, c, 0) with small integers
a, b, c then make every product and every fp64 sum an exact integer whatever the reduction order: the reference is an
int64 numpy sum and the comparison is ==.

Known spectra.  Q3 = (1/3)[[1,2,2],[2,1,-2],[2,-2,1]] and Q7 = (1/7)[[2,3,6],[3,-6,2],[6,2,-3]] are rational orthogonal
matrices.  With d = 3 or 7 the three rows s_i * (d q_i) are integer rows and give M = sum_i (s_i d)^2 q_i q_i^T: exact
eigenvalues (s_i d)^2, exact eigenvectors q_i.  Coordinate permutations and coordinate sign changes of Q (a sign change of
a whole ROW of the scatter input changes nothing: it enters squared) give further orthogonal matrices of the same kind.
Every |M_ij| stays below 2^24, so the float copy of M that the sign rule solves is the same number for device, host and
oracle, and the oracle's float accumulation of M is exact as well (every partial sum of a diagonal entry is below the
final one, every partial off-diagonal sum below the larger diagonal by Cauchy-Schwarz).

Seeded sweep.  SWEEP_N cases of 3 to 8 integer rows, per-axis magnitudes drawn from {1, 8, 60, 500, 1000}.  A draw is
discarded only when an |M_ij| >= 2^24.  Every draw is held to the exact sum and to the eigenpair bounds (the angle bound
scales with lmax / gap and needs no filter; a draw with a gap below 2^-18 lmax is held by its residuals as well).  The
reference is numpy.linalg.eigh in fp64; tests/test_local_frame_cases_np.py brackets each eigenvalue of a SEPARATED draw by
an exact sign change of the integer characteristic polynomial and holds every draw's pairs by residual and orthonormality.
Signs are compared on the draws whose every gap is at least SIGN_MIN_GAP = 2^-18 of the largest eigenvalue: the float
solve whose columns are the sign reference has a backward error near one float epsilon of lmax, so its columns are off by
about 2^-23 * lmax / gap in angle; a column dot of 0.999 is 0.0447 rad = 2^-4.5, reached at gap / lmax = 2^-18.5, and
below that "same sign" stops being a statement about two nearby vectors.  The CPU tests assert how many draws that leaves
out (SWEEP_CLOSE: two axes of magnitude 1 or 8 beside one of 500 or 1000 for the most part; two exact double eigenvalues).
"""
import itertools
from fractions import Fraction

import numpy as np

WF_EXACT = 1000.0          # w == 1.0f at curvature 0
LIMIT = 1 << 24            # |M_ij| below this: float(M) is exact

Q3 = np.array([[1, 2, 2], [2, 1, -2], [2, -2, 1]], dtype=np.int64)       # 3 * Q3, columns d * q_i
Q7 = np.array([[2, 3, 6], [3, -6, 2], [6, 2, -3]], dtype=np.int64)       # 7 * Q7
EYE = np.eye(3, dtype=np.int64)

SEPARATED = "separated"            # three simple eigenvalues (the sweep's and the structured ones: every gap >= 2^-18 lmax)
CLOSE = "close"                    # a sweep draw with a gap below 2^-18 lmax, zero included: no sign comparison
DOUBLE_LOW = "double_low"          # lambda0 == lambda1 < lambda2
DOUBLE_HIGH = "double_high"        # lambda0 < lambda1 == lambda2
TRIPLE = "triple"
RANK2 = "rank2"                    # 0 < lambda1 < lambda2
RANK1 = "rank1"                    # 0 == 0 < lambda2
ZERO = "zero"                      # all-zero rows (n > 0) and n = 0
DEGENERATE = (DOUBLE_LOW, DOUBLE_HIGH, TRIPLE, RANK2, RANK1, ZERO)
BY_RESIDUAL = DEGENERATE + (CLOSE,)   # classes whose every column is also held by its residual


# ------------------------------------------------------------------ rows and exact sums

def as_normals(rows3):
    """[n,3] integers -> the [n,4] float32 normals cloud (curvature 0) the library takes."""
    r = np.asarray(rows3)
    out = np.zeros((r.shape[0], 4), np.float32)
    out[:, :3] = r
    return out


def scatter_int(rows3):
    """The exact scatter matrix of integer rows: int64 [3,3]."""
    r = np.asarray(rows3, dtype=np.int64).reshape(-1, 3)
    return r.T @ r


def six(M):
    """[3,3] -> {xx, xy, xz, yy, yz, zz}, the order of scatter6."""
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


# Position-dependent rows for the size edges: a rule (p, q, r) makes row i = (i % p - p // 2, i % q - q // 2, i % r - r // 2).
# The first repeats only every 105 rows, so a row dropped, doubled or read past n changes M; a stale partial row of an
# earlier call shows because each call of a sequence uses another rule (under one rule whole periods can cancel).
RULES = ((7, 5, 3), (11, 3, 5), (5, 9, 7), (13, 7, 11))


def rule_rows(n, rule=0, start=0):
    p, q, r = RULES[rule]
    i = np.arange(start, start + n, dtype=np.int64)
    out = np.zeros((n, 4), np.float32)
    out[:, 0] = i % p - p // 2
    out[:, 1] = i % q - q // 2
    out[:, 2] = i % r - r // 2
    return out


def rule_sum(n, rule=0, start=0):
    """scatter6 of rule_rows(n, rule, start), exactly (int64)."""
    return six(scatter_int(rule_rows(n, rule, start)[:, :3].astype(np.int64)))


# ------------------------------------------------------------------ cases

class Case:
    """rows: int64 [k,3] (k may be 0).  M: int64 [3,3].  lam: float64 [3] ascending (exact integers for the known
    spectra).  V: float64 [3,3], unit eigenvectors in columns.  simple[i]: lambda_i is a simple eigenvalue.
    vec_int: for the known spectra the integer eigenvectors d * q_i in columns (M vec_int[:, i] == lam_int[i] vec_int[:, i]
    exactly), else None."""

    def __init__(self, name, cls, rows, lam, V, vec_int=None, lam_int=None):
        self.name, self.cls = name, cls
        self.rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        self.M = scatter_int(self.rows)
        self.lam = np.asarray(lam, dtype=np.float64)
        self.V = np.asarray(V, dtype=np.float64)
        self.vec_int, self.lam_int = vec_int, lam_int
        lmax = self.lam[2]
        self.gap = np.array([min(abs(self.lam[i] - self.lam[j]) for j in range(3) if j != i) for i in range(3)])
        self.simple = self.gap > 0 if lmax > 0 else np.zeros(3, bool)

    @property
    def normals(self):
        return as_normals(self.rows)

    def __repr__(self):
        return "Case(%s)" % self.name


def _bases():
    """(name, B) with B an integer matrix whose columns are d * q_i: Q3 and Q7 under the four coordinate sign changes that
    differ (D and -D give the same M) and the six coordinate permutations."""
    out = []
    for qn, Q in (("q3", Q3), ("q7", Q7)):
        for fi, flip in enumerate(((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))):
            for pi, perm in enumerate(itertools.permutations(range(3))):
                B = (np.diag(flip) @ Q)[list(perm), :]
                out.append(("%s_f%d_p%d" % (qn, fi, pi), B))
    return out


def _known(name, cls, B, s):
    """Rows s_i * B[:, i]; the spectrum sorted ascending (stable: equal eigenvalues keep the column order)."""
    s = np.asarray(s, dtype=np.int64)
    d2 = int(B[:, 0] @ B[:, 0])                     # d^2
    rows = (B * s[None, :]).T
    lam = s * s * d2
    order = np.argsort(lam, kind="stable")
    vec = B[:, order]
    lam = lam[order]
    return Case(name, cls, rows, lam.astype(np.float64), vec / np.sqrt(float(d2)), vec_int=vec, lam_int=lam)


def _scaled(s, B):
    """The s triple for this basis: with d = 7 the factors from 500 up are halved so that (s d)^2 < 2^24 (no triple of
    the tables below changes its class by that)."""
    if int(B[:, 0] @ B[:, 0]) == 49:
        return tuple(v // 2 if v >= 500 else v for v in s)
    return s


# eigenvalue ratios (s_i / s_j)^2: from about 1/2 (5:7:10) down to 1e-6 (1:1000)
_SEPARATED_S = ((5, 7, 10), (1, 2, 4), (1, 3, 9), (1, 10, 100), (1, 31, 1000), (1, 2, 1000), (1, 500, 1000), (3, 1000, 400))
_DOUBLE_LOW_S = ((1, 1, 2), (3, 3, 1000), (500, 500, 1000), (7, 7, 8))
_DOUBLE_HIGH_S = ((1, 2, 2), (1, 1000, 1000), (999, 1000, 1000), (7, 8, 8))
_RANK2_S = ((0, 1, 2), (0, 1, 1000), (0, 999, 1000), (0, 5, 5))
_RANK1_S = ((0, 0, 1), (0, 0, 1000))


def known_cases():
    out = []
    bases = _bases()
    for bn, B in bases:
        for s in _SEPARATED_S:
            for rot in range(3):      # which q_i gets which factor
                sr = _scaled(s[rot:] + s[:rot], B)
                out.append(_known("sep_%s_s%d_%d_%d" % ((bn,) + sr), SEPARATED, B, sr))
    for bn, B in bases[::5]:
        for cls, table in ((DOUBLE_LOW, _DOUBLE_LOW_S), (DOUBLE_HIGH, _DOUBLE_HIGH_S), (RANK2, _RANK2_S), (RANK1, _RANK1_S)):
            for s in table:
                for rot in range(3):
                    sr = _scaled(s[rot:] + s[:rot], B)
                    out.append(_known("%s_%s_s%d_%d_%d" % ((cls, bn) + sr), cls, B, sr))
    for s in (1, 7, 1000):
        out.append(_known("triple_q3_s%d" % s, TRIPLE, Q3, (s, s, s)))
        out.append(_known("triple_eye_s%d" % (3 * s), TRIPLE, EYE, (3 * s, 3 * s, 3 * s)))
    # diagonal M in all six orders of the diagonal (the float solve: no reflection, no QR step, the sort alone)
    for perm in itertools.permutations((1, 60, 4000)):
        out.append(_known("diag_%d_%d_%d" % perm, SEPARATED, EYE, perm))
    out.append(_known("diag_double_low", DOUBLE_LOW, EYE, (5, 9, 5)))
    out.append(_known("diag_double_high", DOUBLE_HIGH, EYE, (9, 5, 9)))
    out.append(_known("diag_rank1", RANK1, EYE, (0, 12, 0)))
    # the zero matrix
    out.append(Case("zero_rows_3", ZERO, np.zeros((3, 3)), np.zeros(3), np.eye(3)))
    out.append(Case("zero_rows_1", ZERO, np.zeros((1, 3)), np.zeros(3), np.eye(3)))
    out.append(Case("n_0", ZERO, np.zeros((0, 3)), np.zeros(3), np.eye(3)))
    return out


def eigh_case(name, rows, cls=SEPARATED):
    """A case whose reference is numpy.linalg.eigh of the exact integer M (fp64: eigenvalues to about 1e-16 lmax,
    eigenvectors to about 1e-16 lmax / gap, 2^-12 of what the angle bound allows at any gap); the class is verified by the
    CPU tests, for SEPARATED with exact arithmetic."""
    M = scatter_int(rows)
    lam, V = np.linalg.eigh(M.astype(np.float64))
    return Case(name, cls, rows, lam, V)


def structured_cases():
    """The branches of the float solve's tridiagonalisation (eigen_tridiag_qr3): a20 == 0 with a10 != 0 (no reflection, yet
    QR steps), both Householder signs (a10 > 0, a10 < 0 with a20 != 0), all off-diagonals negative."""
    return [
        eigh_case("a20_zero_a10_pos", [[1, 2, 0], [0, 3, 5], [0, 1, -2], [4, 0, 0]]),
        eigh_case("a20_zero_a10_neg", [[1, -2, 0], [0, 3, 5], [0, 1, -2], [4, 0, 0]]),
        eigh_case("a20_zero_a10_neg_large", [[100, -700, 0], [0, 30, 500], [0, 10, -20], [7, 0, 0]]),
        eigh_case("a10_pos_a20_pos", [[1, 2, 3], [2, 5, 1], [1, 0, 4]]),
        eigh_case("a10_pos_a20_neg", [[1, 2, -3], [2, 5, -1], [1, 0, -4]]),
        eigh_case("a10_neg_a20_pos", [[1, -2, 3], [2, -5, 1], [1, 0, 4]]),
        eigh_case("a10_neg_a20_neg", [[-1, 2, 3], [-2, 5, 1], [-1, 0, 4], [0, 7, 7]]),
        eigh_case("offdiag_all_negative", [[1, -2, 0], [1, 0, -3], [0, 2, -1], [0, 1, -5]]),
        eigh_case("offdiag_all_negative_large", [[1000, -2, 0], [900, 0, -3], [0, 20, -10], [0, 10, -500]]),
    ]


SWEEP_SEED = 20260
SWEEP_N = 2000
SWEEP_MAGS = (1, 8, 60, 500, 1000)
SIGN_MIN_GAP = 2.0 ** -18
SWEEP_CLOSE = 46            # draws of the sweep filed under CLOSE or ZERO, i.e. left out of the sign comparison


def sweep_rows():
    """The first SWEEP_N draws with every |M_ij| < 2^24, in order: a list of int64 [k,3] arrays."""
    rng = np.random.default_rng(SWEEP_SEED)
    out = []
    while len(out) < SWEEP_N:
        k = int(rng.integers(3, 9))
        mag = rng.choice(SWEEP_MAGS, size=3)
        rows = rng.integers(-mag, mag + 1, size=(k, 3))
        if np.abs(scatter_int(rows)).max() >= LIMIT:
            continue
        out.append(rows)
    return out


def sweep_cases():
    """Every draw is a case of the sums and of the eigenpair bounds.  SEPARATED: every gap >= SIGN_MIN_GAP * lmax, the
    draws whose column signs are compared.  CLOSE: the others (double eigenvalues among them); ZERO: M == 0."""
    out = []
    for i, r in enumerate(sweep_rows()):
        M = scatter_int(r)
        if not M.any():
            out.append(Case("sweep_%04d" % i, ZERO, r, np.zeros(3), np.eye(3)))
            continue
        lam = np.linalg.eigvalsh(M.astype(np.float64))
        sep = min(lam[1] - lam[0], lam[2] - lam[1]) >= SIGN_MIN_GAP * lam[2]
        out.append(eigh_case("sweep_%04d" % i, r, SEPARATED if sep else CLOSE))
    return out


def well_separated(lam):
    """Each eigenvalue under half the next."""
    return lam[0] < 0.5 * lam[1] and lam[1] < 0.5 * lam[2]


# Sweep indices, among the SEPARATED draws, on which a build of the float solve (eigen_tridiag_qr3<float>) with its products
# contracted to FMAs and a build that rounds every product return at least one eigenvector column with opposite sign.
# Found on the CPU: the three solvers of csrc/gm_device.hpp as they stood before the solve carried its contraction pragma,
# compiled unchanged into a host program with clang -O3 -ffp-contract=on -fno-fast-math, once plain and once with -mfma,
# run on this sweep (a build with contraction off agrees with the plain one bit for bit).  355 and 461 apart, every one
# has a well-separated spectrum (well_separated above): 25.  The CPU tests check that count.
CONTRACTION_SENSITIVE = (32, 131, 132, 187, 317, 355, 461, 512, 542, 590, 634, 697, 911, 969, 978, 995, 1051, 1135, 1229,
                         1324, 1476, 1482, 1637, 1658, 1792, 1825, 1972)


# ------------------------------------------------------------------ bounds (derived; see the test files' docstrings)

EVAL_REL = 2.0 ** -23          # one float ulp of the stored result
EVAL_ABS = 2.0 ** -40          # 4096 fp64 epsilons of lmax: the Jacobi iteration's backward error
ANGLE_ABS = 2.0 ** -22
ORTHO = 2.0 ** -21
RESIDUAL = 2.0 ** -21
SIGN_DOT = 0.999


def unsigned_angle(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.arcsin(min(s, 1.0)))


def check_eigenpairs(case, ev, V, M=None):
    """The bounds of the eigenpair tests for one solve (ev [3] float32, V [3,3] float32 columns) of case.M; returns the
    figures (worst eigenvalue excess ratio, worst angle ratio, orthonormality defect) and asserts each bound."""
    ev64, V64 = np.asarray(ev, np.float64), np.asarray(V, np.float64)
    Mf = (case.M if M is None else M).astype(np.float64)
    lmax = case.lam[2]
    assert np.all(np.isfinite(ev64)) and np.all(np.isfinite(V64)), (case.name, ev, V)
    assert np.all(np.diff(ev64) >= 0), (case.name, ev)
    tol = EVAL_REL * np.abs(case.lam) + EVAL_ABS * lmax
    err = np.abs(ev64 - case.lam)
    assert np.all(err <= tol), (case.name, "eigenvalues", ev64, case.lam, err, tol)
    ortho = float(np.abs(V64.T @ V64 - np.eye(3)).max())
    assert ortho <= ORTHO, (case.name, "orthonormality", ortho)
    worst_angle = 0.0
    for i in range(3):
        if case.simple[i]:
            a = unsigned_angle(V64[:, i], case.V[:, i])
            bound = ANGLE_ABS + EVAL_ABS * lmax / case.gap[i]
            assert a <= bound, (case.name, "angle of column %d" % i, a, bound)
            worst_angle = max(worst_angle, a / bound)
    if case.cls in BY_RESIDUAL:
        res = np.abs(Mf @ V64 - V64 * ev64[None, :]).max(axis=0)
        assert np.all(res <= RESIDUAL * lmax), (case.name, "residual", res, RESIDUAL * lmax)
    if case.cls == ZERO:
        assert np.all(ev64 == 0.0), (case.name, ev)
    return float((err / np.where(tol > 0, tol, 1.0)).max()), worst_angle, ortho


def column_dots(Va, Vb):
    return (np.asarray(Va, np.float64) * np.asarray(Vb, np.float64)).sum(axis=0)


# ------------------------------------------------------------------ exact characteristic polynomial (CPU tests)

def charpoly(M):
    """det(x I - M) of an integer symmetric 3x3 as a function on Fractions."""
    a, b, c = int(M[0, 0]), int(M[0, 1]), int(M[0, 2])
    d, e, f = int(M[1, 1]), int(M[1, 2]), int(M[2, 2])
    c2 = -(a + d + f)
    c1 = a * d + a * f + d * f - b * b - c * c - e * e
    c0 = -(a * (d * f - e * e) - b * (b * f - e * c) + c * (b * e - d * c))

    def p(x):
        x = Fraction(x)
        return ((x + c2) * x + c1) * x + c0
    return p
