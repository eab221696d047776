"""GPU tests of the local frame's closing step: the curvature-weighted scatter sums (k_scatter_partials, k_valid_scan in
csrc/k_frame.hip), the fixed-order merge of the partial rows and the 3x3 eigen-solve (frame_finalize_block with
eig3_sym_eigen_signs, jacobi_eig3 and eigen_tridiag_qr3<float> in csrc/gm_device.hpp) and the result record.  Cases and
exact references: tests/local_frame_cases.py; tests/test_local_frame_cases_np.py shows on the CPU that the references and
the host compile of the same solvers stay inside every bound used here.

a. Exact sums.  Integer rows at curvature 0 and wf = 1000 have weight 1.0f exactly, so every product and every fp64 sum is
   an exact integer whatever the reduction order: scatter6 == the int64 sum, at every launch edge of gm_get_local_frame
   (256 rows per block, 64 blocks, 4096 rows per block, the 1024-block cap past which the grid-stride loop grows), with
   cloudSize < len(rows), with partial rows of a larger call left on the context, and through gm_compact_valid_stage with
   the drop patterns of test_gpu_valid_in_place.py.
b. Weights.  One row (1, 1, 1, c): the six entries of M are one value, the square of a float w within 1 float ulp of
   float(exp(t^2)), t = double(c) + .001/wf.  The device's fp64 exp is within an ulp or two of libm's, so the float store
   can differ only where the double sits on a float rounding tie, and then by one ulp.  wf = 1e-5 overflows w: inf and NaN
   entries as the numpy restatement gives them, GM_OK (both solvers' loops are bounded: 64 sweeps, 90 iterations).
c. Eigenpairs against the exact references, lmax the largest eigenvalue, gap_i the distance to the nearest other one:
     |lambda_dev - lambda| <= 2^-23 |lambda| + 2^-40 lmax      (one float ulp of the stored result; 4096 fp64 epsilons for
                                                                 the Jacobi iteration's backward error)
     unsigned angle to the exact eigenvector <= 2^-22 + 2^-40 lmax / gap_i     (simple eigenvalues)
     |V^T V - I| <= 2^-21;  degenerate classes: every column's residual |M v - lambda_dev v| <= 2^-21 lmax
     n = 0 and all-zero rows: M == 0, eigenvalues == 0, V orthonormal.
d. Signs.  The device's columns against the f32-faithful oracle's (rows in, Eigen's float tridiagonal-QR solve restated)
   and against gm_solve_local_frame on the M the device returned: every column dot > 0.999, on every separated case: of
   the sweep every draw whose gaps are at least 2^-18 of the largest eigenvalue (tests/local_frame_cases.py derives the
   bar and counts the draws below it, which c holds by their residuals).  None of those is skipped.
e. The frame's own paths (k_frame_finalize on the compaction's rows, the tail of k_ext_finalize, two slots): the frame's
   eigenpairs against gm_solve_local_frame of the frame's scatter6, signs included; center_axis is eigenvectors[:, 0].
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_frame_cases as lf  # noqa: E402
import test_gpu_valid_in_place as vip  # noqa: E402

pytestmark = pytest.mark.gpu

WF = lf.WF_EXACT
CAP = 1024 * 4096                       # kScatterBlocks blocks of 4096 rows: 16 whole grid-stride trips per thread
N_BIG = CAP + 4097                      # past the cap: a 17th trip for the first 4097 threads, the 4097th in a second block
SIZES = (1, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 262143, 262144, 262145, 266241, CAP, N_BIG)
SEQUENCE = ((N_BIG, 0), (257, 1), (0, 2), (16385, 3))   # (n, row rule) per call on one context


@pytest.fixture(scope="module")
def ctx(gm):
    c = gm.GeometricMapping(weightingFactor=WF)
    yield c
    c.close()


def frame_of(c, n, rule, wf=WF):
    rows = lf.rule_rows(n, rule)
    ev, V, M = c.getLocalFrame(n, wf, rows)
    return ev, V, lf.six(M)


# ------------------------------------------------------------------ a. exact sums

@pytest.fixture(scope="module")
def sequence(gm):
    """The calls of SEQUENCE on one context; the first is also the exact-sum case of N_BIG (uploaded once)."""
    with gm.GeometricMapping(weightingFactor=WF) as c:
        return [frame_of(c, n, rule) for n, rule in SEQUENCE]


@pytest.mark.parametrize("n", SIZES)
def test_exact_sums_at_launch_edges(ctx, sequence, n):
    sc = sequence[0][2] if n == N_BIG else frame_of(ctx, n, 0)[2]
    ref = lf.rule_sum(n, 0)
    assert np.array_equal(sc, ref.astype(np.float64)), (n, sc, ref)
    assert np.array_equal(sc.astype(np.int64), ref)


@pytest.mark.parametrize("size,total", [(256, 300), (4096, 4097), (0, 5), (1, 2)])
def test_cloud_size_below_the_rows_given(ctx, size, total):
    rows = lf.rule_rows(total, 0)
    rows[size:, :3] += 100.0           # a row read past cloudSize cannot hide
    _, _, M = ctx.getLocalFrame(size, WF, rows)
    assert np.array_equal(lf.six(M), lf.rule_sum(size, 0).astype(np.float64))


def test_no_stale_partial_rows_on_one_context(gm, sequence):
    """1024 partial rows, then 2, 1 and 64 on the same context: each call equals the same call on a
    fresh context bit for bit, eigenpairs included, and the exact sum."""
    for (n, rule), got in zip(SEQUENCE, sequence):
        assert np.array_equal(got[2], lf.rule_sum(n, rule).astype(np.float64)), (n, rule)
        if n == N_BIG:
            continue                   # (the first call of its context: it is the fresh one)
        with gm.GeometricMapping(weightingFactor=WF) as fresh:
            f = frame_of(fresh, n, rule)
        for a, b in zip(got, f):
            assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                  b.view(np.uint32 if b.dtype == np.float32 else np.uint64)), (n, rule, a, b)


_VALID = vip.exact_cases(4096)


@pytest.mark.parametrize("name,n,drops", _VALID, ids=[c[0] for c in _VALID])
def test_exact_sums_through_compact_valid(ctx, name, n, drops):
    """test_gpu_valid_in_place.py's drop patterns with the integer rule on the surviving rows: == where that file allows
    5e-7."""
    rows, nrm = vip.make_rows(n, drops)
    mask = np.isfinite(nrm[:, :3]).all(axis=1)
    assert int((~mask).sum()) == len(drops)
    exact = lf.rule_rows(n, 0)
    nrm[mask] = exact[mask]                                    # the dropped rows keep their NaN and inf components
    out, on, sc = ctx.compactValid(WF, rows, nrm)
    assert np.array_equal(out.view(np.uint32), rows[mask].view(np.uint32))
    assert np.array_equal(on.view(np.uint32), nrm[mask].view(np.uint32))
    ref = lf.six(lf.scatter_int(exact[mask][:, :3].astype(np.int64)))
    assert np.array_equal(sc, ref.astype(np.float64)), (name, sc, ref)


# ------------------------------------------------------------------ b. weights

CURVATURES = (0.0, 1e-7, 1e-3, 0.01, 0.1, 0.25, 1.0 / 3.0, 0.5, -0.005, -0.1)
FACTORS = (0.2, -0.2, 0.01, 1e-3, 1000.0)


@pytest.mark.parametrize("wf", FACTORS)
def test_weight_of_one_row(ctx, wf):
    for c in CURVATURES:
        row = np.array([[1.0, 1.0, 1.0, c]], np.float32)
        _, _, M = ctx.getLocalFrame(1, wf, row)
        sc = lf.six(M)
        assert np.all(sc == sc[0]), (c, wf, sc)
        w = np.float32(np.sqrt(sc[0]))
        assert np.float64(w) * np.float64(w) == sc[0], (c, wf, sc[0])          # the square of a float
        t = np.float64(row[0, 3]) + 0.001 / wf
        ref = np.float32(np.exp(t * t))
        ulps = abs(int(w.view(np.int32)) - int(ref.view(np.int32)))
        print("c=%g wf=%g w=%.9g libm=%.9g ulps=%d" % (c, wf, w, ref, ulps))
        assert ulps <= 1, (c, wf, w, ref)


def test_weight_overflow(ctx):
    nrm = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    _, _, M = ctx.getLocalFrame(1, 1e-5, nrm)          # returns: GM_OK
    sc = lf.six(M)
    with np.errstate(all="ignore"):
        ref = vip.scatter_ref(nrm, 1e-5)
    assert sc[0] == np.inf and np.all(np.isnan(sc[1:]))
    assert ref[0] == np.inf and np.array_equal(np.isnan(sc), np.isnan(ref))


# ------------------------------------------------------------------ c, d. eigenpairs and signs

@pytest.fixture(scope="module")
def cases():
    known, structured, sweep = lf.known_cases(), lf.structured_cases(), lf.sweep_cases()
    return dict(known=known, structured=structured, sweep=sweep,
                signed=[c for c in known + structured + sweep if c.cls == lf.SEPARATED])


@pytest.fixture(scope="module")
def device(ctx, cases):
    """name -> (eigenvalues, eigenvectors, M) from gm_get_local_frame, once for every case."""
    out = {}
    for c in cases["known"] + cases["structured"] + cases["sweep"]:
        out[c.name] = ctx.getLocalFrame(len(c.rows), WF, c.normals)
    return out


def run_checks(group, device):
    bad, worst = [], [0.0, 0.0, 0.0]
    for c in group:
        ev, V, M = device[c.name]
        try:
            assert np.array_equal(M, c.M.astype(np.float64)), (c.name, "scatter", M)
            f = lf.check_eigenpairs(c, ev, V)
            worst = [max(a, b) for a, b in zip(worst, f)]
        except AssertionError as e:
            bad.append(str(e)[:300])
    print("%d cases: eigenvalue error / bound %.3f, angle / bound %.3f, |V^T V - I| %.3g (bound %.3g); %d failed"
          % (len(group), worst[0], worst[1], worst[2], lf.ORTHO, len(bad)))
    assert not bad, (len(bad), bad[:10])


def test_eigenpairs_separated_known_spectra(cases, device):
    run_checks([c for c in cases["known"] if c.cls == lf.SEPARATED] + cases["structured"], device)


def test_eigenpairs_sweep(cases, device):
    run_checks(cases["sweep"], device)


@pytest.mark.parametrize("cls", lf.DEGENERATE)
def test_eigenpairs_degenerate(cases, device, cls):
    group = [c for c in cases["known"] if c.cls == cls]
    assert group
    run_checks(group, device)


def sign_failures(group, device, reference):
    bad, low = [], 1.0
    for c in group:
        d = lf.column_dots(device[c.name][1], reference(c))
        low = min(low, float(np.abs(d).min()))
        if not np.all(d > lf.SIGN_DOT):
            bad.append((c.name, [round(float(x), 6) for x in d]))
    print("%d cases, smallest |column dot| %.9f, %d failed" % (len(group), low, len(bad)))
    return bad


def test_signs_against_the_f32_faithful_oracle(cases, device, oc):
    bad = sign_failures(cases["signed"], device, lambda c: oc.local_frame(c.normals, WF, oc.F32_FAITHFUL)[1])
    assert not bad, (len(bad), bad[:20])


def test_signs_against_the_host_solve(cases, device, gm):
    bad = sign_failures(cases["signed"], device, lambda c: gm.solve_local_frame(lf.six(device[c.name][2]))[1])
    assert not bad, (len(bad), bad[:20])


def test_signs_on_the_contraction_sensitive_indices(cases, device, gm, oc):
    """The sweep cases on which an FMA-contracted and a product-rounding build of the float solve disagree on the CPU."""
    group = [cases["sweep"][i] for i in lf.CONTRACTION_SENSITIVE]
    bad = sign_failures(group, device, lambda c: oc.local_frame(c.normals, WF, oc.F32_FAITHFUL)[1])
    bad += sign_failures(group, device, lambda c: gm.solve_local_frame(lf.six(device[c.name][2]))[1])
    assert not bad, (len(bad), bad)


def test_device_and_host_solves_agree_on_the_sweep(cases, device, gm):
    """With the float solve rounding every product on both sides of the compile, the sign rule runs one float sequence on
    device and host.  The fp64 Jacobi pairs are within the bounds of c on both; printed: how many cases are bit-equal."""
    equal = 0
    for c in cases["sweep"]:
        ev, V, M = device[c.name]
        hev, hV = gm.solve_local_frame(lf.six(M))
        equal += int(np.array_equal(ev.view(np.uint32), hev.view(np.uint32)) and
                     np.array_equal(V.view(np.uint32), hV.view(np.uint32)))
        assert np.all(np.abs(ev.astype(np.float64) - hev) <= lf.EVAL_REL * np.abs(hev) + lf.EVAL_ABS * c.lam[2]), c.name
    print("device == host bit for bit on %d of %d sweep cases" % (equal, len(cases["sweep"])))


# ------------------------------------------------------------------ e. the frame's own paths

def check_frame_result(gm, res):
    ev, V = res["eigenvalues"], res["eigenvectors"]
    hev, hV = gm.solve_local_frame(res["scatter6"])
    lmax = float(hev[2])
    assert lmax > 0 and res["n_valid"] > 1000
    err = np.abs(ev.astype(np.float64) - hev.astype(np.float64))
    assert np.all(err <= lf.EVAL_REL * np.abs(hev) + lf.EVAL_ABS * lmax), (ev, hev)
    d = lf.column_dots(V, hV)
    assert np.all(d > lf.SIGN_DOT), d
    assert np.array_equal(res["center_axis"].view(np.uint32), V[:, 0].copy().view(np.uint32))
    return d


@pytest.fixture(scope="module")
def tunnels():
    from geometric_mapping_amd import synth
    return [synth.tunnel_frame(5000, seed) for seed in (0, 1, 2)]


def test_frame_without_ransac(gm, tunnels):
    with gm.GeometricMapping() as c:
        for xyz in tunnels:
            check_frame_result(gm, c.process_frame(xyz))


def test_frame_with_ransac_tail(gm, tunnels):
    from geometric_mapping_amd import _lib
    flags = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_PLANE | _lib.GM_CFG_RANSAC_CYLINDER
    with gm.GeometricMapping(flags=flags) as c:
        for xyz in tunnels:
            check_frame_result(gm, c.process_frame(xyz))


def test_frame_two_slots(gm, tunnels):
    with gm.GeometricMapping(n_slots=2) as c:
        c.submit_frame(0, tunnels[0])
        c.submit_frame(1, tunnels[1])
        check_frame_result(gm, c.wait_frame(0))
        c.submit_frame(0, tunnels[2])
        check_frame_result(gm, c.wait_frame(1))
        check_frame_result(gm, c.wait_frame(0))
