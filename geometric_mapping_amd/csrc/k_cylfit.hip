// k_cylfit.hip -- BUILD-DEFINED EXTENSION: least-squares regression of the RANSAC cylinder (GM_CFG_CYLINDER_FIT).
//
// The reference declares getCylinder (/root/reference include/geometric_mapping/tunnel_processing.hpp:56-59) and leaves
// its body empty under "//Regression function" (src/tunnel_processing.cpp:149-154).  This is that regression: three
// Gauss-Newton passes (gates 4 tau, 2 tau, tau) from the frame's winning hypothesis, then one label pass at tau with the
// RANSAC's own inlier predicate (cyl_inlier).  The algorithm is stated in include/gm_hip.h and DESIGN.md; the CPU twin
// is tests/cylfit_np.py.
//
// Shape: one streaming launch per pass, 4 per frame, on a FIXED grid (kFitBlocks x 256): a thread's points and the order
// of every sum do not depend on the point count or on the launch site, so the frame pipeline, a replayed graph and the
// gm_fit_cylinder stage call give the same bits.  A block sums its points in fp64 registers (22 accumulators of a GN
// pass, 3 of the label pass), reduces them through wave_sum and LDS, and writes one partial row to its own slot; the
// block that takes the last ticket reduces the rows of the grid in a fixed order, solves the 5x5 system (fp64 Cholesky,
// one thread), writes the next model to CylFitWork and resets the ticket.  No host round trip; the point count is the
// device word n_valid in the frame.  Bound: HBM (17 B per eligible point per GN pass, 18 B per label pass).
//
// Sharded frame (gm_group_fit_cylinder, gm_group.hip): the same launches on every rank's resident valid cloud with
// CylFitArgs.rank_row set -- the last block writes the rank's reduced row to the exchange instead of solving -- then,
// after the rows are gathered, k_cylfit_merge (one block per rank) sums them in rank order and runs the same solve or
// finish.  Those are __device__ functions shared with the single-device last block, so one rank gives its bits.
#include <math.h>

#include "gm_fit_reduce.hpp"
#include "gm_internal.hpp"

namespace gm {

constexpr int kFitAcc = 22;

__device__ inline bool fit_eligible(const uint8_t *__restrict__ labels, uint32_t i, uint32_t want, uint32_t want2)
{
    if (!labels) return true;
    const uint32_t l = labels[i];
    return l == want || l == want2;
}

// failure: NaN parameters, the RANSAC's labels stay (the label pass returns early on a failed status)
__device__ inline void fit_fail(const CylFitArgs &a, uint32_t status, uint32_t passes)
{
    const double nan = __builtin_nan("");
    a.work->status = status;
    a.work->passes = passes;
    a.work->last_step = nan;
    gm_cylinder_fit f;
    f.struct_size = (uint32_t)sizeof(gm_cylinder_fit);
    f.status = status;
    f.inliers = 0;
    f.passes = passes;
    for (int k = 0; k < 3; ++k) { f.point[k] = nan; f.axis[k] = nan; }
    f.radius = nan; f.rms = nan; f.last_step = nan;
    for (int k = 0; k < 7; ++k) f.model[k] = __builtin_nanf("");
    *a.fit = f;
}

// the model a pass starts from: pass 0 the starting row (its failure is published by block 0), later passes CylFitWork.
// Returns false when there is nothing to do (uniform over the grid: every thread reads the same words).
__device__ inline bool fit_start(const CylFitArgs &a, int pass, double (&c)[3], double (&d)[3], double &r, double (&dh)[3])
{
    if (pass == 0) {
        const uint32_t h = a.best ? a.best[0] : 0u;
        bool ok = h != 0xFFFFFFFFu;
        if (ok) {
            const float *row = a.init + 8 * (size_t)h;
            for (int k = 0; k < 3; ++k) { c[k] = row[k]; d[k] = row[3 + k]; }
            r = row[6];
            const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            ok = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(r) && isfinite(dn) && dn > 0.0;
            if (ok)
                for (int k = 0; k < 3; ++k) { d[k] /= dn; dh[k] = d[k]; }
        }
        if (!ok) {
            if (blockIdx.x == 0 && threadIdx.x == 0) fit_fail(a, GM_FIT_NO_MODEL, 0u);
            return false;
        }
    } else {
        if (a.work->status != GM_FIT_OK) return false;   // (uniform: written by the last block of the launch before)
        for (int k = 0; k < 3; ++k) { c[k] = a.work->c[k]; d[k] = a.work->d[k]; dh[k] = a.work->d_hyp[k]; }
        r = a.work->r;
    }
    return true;
}

// The solve of a Gauss-Newton pass on the reduced sums tot[0..kFitAcc) (one thread, fp64): re-centre, 5x5 normal
// equations, Cholesky, update.  The last block of k_cylfit_gn and k_cylfit_merge run this same code.
__device__ inline void fit_solve(const CylFitArgs &a, int pass, const double *tot, const double (&c)[3], const double (&d)[3],
                                 double r, const double (&dh)[3], const double (&e1)[3], const double (&e2)[3])
{
    const double cnt = tot[14];
    if (!(cnt >= 5.0)) { fit_fail(a, GM_FIT_DEGENERATE, (uint32_t)pass); return; }
    const double tb = tot[21] / cnt;   // c -> foot of the gated points' mean t: the tilt columns become (t - tb) a_k
    double M[5][5], g[5];
    {
        const double A[4][4] = {{tot[0], tot[1], tot[2], tot[3]}, {tot[1], tot[4], tot[5], tot[6]},
                                {tot[2], tot[5], tot[7], tot[8]}, {tot[3], tot[6], tot[8], tot[9]}};
        double F[5][5];
        for (int i = 0; i < 4; ++i) {
            for (int j = 0; j < 4; ++j) F[i][j] = A[i][j];
            F[i][4] = F[4][i] = -tot[10 + i];
        }
        F[4][4] = cnt;
        const double G[5] = {tot[15], tot[16], tot[17], tot[18], -tot[19]};
        // J' = T J: rows 2, 3 of T subtract tb times rows 0, 1
        double TF[5][5];
        for (int j = 0; j < 5; ++j) {
            TF[0][j] = F[0][j]; TF[1][j] = F[1][j]; TF[4][j] = F[4][j];
            TF[2][j] = F[2][j] - tb * F[0][j];
            TF[3][j] = F[3][j] - tb * F[1][j];
        }
        for (int i = 0; i < 5; ++i) {
            M[i][0] = TF[i][0]; M[i][1] = TF[i][1]; M[i][4] = TF[i][4];
            M[i][2] = TF[i][2] - tb * TF[i][0];
            M[i][3] = TF[i][3] - tb * TF[i][1];
        }
        g[0] = G[0]; g[1] = G[1]; g[4] = G[4];
        g[2] = G[2] - tb * G[0];
        g[3] = G[3] - tb * G[1];
    }
    // Cholesky M = L L^T (lower triangle in place); a pivot that is not positive relative to its diagonal is singular
    for (int k = 0; k < 5; ++k) {
        const double diag = M[k][k];
        double piv = diag;
        for (int j = 0; j < k; ++j) piv -= M[k][j] * M[k][j];
        if (!(piv > 1e-12 * diag) || !isfinite(piv)) { fit_fail(a, GM_FIT_SINGULAR, (uint32_t)pass); return; }
        const double l = sqrt(piv);
        M[k][k] = l;
        for (int i = k + 1; i < 5; ++i) {
            double v = M[i][k];
            for (int j = 0; j < k; ++j) v -= M[i][j] * M[k][j];
            M[i][k] = v / l;
        }
    }
    double y[5], x[5];
    for (int i = 0; i < 5; ++i) {
        double v = -g[i];
        for (int j = 0; j < i; ++j) v -= M[i][j] * y[j];
        y[i] = v / M[i][i];
    }
    for (int i = 4; i >= 0; --i) {
        double v = y[i];
        for (int j = i + 1; j < 5; ++j) v -= M[j][i] * x[j];
        x[i] = v / M[i][i];
    }
    double cn[3], dn[3];
    for (int k = 0; k < 3; ++k) {
        cn[k] = c[k] + tb * d[k] + x[0] * e1[k] + x[1] * e2[k];
        dn[k] = d[k] + x[2] * e1[k] + x[3] * e2[k];
    }
    const double dl = sqrt(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]);
    const double step = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4]);
    CylFitWork wk;
    for (int k = 0; k < 3; ++k) { wk.c[k] = cn[k]; wk.d[k] = dn[k] / dl; wk.d_hyp[k] = dh[k]; }
    wk.r = r + x[4];
    wk.last_step = step;
    wk.status = GM_FIT_OK;
    wk.passes = (uint32_t)pass + 1u;
    if (!isfinite(step) || !isfinite(wk.r) || !isfinite(dl)) { fit_fail(a, GM_FIT_SINGULAR, (uint32_t)pass); return; }
    *a.work = wk;
}

// One Gauss-Newton pass.  Sums (fp64) over the eligible points with |res| < gate:
//   0..9   J_i J_j, i <= j in 1..4 (11 12 13 14 22 23 24 33 34 44)      J = (a1, a2, t a1, t a2, -1), a_k = -n.e_k
//   10..13 J_i (the cross terms with the radius column are -J_i)        14 count
//   15..18 J_i res    19 res    20 res^2    21 t
__global__ __launch_bounds__(kFitThreads) void k_cylfit_gn(CylFitArgs a, int pass)
{
    __shared__ double tot[kFitCols];
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    double c[3], d[3], r, dh[3];
    if (!fit_start(a, pass, c, d, r, dh)) return;
    double e1[3], e2[3];
    fit_basis(d, e1, e2);
    const float cx = (float)c[0], cy = (float)c[1], cz = (float)c[2];
    const float dx = (float)d[0], dy = (float)d[1], dz = (float)d[2];
    const float ax = (float)e1[0], ay = (float)e1[1], az = (float)e1[2];
    const float bx = (float)e2[0], by = (float)e2[1], bz = (float)e2[2];
    const float rf = (float)r, gate = (float)((double)(4 >> pass) * a.tau);

    double s[kFitAcc];
#pragma unroll
    for (int k = 0; k < kFitAcc; ++k) s[k] = 0.0;
    auto accumulate = [&](const float4 p) {
        const float vx = __fsub_rn(p.x, cx), vy = __fsub_rn(p.y, cy), vz = __fsub_rn(p.z, cz);
        const float t = __fmaf_rn(vx, dx, __fmaf_rn(vy, dy, __fmul_rn(vz, dz)));
        const float wx = __fmaf_rn(-t, dx, vx), wy = __fmaf_rn(-t, dy, vy), wz = __fmaf_rn(-t, dz, vz);
        const float rho = __fsqrt_rn(__fmaf_rn(wx, wx, __fmaf_rn(wy, wy, __fmul_rn(wz, wz))));
        const float res = __fsub_rn(rho, rf);
        if (!(fabsf(res) < gate) || !(rho > 0.0f)) return;   // (a NaN point fails the gate)
        const float inv = __frcp_rn(rho);
        const float nx = __fmul_rn(wx, inv), ny = __fmul_rn(wy, inv), nz = __fmul_rn(wz, inv);
        const double a1 = -(double)__fmaf_rn(nx, ax, __fmaf_rn(ny, ay, __fmul_rn(nz, az)));
        const double a2 = -(double)__fmaf_rn(nx, bx, __fmaf_rn(ny, by, __fmul_rn(nz, bz)));
        const double td = t, rs = res;
        const double j3 = td * a1, j4 = td * a2;
        s[0] += a1 * a1; s[1] += a1 * a2; s[2] += a1 * j3; s[3] += a1 * j4;
        s[4] += a2 * a2; s[5] += a2 * j3; s[6] += a2 * j4;
        s[7] += j3 * j3; s[8] += j3 * j4; s[9] += j4 * j4;
        s[10] += a1; s[11] += a2; s[12] += j3; s[13] += j4; s[14] += 1.0;
        s[15] += a1 * rs; s[16] += a2 * rs; s[17] += j3 * rs; s[18] += j4 * rs; s[19] += rs; s[20] += rs * rs;
        s[21] += td;
    };
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += kFitUnroll * stride) {
        float4 p[kFitUnroll];
        bool el[kFitUnroll];
#pragma unroll
        for (int u = 0; u < kFitUnroll; ++u) {
            const uint32_t i = i0 + (uint32_t)u * stride;
            el[u] = i < n && i >= i0 && fit_eligible(a.labels, i, a.want, a.want2);   // (i >= i0: no wrap past 2^32)
            if (el[u]) p[u] = a.pts[i];
        }
#pragma unroll
        for (int u = 0; u < kFitUnroll; ++u)
            if (el[u]) accumulate(p[u]);
    }
    if (!fit_block_reduce<kFitAcc>(a.partial, a.ticket, s, tot)) return;
    if (a.rank_row) {   // group: the rank's row goes to the exchange, k_cylfit_merge solves
        if (threadIdx.x < (uint32_t)kFitCols) a.rank_row[threadIdx.x] = tot[threadIdx.x];
        return;
    }
    if (threadIdx.x != 0) return;
    fit_solve(a, pass, tot, c, d, r, dh, e1, e2);
}

// the final model of a successful fit: (c, d, r) of CylFitWork with the axis sign of the hypothesis, and its fp32 row
__device__ inline void fit_final_model(const CylFitArgs &a, double (&c)[3], double (&d)[3], double &r, float (&row)[7])
{
    double dot = 0.0;
    for (int k = 0; k < 3; ++k) { c[k] = a.work->c[k]; d[k] = a.work->d[k]; dot += d[k] * a.work->d_hyp[k]; }
    if (dot < 0.0)
        for (int k = 0; k < 3; ++k) d[k] = -d[k];
    r = a.work->r;
    for (int k = 0; k < 3; ++k) { row[k] = (float)c[k]; row[3 + k] = (float)d[k]; }
    row[6] = (float)r;
}

// the published record from the label pass's reduced sums (count, t, res^2 of the inliers; one thread).  The last block
// of k_cylfit_label and k_cylfit_merge run this same code.
__device__ inline void fit_finish(const CylFitArgs &a, const double *tot, const double (&c)[3], const double (&d)[3], double r,
                                  const float (&row)[7])
{
    const double cnt = tot[0];
    const double tb = cnt > 0.0 ? tot[1] / cnt : 0.0;
    const double step = a.work->last_step;
    gm_cylinder_fit f;
    f.struct_size = (uint32_t)sizeof(gm_cylinder_fit);
    f.status = GM_FIT_OK | (step > GM_FIT_STEP_BOUND ? GM_FIT_NOT_CONVERGED : 0u);
    f.inliers = (uint32_t)cnt;
    f.passes = a.work->passes;
    for (int k = 0; k < 3; ++k) { f.point[k] = c[k] + tb * d[k]; f.axis[k] = d[k]; }
    f.radius = r;
    f.rms = cnt > 0.0 ? sqrt(tot[2] / cnt) : __builtin_nan("");
    f.last_step = step;
    for (int k = 0; k < 7; ++k) f.model[k] = row[k];
    *a.fit = f;
}

// The label pass at tau with the fp32 row of the final model.  Frame (mask_mode 0): an eligible point's label becomes
// 2 (inlier) or 0; label 1 and the non-eligible are not written.  Stage call (mask_mode 1): out[i] = 1 for the eligible
// inliers, 0 for every other point.  Sums count, t and res^2 of the inliers; the last block publishes the fit.
__global__ __launch_bounds__(kFitThreads) void k_cylfit_label(CylFitArgs a)
{
    __shared__ double tot[kFitCols];
    if (a.work->status != GM_FIT_OK) return;   // the labels stay the RANSAC's (a stage call's mask was cleared)
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    double c[3], d[3], r;
    float row[7];
    fit_final_model(a, c, d, r, row);
    float lo2, hi2;
    cyl_band(row[6], a.tau, lo2, hi2);
    double s[3] = {0.0, 0.0, 0.0};
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += kFitUnroll * stride) {
        float4 p[kFitUnroll];
        bool el[kFitUnroll];
#pragma unroll
        for (int u = 0; u < kFitUnroll; ++u) {
            const uint32_t i = i0 + (uint32_t)u * stride;
            el[u] = i < n && i >= i0 && fit_eligible(a.labels, i, a.want, a.want2);
            if (el[u]) p[u] = a.pts[i];
        }
#pragma unroll
        for (int u = 0; u < kFitUnroll; ++u) {
            const uint32_t i = i0 + (uint32_t)u * stride;
            if (i >= n || i < i0) continue;
            bool in = false;
            if (el[u]) {
                in = cyl_inlier(p[u].x, p[u].y, p[u].z, row[0], row[1], row[2], row[3], row[4], row[5], lo2, hi2);
                if (in) {
                    const float vx = __fsub_rn(p[u].x, row[0]), vy = __fsub_rn(p[u].y, row[1]), vz = __fsub_rn(p[u].z, row[2]);
                    const float t = __fmaf_rn(vx, row[3], __fmaf_rn(vy, row[4], __fmul_rn(vz, row[5])));
                    const float vv = __fmaf_rn(vx, vx, __fmaf_rn(vy, vy, __fmul_rn(vz, vz)));
                    const double res = (double)__fsqrt_rn(__fmaf_rn(-t, t, vv)) - (double)row[6];
                    s[0] += 1.0; s[1] += (double)t; s[2] += res * res;
                }
            }
            if (a.mask_mode) a.out[i] = in ? (uint8_t)1 : (uint8_t)0;
            else if (el[u]) a.out[i] = in ? (uint8_t)2 : (uint8_t)0;
        }
    }
    if (!fit_block_reduce<3>(a.partial, a.ticket, s, tot)) return;
    if (a.rank_row) {   // group: the rank's row goes to the exchange, k_cylfit_merge publishes
        if (threadIdx.x < (uint32_t)kFitCols) a.rank_row[threadIdx.x] = tot[threadIdx.x];
        return;
    }
    if (threadIdx.x != 0) return;
    fit_finish(a, tot, c, d, r, row);
}

// Group (gm_group_fit_cylinder): one block on every rank after the exchange of a pass.  The R rank rows (each reduced
// from its rank's kFitBlocks partial rows by fit_block_reduce, in its fixed order) are summed in rank order, starting
// from rank 0's row -- one rank reproduces the single-device sums bit for bit -- and the same solve (passes 0..2) or
// finish (pass 3) as the last block of k_cylfit_gn / k_cylfit_label runs on them.  Every rank reads the same rows and
// the same model words, so every rank writes the same bits.
__global__ __launch_bounds__(64) void k_cylfit_merge(CylFitArgs a, int pass, const double *__restrict__ rows, uint32_t R)
{
    __shared__ double tot[kFitCols];
    if (threadIdx.x < (uint32_t)kFitCols) {
        double t = rows[threadIdx.x];
        for (uint32_t q = 1; q < R; ++q) t += rows[(size_t)q * kFitCols + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass < 3) {
        double c[3], d[3], r, dh[3];
        if (!fit_start(a, pass, c, d, r, dh)) return;
        double e1[3], e2[3];
        fit_basis(d, e1, e2);
        fit_solve(a, pass, tot, c, d, r, dh, e1, e2);
    } else {
        if (a.work->status != GM_FIT_OK) return;
        double c[3], d[3], r;
        float row[7];
        fit_final_model(a, c, d, r, row);
        fit_finish(a, tot, c, d, r, row);
    }
}

void launch_cylinder_fit_pass(const CylFitArgs &a, int pass, hipStream_t s)
{
    if (pass < 3) hipLaunchKernelGGL(k_cylfit_gn, dim3(kFitBlocks), dim3(kFitThreads), 0, s, a, pass);
    else hipLaunchKernelGGL(k_cylfit_label, dim3(kFitBlocks), dim3(kFitThreads), 0, s, a);
}

void launch_cylinder_fit(const CylFitArgs &a, hipStream_t s)
{
    for (int pass = 0; pass < 4; ++pass) launch_cylinder_fit_pass(a, pass, s);
}

void launch_cylinder_fit_merge(const CylFitArgs &a, int pass, const double *rows, uint32_t n_ranks, hipStream_t s)
{
    hipLaunchKernelGGL(k_cylfit_merge, dim3(1), dim3(64), 0, s, a, pass, rows, n_ranks);
}

}  // namespace gm
