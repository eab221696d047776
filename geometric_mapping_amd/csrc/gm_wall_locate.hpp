// gm_wall_locate.hpp -- what the two pose corrections share on the device: k_wall_locate.hip (gm_wall_map_locate_*) and
// k_wall_locate_joint.hip (gm_wall_alignment_locate_*).  The columns of a partial row, the 4x4 solve of a pass and the
// update of the state; include/gm_hip.h states both rules.  One thread, fp64.
#pragma once
#include <math.h>

#include "gm_fit_reduce.hpp"
#include "gm_internal.hpp"

namespace gm {

// the columns of a partial row:
//   0..9   J_i J_j, i <= j in 1..4 (11 12 13 14 22 23 24 33 34 44)
//   10..13 J_i res    14 count    15 res^2    16..19 the other classes: plane, outside, unsurveyed, gated
constexpr int kLocUsed = 14, kLocRes2 = 15, kLocPlane = 16, kLocOutside = 17, kLocUnsurveyed = 18, kLocGated = 19;
constexpr int kLocAcc = 20;

__device__ inline double loc_dot(const double (&x)[3], const double (&y)[3]) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// a used point's row J, res into the thread's sums
__device__ __forceinline__ void loc_sum_row(double (&s)[kLocAcc], double a1, double a2, double j3, double j4, double rs)
{
    s[0] += a1 * a1; s[1] += a1 * a2; s[2] += a1 * j3; s[3] += a1 * j4;
    s[4] += a2 * a2; s[5] += a2 * j3; s[6] += a2 * j4;
    s[7] += j3 * j3; s[8] += j3 * j4; s[9] += j4 * j4;
    s[10] += a1 * rs; s[11] += a2 * rs; s[12] += j3 * rs; s[13] += j4 * rs;
    s[kLocRes2] += rs * rs;
}

// x = -(J^T J)^-1 J^T res on the reduced row: GM_LOCATE_OK, GM_LOCATE_DEGENERATE (fewer than 4 used points) or
// GM_LOCATE_SINGULAR (the cylinder fit's pivot rule); x stays NaN unless OK
__device__ inline uint32_t loc_normal_solve(const double *tot, double (&x)[4])
{
    const double nan = __builtin_nan("");
    for (int k = 0; k < 4; ++k) x[k] = nan;
    if (!(tot[kLocUsed] >= 4.0)) return GM_LOCATE_DEGENERATE;
    double M[4][4] = {{tot[0], tot[1], tot[2], tot[3]}, {tot[1], tot[4], tot[5], tot[6]},
                      {tot[2], tot[5], tot[7], tot[8]}, {tot[3], tot[6], tot[8], tot[9]}};
    // Cholesky M = L L^T (lower triangle in place); a pivot that is not positive relative to its diagonal is singular
    for (int k = 0; k < 4; ++k) {
        const double diag = M[k][k];
        double piv = diag;
        for (int j = 0; j < k; ++j) piv -= M[k][j] * M[k][j];
        if (!(piv > 1e-12 * diag) || !isfinite(piv)) return GM_LOCATE_SINGULAR;
        const double l = sqrt(piv);
        M[k][k] = l;
        for (int i = k + 1; i < 4; ++i) {
            double t = M[i][k];
            for (int j = 0; j < k; ++j) t -= M[i][j] * M[k][j];
            M[i][k] = t / l;
        }
    }
    double y[4];
    for (int i = 0; i < 4; ++i) {
        double t = -tot[10 + i];
        for (int j = 0; j < i; ++j) t -= M[i][j] * y[j];
        y[i] = t / M[i][i];
    }
    for (int i = 3; i >= 0; --i) {
        double t = y[i];
        for (int j = i + 1; j < 4; ++j) t -= M[j][i] * x[j];
        x[i] = t / M[i][i];
    }
    return GM_LOCATE_OK;
}

// The state moved by x: cn comes in as the translated origin (c + x0 u + x1 v, or the alignment's c0 + x0 u + x1 v) and
// goes out slid to -cn.dn = s0; dn, un, vn the turned frame; step = |x|.  false: something is not finite.
__device__ inline bool loc_update(const double (&d)[3], const double (&u)[3], const double (&v)[3], const double (&x)[4], double s0,
                                  double (&cn)[3], double (&dn)[3], double (&un)[3], double (&vn)[3], double &step)
{
    for (int k = 0; k < 3; ++k) dn[k] = d[k] + x[2] * u[k] + x[3] * v[k];
    const double dl = sqrt(loc_dot(dn, dn));
    for (int k = 0; k < 3; ++k) dn[k] /= dl;
    const double ud = loc_dot(u, dn);
    for (int k = 0; k < 3; ++k) un[k] = u[k] - ud * dn[k];
    const double ul = sqrt(loc_dot(un, un));
    for (int k = 0; k < 3; ++k) un[k] /= ul;
    vn[0] = dn[1] * un[2] - dn[2] * un[1];
    vn[1] = dn[2] * un[0] - dn[0] * un[2];
    vn[2] = dn[0] * un[1] - dn[1] * un[0];
    const double cd = loc_dot(cn, dn);
    for (int k = 0; k < 3; ++k) cn[k] = cn[k] - cd * dn[k] - s0 * dn[k];
    step = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
    bool ok = isfinite(step) && isfinite(dl) && isfinite(ul) && dl > 0.0 && ul > 0.0;
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(cn[k]) && isfinite(dn[k]) && isfinite(un[k]);
    return ok;
}

}  // namespace gm
