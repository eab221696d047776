// k_wall_locate.hip -- BUILD-DEFINED EXTENSION: a frame's pose corrected against the wall map (gm_wall_map_locate_*), the
// device side.  The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_locate_np.py.
//
// Shape: the cylinder regression's (k_cylfit.hip).  One streaming launch per pass, three per locate, on the FIXED grid
// kFitBlocks x kFitThreads with the 4-point unroll: a thread's points and the order of every sum depend on neither the
// point count nor the launch site, so the frame path and the stage call give the same bits.  A thread runs the add's fp32
// chain (gm_device.hpp) on its points against the state of the pass, sums the 16 fp64 terms of the 4-parameter normal
// equations of the used ones and counts the other classes; fit_block_reduce (gm_fit_reduce.hpp) brings the grid's rows
// together in a fixed order, and thread 0 of the block that took the last ticket solves the 4x4 system (fp64 Cholesky),
// moves the fp64 state in WallLocateWork and writes the pass record.  No host round trip between the passes; the point
// count is the device word n_valid.  In MAP mode a point gathers count (4 B) and sum (8 B) of its cell straight from the
// map's table: the cells a frame reaches are a window of a few hundred KiB that stays in L2.  No atomics but the ticket.
// Bound: HBM (17 B per point and pass, 12 B more from L2 in MAP).
#include <math.h>

#include "gm_wall_locate.hpp"

namespace gm {

// the state a pass starts from: pass 0 the launch's arguments, later passes WallLocateWork.  Returns false when the
// chain has failed (uniform over the grid: every thread reads the same word, written by the launch before).
__device__ inline bool loc_start(const WallLocateArgs &a, int pass, double (&c)[3], double (&d)[3], double (&u)[3], double (&v)[3])
{
    if (pass == 0) {
        for (int k = 0; k < 3; ++k) { c[k] = a.c0[k]; d[k] = a.d0[k]; u[k] = a.u0[k]; v[k] = a.v0[k]; }
        return true;
    }
    if (a.work->status != GM_LOCATE_OK) return false;
    for (int k = 0; k < 3; ++k) { c[k] = a.work->c[k]; d[k] = a.work->d[k]; u[k] = a.work->u[k]; v[k] = a.work->v[k]; }
    return true;
}

// The solve of a pass on the reduced row (one thread, fp64): the pass record, the 4x4 normal equations, Cholesky, the
// update of the state.
__device__ inline void loc_solve(const WallLocateArgs &a, int pass, uint32_t n, const double *tot, const double (&c)[3],
                                 const double (&d)[3], const double (&u)[3], const double (&v)[3], float gate)
{
    WallLocateWork *wk = a.work;
    const double nan = __builtin_nan("");
    const double used = tot[kLocUsed];
    gm_wall_locate_pass rec;
    for (int k = 0; k < 3; ++k) { rec.o[k] = (float)c[k]; rec.a[k] = (float)d[k]; rec.u[k] = (float)u[k]; rec.v[k] = (float)v[k]; }
    rec.gate = gate;
    rec.plane = (uint32_t)tot[kLocPlane];
    rec.outside = (uint32_t)tot[kLocOutside];
    rec.unsurveyed = (uint32_t)tot[kLocUnsurveyed];
    rec.gated = (uint32_t)tot[kLocGated];
    rec.used = (uint32_t)used;
    rec.rms = used > 0.0 ? sqrt(tot[kLocRes2] / used) : nan;
    for (int k = 0; k < 4; ++k) rec.step[k] = nan;
    if (pass == 0) {   // the records behind a failed pass stay zero
        const gm_wall_locate_pass zero = {};
        wk->pass[1] = zero;
        wk->pass[2] = zero;
        wk->lateral[0] = wk->lateral[1] = wk->tilt[0] = wk->tilt[1] = 0.0;
    }
    wk->n_points = n;
    wk->pad = 0u;
    double x[4];
    uint32_t status = loc_normal_solve(tot, x);
    double cn[3], dn[3], un[3], vn[3];
    double step = nan;
    if (status == GM_LOCATE_OK) {
        for (int k = 0; k < 3; ++k) cn[k] = c[k] + x[0] * u[k] + x[1] * v[k];
        if (!loc_update(d, u, v, x, a.s0, cn, dn, un, vn, step)) status = GM_LOCATE_SINGULAR;
    }
    if (status != GM_LOCATE_OK) {   // the chain stops here: the state stays that of this pass
        wk->pass[pass] = rec;
        wk->status = status;
        wk->passes = (uint32_t)pass;
        wk->last_step = nan;
        wk->lateral[0] = wk->lateral[1] = wk->tilt[0] = wk->tilt[1] = nan;
        if (pass == 0)
            for (int k = 0; k < 3; ++k) { wk->c[k] = c[k]; wk->d[k] = d[k]; wk->u[k] = u[k]; wk->v[k] = v[k]; }
        return;
    }
    for (int k = 0; k < 4; ++k) rec.step[k] = x[k];
    wk->pass[pass] = rec;
    for (int k = 0; k < 3; ++k) { wk->c[k] = cn[k]; wk->d[k] = dn[k]; wk->u[k] = un[k]; wk->v[k] = vn[k]; }
    wk->lateral[0] += x[0]; wk->lateral[1] += x[1];
    wk->tilt[0] += x[2]; wk->tilt[1] += x[3];
    wk->last_step = step;
    wk->status = GM_LOCATE_OK;
    wk->passes = (uint32_t)pass + 1u;
}

// One pass.  Sums (fp64, the columns of gm_wall_locate.hpp) over the used points: J = (a1, a2, t a1, t a2), a_k = -n.e_k
__global__ __launch_bounds__(kFitThreads) void k_wall_locate(WallLocateArgs a, int pass)
{
    __shared__ double tot[kFitCols];
    const uint32_t n = a.w.n_ptr ? *a.w.n_ptr : a.w.n_host;
    double c[3], d[3], u[3], v[3];
    if (!loc_start(a, pass, c, d, u, v)) return;
    const float of[3] = {(float)c[0], (float)c[1], (float)c[2]}, af[3] = {(float)d[0], (float)d[1], (float)d[2]};
    const float uf[3] = {(float)u[0], (float)u[1], (float)u[2]}, vf[3] = {(float)v[0], (float)v[1], (float)v[2]};
    const float gate = (float)(a.gate * (1.0 / (double)(1 << pass)));
    const bool map_mode = a.reference == (uint32_t)GM_WALL_LOCATE_MAP;
    const float R = a.w.R, ds = a.w.station_length, two_pi = a.w.two_pi, dtheta = a.w.sector_angle;
    const uint32_t nsec = a.w.n_sectors, min_count = a.min_count;
    const int64_t nst = (int64_t)a.w.n_stations, anchor = a.w.anchor;
    const uint32_t *__restrict__ t_cnt = a.w.table.cnt;
    const unsigned long long *__restrict__ t_sum = a.w.table.sum;
    const float inf = __builtin_inff();

    double s[kLocAcc];
#pragma unroll
    for (int k = 0; k < kLocAcc; ++k) s[k] = 0.0;
    uint32_t n_plane = 0u, n_outside = 0u, n_unsurveyed = 0u, n_gated = 0u, n_used = 0u;
    auto accumulate = [&](const float4 p, uint32_t lab, uint32_t i) {
        float res = __builtin_nanf("");
        int cell = -1;
        if (lab == 1u) {
            ++n_plane;
        } else {
            float t, wx, wy, wz;
            const float rho = surf_rho(p, of, af, t, wx, wy, wz);
            const float e = __fsub_rn(rho, R);
            float m = 0.0f;
            int cls = 0;   // 0 goes on to the gate, 1 gated (e not finite), 2 outside, 3 unsurveyed
            if (!(fabsf(e) < inf)) {
                cls = 1;
            } else if (map_mode) {
                const float jl = surf_station(t, 0.0f, ds);   // relative to the anchor
                const int64_t j = fabsf(jl) < 4.0e18f ? anchor + (int64_t)jl : -1;
                if (!(j >= 0 && j < nst)) {
                    cls = 2;
                } else {
                    const uint32_t kk = surf_sector(wx, wy, wz, uf, vf, two_pi, dtheta, nsec);
                    const uint32_t cc = (uint32_t)j * nsec + kk;   // < n_stations n_sectors <= 2^24: inside the table
                    cell = (int)cc;
                    const uint32_t cnt = t_cnt[cc];
                    if (cnt < min_count) {
                        cls = 3;
                    } else {
                        const long long q = (long long)t_sum[cc] / (long long)cnt;
                        m = (float)((double)q * 0x1p-20);
                    }
                }
            }
            if (cls == 0) {
                const float r = __fsub_rn(e, m);
                if (!(fabsf(r) < gate) || !(rho > 0.0f)) {
                    cls = 1;
                } else {
                    res = r;
                    const float inv = __frcp_rn(rho);
                    const float nx = __fmul_rn(wx, inv), ny = __fmul_rn(wy, inv), nz = __fmul_rn(wz, inv);
                    const double a1 = -(double)surf_dot3(nx, ny, nz, uf);
                    const double a2 = -(double)surf_dot3(nx, ny, nz, vf);
                    const double td = t, rs = r;
                    const double j3 = td * a1, j4 = td * a2;
                    loc_sum_row(s, a1, a2, j3, j4, rs);
                    ++n_used;
                }
            }
            n_gated += cls == 1 ? 1u : 0u;
            n_outside += cls == 2 ? 1u : 0u;
            n_unsurveyed += cls == 3 ? 1u : 0u;
        }
        if (a.w.res) a.w.res[i] = res;     // (stage call only; i < n <= the buffers' points)
        if (a.w.cell) a.w.cell[i] = cell;
    };
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += kFitUnroll * stride) {
        float4 p[kFitUnroll];
        uint32_t lab[kFitUnroll];
        bool in[kFitUnroll];
#pragma unroll
        for (int q = 0; q < kFitUnroll; ++q) {
            const uint32_t i = i0 + (uint32_t)q * stride;
            in[q] = i < n && i >= i0;   // (i >= i0: no wrap past 2^32)
            lab[q] = 0u;
            if (in[q]) {
                p[q] = a.w.pts[i];
                if (a.w.labels) lab[q] = a.w.labels[i];
            }
        }
#pragma unroll
        for (int q = 0; q < kFitUnroll; ++q)
            if (in[q]) accumulate(p[q], lab[q], i0 + (uint32_t)q * stride);
    }
    // a thread sees at most 2^32 / (kFitBlocks kFitThreads) points: its counts are exact in fp64, and so is every sum of them
    s[kLocUsed] = (double)n_used;
    s[kLocPlane] = (double)n_plane;
    s[kLocOutside] = (double)n_outside;
    s[kLocUnsurveyed] = (double)n_unsurveyed;
    s[kLocGated] = (double)n_gated;
    if (!fit_block_reduce<kLocAcc>(a.partial, a.ticket, s, tot)) return;
    if (threadIdx.x != 0) return;
    loc_solve(a, pass, n, tot, c, d, u, v, gate);
}

void launch_wall_locate(const WallLocateArgs &a, hipStream_t s)
{
    for (int pass = 0; pass < GM_LOCATE_PASSES; ++pass)
        hipLaunchKernelGGL(k_wall_locate, dim3(kFitBlocks), dim3(kFitThreads), 0, s, a, pass);
}

}  // namespace gm
