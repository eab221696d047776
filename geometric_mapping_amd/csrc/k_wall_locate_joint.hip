// k_wall_locate_joint.hip -- BUILD-DEFINED EXTENSION: a frame's pose corrected against a wall alignment
// (gm_wall_alignment_locate_*), the device side.  The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is
// tests/wall_alignment_locate_np.py.
//
// Shape: k_wall_locate's (the cylinder regression's): one streaming launch per pass, three per locate, on the FIXED grid
// kFitBlocks x kFitThreads with the 4-point unroll, fit_block_reduce, the ticket, and the solve by thread 0 of the block
// that finished last.  What differs is the point: it is given its owner by the joint planes of the pass (gm_wall_joint.hpp's
// rule, the planes in LDS) and runs that side's chain alone -- a loop over the sides that is wave-uniform, with a
// wave-uniform switch on the side's axis in front of surf_rho, arc_chain and clothoid_chain (gm_device.hpp); the side's
// block is read through uniform addresses and stays in scalar registers.  The chain yields e, t and the unit radial
// direction nrm in sensor coordinates, from which the row J of the four parameters at the home section follows in fp64.
// The state is the home section (c, d, u', v'), fp64 in WallLocateJointWork; every side's block and every joint plane is
// attached to it rigidly (h, its coordinates in the home section): pass 0 takes their fp32 images in the launch arguments,
// and the solve of pass k writes those of pass k + 1 beside the state.  No host round trip between the passes; no atomics
// but the ticket.  In MAP mode a point gathers count and sum of its cell from its OWNER's table.
// Measured: 45 us per pass of the 1 M-point frame on an arc side, 54 us on a clothoid side (fifteen sincos per
// point), 33 us for k_wall_locate on a straight map: 17 B per point and pass, so none of them is bound by HBM.
#include <math.h>

#include "gm_wall_joint.hpp"   // the grid, the planes, the owner rule
#include "gm_wall_locate.hpp"

namespace gm {

constexpr int kLocSides = GM_WALL_JOINT_MAX_SIDES;

// the state a pass starts from: pass 0 the launch's arguments, later passes the work block
__device__ __forceinline__ void locj_state(const WallLocateJointArgs &a, int pass, double (&c)[3], double (&d)[3], double (&u)[3], double (&v)[3])
{
    const WallLocateJointWork *wk = a.work;
    if (pass == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { c[k] = a.c0[k]; d[k] = a.d0[k]; u[k] = a.u0[k]; v[k] = a.v0[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { c[k] = wk->c[k]; d[k] = wk->d[k]; u[k] = wk->u[k]; v[k] = wk->v[k]; }
    }
}

// The solve of a pass on the reduced row (one thread, fp64): the pass record, the solve, the update of the state and of
// the attached blocks.
__device__ __forceinline__ void locj_solve(const WallLocateJointArgs &a, int pass, uint32_t n, const double *tot, const double (&c)[3],
                                  const double (&d)[3], const double (&u)[3], const double (&v)[3], float gate,
                                  const WallLocateJointBlocks &blk)
{
    WallLocateJointWork *wk = a.work;
    const double nan = __builtin_nan("");
    const double used = tot[kLocUsed];
    gm_wall_alignment_locate_pass &rec = wk->pass[pass];   // (written in place: 376 bytes need not live in registers)
    for (int k = 0; k < 3; ++k) { rec.o[k] = (float)c[k]; rec.a[k] = (float)d[k]; rec.u[k] = (float)u[k]; rec.v[k] = (float)v[k]; }
    rec.gate = gate;
    rec.plane = (uint32_t)tot[kLocPlane];
    rec.outside = (uint32_t)tot[kLocOutside];
    rec.unsurveyed = (uint32_t)tot[kLocUnsurveyed];
    rec.gated = (uint32_t)tot[kLocGated];
    rec.used = (uint32_t)used;
    rec.rms = used > 0.0 ? sqrt(tot[kLocRes2] / used) : nan;
    for (int k = 0; k < 4; ++k) rec.step[k] = nan;
    for (int s = 0; s < kLocSides; ++s)
        for (int k = 0; k < 12; ++k) rec.side[s][k] = blk.side[s][k];
    for (int j = 0; j < kLocSides - 1; ++j)
        for (int k = 0; k < 3; ++k) { rec.joint_o[j][k] = blk.planes.jo[j][k]; rec.joint_a[j][k] = blk.planes.ja[j][k]; }
    if (pass == 0) {   // the records behind a failed pass stay zero
        const gm_wall_alignment_locate_pass zero = {};
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
        for (int k = 0; k < 3; ++k) cn[k] = (c[k] + a.s0 * d[k]) + x[0] * u[k] + x[1] * v[k];   // c0, moved
        if (!loc_update(d, u, v, x, a.s0, cn, dn, un, vn, step)) status = GM_LOCATE_SINGULAR;
    }
    if (status != GM_LOCATE_OK) {   // the chain stops here: the state stays that of this pass
        wk->status = status;
        wk->passes = (uint32_t)pass;
        wk->last_step = nan;
        wk->lateral[0] = wk->lateral[1] = wk->tilt[0] = wk->tilt[1] = nan;
        if (pass == 0)
            for (int k = 0; k < 3; ++k) { wk->c[k] = c[k]; wk->d[k] = d[k]; wk->u[k] = u[k]; wk->v[k] = v[k]; }
        return;
    }
    for (int k = 0; k < 4; ++k) rec.step[k] = x[k];
    for (int k = 0; k < 3; ++k) { wk->c[k] = cn[k]; wk->d[k] = dn[k]; wk->u[k] = un[k]; wk->v[k] = vn[k]; }
    wall_locate_blocks(a, cn, dn, un, vn, wk->next);
    wk->lateral[0] += x[0]; wk->lateral[1] += x[1];
    wk->tilt[0] += x[2]; wk->tilt[1] += x[3];
    wk->last_step = step;
    wk->status = GM_LOCATE_OK;
    wk->passes = (uint32_t)pass + 1u;
}

__global__ __launch_bounds__(kFitThreads) void k_wall_locate_joint(WallLocateJointArgs a, int pass)
{
    __shared__ double tot[kFitCols];
    // the joint planes, read per point from LDS (a broadcast), as in k_wall_add_joint: the scalar registers go to the
    // owner's block
    __shared__ JointPlaneLds s_plane;
    __shared__ double s_home[9];   // c0, u, v
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    const WallLocateJointWork *wk = a.work;
    if (pass > 0 && wk->status != GM_LOCATE_OK) return;   // the chain has failed (uniform over the grid)
    // the blocks of this pass: uniform addresses, in the arguments or behind the state
    const WallLocateJointBlocks &blk = pass == 0 ? a.first : wk->next;
    if (threadIdx.x == 0) {
        double c[3], d[3], u[3], v[3];
        locj_state(a, pass, c, d, u, v);
        // (a call per branch: through blk, a select of two pointers, the whole argument block goes to private memory)
        if (pass == 0) joint_planes_store(s_plane, a.first.planes);
        else joint_planes_store(s_plane, wk->next.planes);
        // the pass's fp32 state, as fp64, and c0 = o + s0 a: what J is taken against (LDS too: eighteen scalar registers)
        for (int k = 0; k < 3; ++k) {
            s_home[k] = (double)(float)c[k] + a.s0 * (double)(float)d[k];
            s_home[3 + k] = (double)(float)u[k];
            s_home[6 + k] = (double)(float)v[k];
        }
    }
    __syncthreads();
    const float gate = (float)(a.gate * (1.0 / (double)(1 << pass)));
    const bool map_mode = a.reference == (uint32_t)GM_WALL_LOCATE_MAP;
    const float R = a.grid.R, ds = a.grid.station_length, two_pi = a.grid.two_pi, dtheta = a.grid.sector_angle;
    const uint32_t nsec = a.grid.n_sectors, min_count = a.min_count, nside = a.n_sides;
    const float inf = __builtin_inff();

    double s[kLocAcc];
#pragma unroll
    for (int k = 0; k < kLocAcc; ++k) s[k] = 0.0;
    // gated, outside and unsurveyed in 21-bit fields of one word (a thread sees at most 2^32 / (kFitBlocks kFitThreads) =
    // 2^15 points): three counters selected by the class become an indexed array in private memory otherwise
    uint32_t n_plane = 0u, n_used = 0u;
    unsigned long long n_cls = 0ull;
    auto accumulate = [&](const float4 p, uint32_t lab, uint32_t i) {
        // without the guard on the plan's joints: a joint the plan does not have is attached as h = 0, so its aJ' is
        // (0, 0, 0) in every pass, its d is 0 or a NaN and never < 0 -- three uniform conditions less in the scalar file
        const uint32_t owner = joint_owner<false>(p, s_plane, nside);
        float res = __builtin_nanf("");
        int cell = -1;
        int32_t element = 0;
#pragma unroll 1
        for (uint32_t sd = 0; sd < nside; ++sd) {   // sd is uniform: the side's block is read once per wave
            if (owner != sd) continue;
            const WallLocateJointSide &S = a.side[sd];
            element = S.element;
            if (lab == 1u) {
                ++n_plane;
                continue;
            }
            const float(&B)[12] = blk.side[sd];
            const float o[3] = {B[0], B[1], B[2]}, ax[3] = {B[3], B[4], B[5]};
            const float nv[3] = {B[6], B[7], B[8]}, bv[3] = {B[9], B[10], B[11]};   // (straight: u', v')
            float t, e, rho, nx, ny, nz;
            float yc = 0.0f, z = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;
            bool guard = true;
            if (S.axis == kAxisStraight) {
                (void)surf_rho(p, o, ax, t, wx, wy, wz);   // t, w; the root again, rounded to nearest as on the curved sides
                rho = sqrt_rn(__fmaf_rn(wx, wx, __fmaf_rn(wy, wy, __fmul_rn(wz, wz))));
                e = __fsub_rn(rho, R);
                const float inv = __frcp_rn(rho);
                nx = __fmul_rn(wx, inv); ny = __fmul_rn(wy, inv); nz = __fmul_rn(wz, inv);
            } else {
                float cs, sn, g;
                if (S.axis == kAxisClothoid) e = clothoid_chain(p, o, ax, nv, bv, S.kappa, S.rate, R, t, yc, z, g, rho, cs, sn);
                else e = arc_chain(p, o, ax, nv, bv, S.kappa, R, t, yc, z, g, rho, cs, sn);
                guard = g > 0.0f;   // (arc: cy; clothoid: ok -- what wall_chain tests)
                const float inv = __frcp_rn(rho);
                const float tx = __fmaf_rn(cs, nv[0], -__fmul_rn(sn, ax[0]));
                const float ty = __fmaf_rn(cs, nv[1], -__fmul_rn(sn, ax[1]));
                const float tz = __fmaf_rn(cs, nv[2], -__fmul_rn(sn, ax[2]));
                nx = __fmul_rn(__fmaf_rn(yc, tx, __fmul_rn(z, bv[0])), inv);
                ny = __fmul_rn(__fmaf_rn(yc, ty, __fmul_rn(z, bv[1])), inv);
                nz = __fmul_rn(__fmaf_rn(yc, tz, __fmul_rn(z, bv[2])), inv);
            }
            float m = 0.0f;
            int cls = 0;   // 0 goes on to the gate, 1 gated, 2 outside, 3 unsurveyed
            if (!(fabsf(e) < inf) || !guard) {
                cls = 1;
            } else if (map_mode) {
                const float jl = surf_station(t, 0.0f, ds);   // relative to the owner's anchor
                const int64_t j = fabsf(jl) < 4.0e18f ? S.anchor + (int64_t)jl : -1;
                if (!(j >= 0 && j < (int64_t)S.n_stations)) {
                    cls = 2;
                } else {
                    const uint32_t kk = S.axis == kAxisStraight ? surf_sector(wx, wy, wz, nv, bv, two_pi, dtheta, nsec)
                                                                : arc_sector(yc, z, S.un, S.ub, S.vn, S.vb, two_pi, dtheta, nsec);
                    const uint32_t cc = (uint32_t)j * nsec + kk;   // < n_stations n_sectors <= 2^24: inside the owner's table
                    cell = (int)cc;
                    const uint32_t cnt = S.table.cnt[cc];
                    if (cnt < min_count) {
                        cls = 3;
                    } else {
                        const long long q = (long long)S.table.sum[cc] / (long long)cnt;
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
                    const double n0 = nx, n1 = ny, n2 = nz;
                    const double uh[3] = {s_home[3], s_home[4], s_home[5]}, vh[3] = {s_home[6], s_home[7], s_home[8]};
                    const double q0 = (double)p.x - s_home[0], q1 = (double)p.y - s_home[1], q2 = (double)p.z - s_home[2];
                    const double a1 = -(n0 * uh[0] + n1 * uh[1] + n2 * uh[2]);
                    const double a2 = -(n0 * vh[0] + n1 * vh[1] + n2 * vh[2]);
                    const double vq0 = vh[1] * q2 - vh[2] * q1, vq1 = vh[2] * q0 - vh[0] * q2, vq2 = vh[0] * q1 - vh[1] * q0;
                    const double uq0 = uh[1] * q2 - uh[2] * q1, uq1 = uh[2] * q0 - uh[0] * q2, uq2 = uh[0] * q1 - uh[1] * q0;
                    const double j3 = -(n0 * vq0 + n1 * vq1 + n2 * vq2);
                    const double j4 = n0 * uq0 + n1 * uq1 + n2 * uq2;
                    loc_sum_row(s, a1, a2, j3, j4, (double)r);
                    ++n_used;
                }
            }
            n_cls += cls ? 1ull << (21 * (cls - 1)) : 0ull;
        }
        if (a.res) {   // (stage call only, which hands over all three; i < n <= the buffers' points)
            a.res[i] = res;
            a.cell[i] = cell;
            if (pass == 0) a.element[i] = element;   // (the owner under the caller's pose: the add's)
        }
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
                p[q] = a.pts[i];
                if (a.labels) lab[q] = a.labels[i];
            }
        }
        // the loads above are in flight together; the chains run one after the other through ONE copy of the point's code (q
        // is uniform: the selects are scalar compares), which keeps the sides' blocks of four copies out of the scalar file
#pragma unroll 1
        for (int q = 0; q < kFitUnroll; ++q) {
            float4 pq = p[0];
            uint32_t lq = lab[0];
            bool iq = in[0];
#pragma unroll
            for (int r = 1; r < kFitUnroll; ++r)
                if (q == r) { pq = p[r]; lq = lab[r]; iq = in[r]; }
            if (iq) accumulate(pq, lq, i0 + (uint32_t)q * stride);
        }
    }
    s[kLocUsed] = (double)n_used;
    s[kLocPlane] = (double)n_plane;
    s[kLocGated] = (double)(uint32_t)(n_cls & 0x1FFFFFu);
    s[kLocOutside] = (double)(uint32_t)((n_cls >> 21) & 0x1FFFFFu);
    s[kLocUnsurveyed] = (double)(uint32_t)((n_cls >> 42) & 0x1FFFFFu);
    if (!fit_block_reduce<kLocAcc>(a.partial, a.ticket, s, tot)) return;
    if (threadIdx.x != 0) return;
    double c[3], d[3], u[3], v[3];   // (read again: twelve fp64 values need not stay in scalar registers through the loop)
    locj_state(a, pass, c, d, u, v);
    locj_solve(a, pass, n, tot, c, d, u, v, gate, blk);
}

void launch_wall_locate_joint(const WallLocateJointArgs &a, hipStream_t s)
{
    for (int pass = 0; pass < GM_LOCATE_PASSES; ++pass)
        hipLaunchKernelGGL(k_wall_locate_joint, dim3(kFitBlocks), dim3(kFitThreads), 0, s, a, pass);
}

}  // namespace gm
