// gm_wall_cloud_emit.hpp -- the predicate and the emit step of the wall cloud's compaction (k_compact<WallCloudPred, ...>),
// shared by k_wall_cloud.hip (gm_wall_map_cloud) and k_wall_mesh.hip (gm_wall_map_mesh, whose vertices are the cloud's
// rows: its emit step wraps this one).  The predicate loads the block's accumulators as its payload and keeps
// count >= min_count; the emit step builds the 40-byte record at the survivor's rank in the staging buffer.  The two other
// classes are counted in LDS and added once per class and block.  The position is fp64 with explicit roundings
// (__dmul_rn / __dadd_rn: nothing the build flags could contract) on a direction table the host computed.
#pragma once

#include "gm_compact.hpp"
#include "gm_internal.hpp"

namespace gm {

// the block's counts of the two classes that do not survive: empty, below_min_count
__device__ __forceinline__ uint32_t *wc_class_counts()
{
    __shared__ uint32_t c[2];
    return c;
}

struct WallCloudPred {
    WallCloudArgs a;
    struct Payload { unsigned long long sum, count; uint32_t lo, hi, cells; };
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const
    {
        p.sum = 0ull; p.lo = 0u; p.hi = 0u;
        bool keep;
        if (a.merged) {
            p.count = a.acc_cnt[i];
            p.cells = a.acc_cells[i];
            keep = p.count >= (unsigned long long)a.min_count;   // (min_count >= 1: an empty block never passes)
            if (keep) { p.sum = a.acc_sum[i]; p.lo = a.acc_lo[i]; p.hi = a.acc_hi[i]; }
        } else {   // one cell per block: block row = station, NK = n_sectors
            const uint64_t c = a.first + (uint64_t)a.J0 * a.NK + i;
            const uint32_t cc = a.map.cnt[c];
            p.count = cc;
            p.cells = cc ? 1u : 0u;
            keep = cc >= a.min_count;
            if (keep) { p.sum = a.map.sum[c]; p.lo = a.map.lo[c]; p.hi = a.map.hi[c]; }
        }
        // (the lanes past the end of the input are not here: the ballots see the active lanes only)
        const bool empty = p.count == 0ull;
        const unsigned long long em = __ballot(empty), bm = __ballot(!empty && !keep);
        const int lane = lane_id();
        if (em && lane == (int)__builtin_ctzll(em)) atomicAdd(&wc_class_counts()[0], (uint32_t)__popcll(em));
        if (bm && lane == (int)__builtin_ctzll(bm)) atomicAdd(&wc_class_counts()[1], (uint32_t)__popcll(bm));
        return keep;
    }
};

// the straight position rule: p = (o - anchor) + tc a + rho (c u + s v)
struct WallCloudStraight {
    __device__ __forceinline__ void operator()(const WallCloudArgs &a, uint32_t, double tc, double rho, double c, double s,
                                               float (&xyz)[3]) const
    {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double w = __dadd_rn(__dmul_rn(c, a.u[i]), __dmul_rn(s, a.v[i]));
            const double q = __dadd_rn(__dadd_rn(a.oa[i], __dmul_rn(tc, a.a[i])), __dmul_rn(rho, w));
            xyz[i] = __double2float_rn(q);
        }
    }
};
// the arc position rule (a map of gm_wall_map_create_arc): p = (C - anchor) + (yc - 1 / kappa) n(tc) + zb b, with (cos, sin)
// of the block row's psi from the host's table: no fp64 trigonometry here either
struct WallCloudOnArc {
    WallCloudArc arc;
    __device__ __forceinline__ void operator()(const WallCloudArgs &a, uint32_t jl, double, double rho, double c, double s,
                                               float (&xyz)[3]) const
    {
        const double cp = arc.rows[2u * jl], sp = arc.rows[2u * jl + 1u];
        const double yc = __dmul_rn(rho, __dadd_rn(__dmul_rn(c, arc.un), __dmul_rn(s, arc.vn)));
        const double zb = __dmul_rn(rho, __dadd_rn(__dmul_rn(c, arc.ub), __dmul_rn(s, arc.vb)));
        const double r = __dsub_rn(yc, arc.inv_kappa);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double nr = __dsub_rn(__dmul_rn(arc.n[i], cp), __dmul_rn(a.a[i], sp));
            const double q = __dadd_rn(__dadd_rn(arc.ca[i], __dmul_rn(r, nr)), __dmul_rn(zb, arc.b[i]));
            xyz[i] = __double2float_rn(q);
        }
    }
};

// the clothoid position rule (a map of gm_wall_map_create_clothoid): p = ((P(tc) - anchor) + yc n(tc)) + zb b, with
// P(tc) - anchor and (cos, sin) of the block row's psi from the host's table: no fp64 trigonometry and no quadrature here
struct WallCloudOnClothoid {
    WallCloudClothoid cl;
    __device__ __forceinline__ void operator()(const WallCloudArgs &a, uint32_t jl, double, double rho, double c, double s,
                                               float (&xyz)[3]) const
    {
        const double *row = cl.rows + 5u * (size_t)jl;
        const double cp = row[3], sp = row[4];
        const double yc = __dmul_rn(rho, __dadd_rn(__dmul_rn(c, cl.un), __dmul_rn(s, cl.vn)));
        const double zb = __dmul_rn(rho, __dadd_rn(__dmul_rn(c, cl.ub), __dmul_rn(s, cl.vb)));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double nr = __dsub_rn(__dmul_rn(cl.n[i], cp), __dmul_rn(a.a[i], sp));
            const double q = __dadd_rn(__dadd_rn(row[i], __dmul_rn(yc, nr)), __dmul_rn(zb, cl.b[i]));
            xyz[i] = __double2float_rn(q);
        }
    }
};

// the record of survivor `src` of the chunk at rank `dst`, its position by `pos`
template <class Position>
__device__ __forceinline__ void wc_emit(const WallCloudArgs &a, const Position &pos, uint32_t src, uint32_t dst,
                                        const WallCloudPred::Payload &p)
{
    const uint32_t jl = src / a.NK, K = src % a.NK, J = a.J0 + jl;
    const uint32_t jw = J * a.bs;                                   // window-relative first station, < n
    const uint32_t ns = a.n - jw < a.bs ? a.n - jw : a.bs;
    const uint32_t j0 = a.station0 + jw;
    const double m = __ddiv_rn(__dmul_rn((double)(long long)p.sum, 0x1p-20), (double)p.count);
    const double h = __dmul_rn((double)(2u * j0 + ns), 0.5);
    const double tc = __dadd_rn(a.t_min, __dmul_rn(h, a.ds));
    const double rho = __dadd_rn(a.R, __dmul_rn(a.g, m));
    const double c = a.dirs[2u * K], s = a.dirs[2u * K + 1u];
    float xyz[3];
    pos(a, jl, tc, rho, c, s, xyz);
    gm_wall_cloud_point r;
    r.x = xyz[0]; r.y = xyz[1]; r.z = xyz[2];
    r.mean = __double2float_rn(m);
    r.min = ordered_to_float(~p.lo);
    r.max = ordered_to_float(p.hi);
    r.block = J * a.NK + K;
    r.cells = p.cells;
    r.count = p.count;
    a.out[dst] = r;
}
__device__ __forceinline__ void wc_prepare()
{
    if (threadIdx.x < 2) wc_class_counts()[threadIdx.x] = 0u;
}
__device__ __forceinline__ void wc_finish(const WallCloudArgs &a)
{
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t c = wc_class_counts()[threadIdx.x];
        if (c) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)c);
    }
}

struct WallCloudEmit {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallCloudArgs a;
    __device__ __forceinline__ void prepare() const { wc_prepare(); }
    __device__ __forceinline__ void finish(uint32_t) const { wc_finish(a); }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCloudPred::Payload &p) const
    {
        wc_emit(a, WallCloudStraight(), src, dst, p);
    }
};
// a map of gm_wall_map_create_arc: an emit step, hence a kernel, of its own
struct WallCloudEmitArc {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallCloudArgs a;
    WallCloudOnArc pos;
    __device__ __forceinline__ void prepare() const { wc_prepare(); }
    __device__ __forceinline__ void finish(uint32_t) const { wc_finish(a); }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCloudPred::Payload &p) const
    {
        wc_emit(a, pos, src, dst, p);
    }
};
// a map of gm_wall_map_create_clothoid: likewise
struct WallCloudEmitClothoid {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallCloudArgs a;
    WallCloudOnClothoid pos;
    __device__ __forceinline__ void prepare() const { wc_prepare(); }
    __device__ __forceinline__ void finish(uint32_t) const { wc_finish(a); }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCloudPred::Payload &p) const
    {
        wc_emit(a, pos, src, dst, p);
    }
};

// host side: the clothoid rule's struct of a launch's axis, and the compaction of a chunk's blocks under the emit step `emit`
inline WallCloudClothoid wall_cloud_clothoid(const WallCloudAxis &axis)
{
    WallCloudClothoid cl;
    cl.rows = axis.arc.rows;
    for (int k = 0; k < 3; ++k) { cl.n[k] = axis.arc.n[k]; cl.b[k] = axis.arc.b[k]; }
    cl.un = axis.arc.un; cl.ub = axis.arc.ub; cl.vn = axis.arc.vn; cl.vb = axis.arc.vb;
    return cl;
}
template <class Emit>
void wall_cloud_launch(const WallCloudArgs &a, const Emit &emit, const ScanState &st, hipStream_t s)
{
    const uint32_t nb = a.nJ * a.NK;   // >= 1
    WallCloudPred pred{a};
    hipLaunchKernelGGL((k_compact<WallCloudPred, Emit>), dim3(compact_grid(nb)), dim3(kCpThreads), 0, s, pred, emit,
                       (const uint32_t *)nullptr, nb, st, reinterpret_cast<uint32_t *>(a.ctr + 2), (uint32_t *)nullptr);
}

}  // namespace gm
