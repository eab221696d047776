// k_wall.hip -- BUILD-DEFINED EXTENSION: persistent wall map (gm_wall_*), the device side.
//
// The semantics are stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_np.py.  k_wall_add is
// k_surface_map's problem (one streaming pass over the valid cloud, scatter-reduce into station x sector cells, the
// per-point chain of gm_device.hpp) with two differences: the table is the map's (up to 2^24 cells, far beyond LDS) and
// outlives the launch, so no block converts or re-zeroes anything at the end.
//
// Shape: ONE launch per add, kWallThreads per block, one block per 8192 points of the frame's capacity (at most
// kWallMaxBlocks; small frames on up to 48 blocks: wall_blocks below).  The host derives the frame-local map frame
// (o', a', u', v') around the anchor station j_f in fp64 and passes it by value; the crop box bounds |t|, so the host
// also knows a window of whole stations around j_f that the frame's points fall into.
//   1. a block zeroes its private LDS table for the window: win_stations x n_sectors <= GM_SURF_MAX_CELLS cells of
//      sum i64, count u32, ~ordered(min e) u32, ordered(max e) u32 (80 KiB of static LDS, one block per CU);
//   2. the point stream of gm_point_stream.hpp (stream_points: 16 B of point + 1 B of label read) with the chain head of
//      gm_device.hpp (wall_chain); nothing written per point (the stage call's optional residual / cell outputs apart).
//      The in-wave run merge of the surface kernel, then LDS integer atomics for cells inside the window; a mapped point
//      outside it (fine grids, long crop boxes, oblique axes) goes straight to the map with the same device atomics --
//      slower, identical result;
//   3. the block flushes the window cells it touched to the map at (j_f + win_first) * n_sectors + cell with integer
//      device atomics (atomicAdd u32 / i64, atomicMax u32) and adds its class counts, one atomic per class
//      (block_class_counts).
// No floating-point atomics, no ticket, no host round trip: the point count is the device word n_valid.  Adds from
// several streams may interleave in the map: every update is an integer atomic, so the result does not depend on it.
#include <math.h>
#include <string.h>

#include "gm_wall_add.hpp"   // the launch shape and the map's integer update, shared with k_wall_joint.hip

namespace gm {

// kMasked (gm_wall_map_add_*_checked, k_wall_add_checked.hip marks the bits): bit i of m.words set = point i is SKIPPED,
// decided before every other class: it takes cell -1 and no count ahead of the run merge (every lane still takes part in
// it) and reaches neither the table nor T.totals.  A wave's 64 points are one aligned 64-bit word of the mask (w0 is a
// multiple of 64 in every trip: stride is a multiple of kWallThreads), so the mask costs one wave-uniform 8-byte load per
// trip.  The call's five class counts go to m.ctr[4 ..] beside T.totals.  The unmasked instantiation carries none of it,
// and each instantiation has an entry point of its own below, so that k_wall_add keeps its name and its arguments.
// (WallMask: gm_wall_add.hpp, shared with k_wall_add_joint)

// Axis (WallArcArg<false> straight, WallArcArg<true> a map of gm_wall_map_create_arc, WallClothoidArg one of
// gm_wall_map_create_clothoid): the chain head runs on the by-value axis block (wall_chain, gm_device.hpp); everything
// behind (e, jl, k) -- classes, window, run merge, flush -- is shared.  The straight instantiations carry none of it, and
// the arc and clothoid ones have entry points of their own below.
template <bool kMasked, class Axis>
__device__ __forceinline__ void wall_add(const WallArgs a, const WallMask<kMasked> m, const Axis c)
{
    constexpr int kCls = kMasked ? 5 : 4;
    __shared__ unsigned long long s_sum[kWallCells];
    __shared__ uint32_t s_cnt[kWallCells];
    __shared__ uint32_t s_lo[kWallCells];
    __shared__ uint32_t s_hi[kWallCells];
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    const uint32_t nsec = a.n_sectors;
    const uint32_t wcells = a.win_stations * nsec;   // <= kWallCells (the host sizes the window)
    const float win_lo = (float)a.win_first, win_hi = (float)(a.win_first + (int32_t)a.win_stations);
    const WallTable T = a.table;
    const int lane = lane_id();

    for (uint32_t c = threadIdx.x; c < wcells; c += kWallThreads) { s_sum[c] = 0ull; s_cnt[c] = 0u; s_lo[c] = 0u; s_hi[c] = 0u; }
    __syncthreads();

    uint32_t cls[kCls] = {};   // mapped, outside, beyond_gate, plane (, skipped)
    auto point = [&](uint64_t i, bool in, const float4 &q, uint32_t lab, unsigned long long mw) {
        const bool skip = kMasked && ((mw >> lane) & 1ull);
        const uint32_t live = skip ? 0u : 1u;
        float e = __builtin_nanf("");
        int cell = -1;      // global cell j * n_sectors + k (< 2^24)
        int lcell = -1;     // the same cell in the block's window, -1 outside it
        if (in) {
            if constexpr (kMasked) cls[kCls - 1] += 1u - live;
            int64_t j;
            float jl;
            uint32_t kk;
            if (wall_chain(q, lab, a, c, [&](float s) { return (j = wall_station(a, s)) >= 0; },
                           [&](uint32_t k) { cls[kChainMapped - k] += live; }, e, jl, kk)) {
                cell = (int)((uint32_t)j * nsec + kk);
                if (jl >= win_lo && jl < win_hi) lcell = (int)((uint32_t)((int32_t)jl - a.win_first) * nsec + kk);
            }
        }
        if (skip) { cell = -1; lcell = -1; }
        if (in && a.res) a.res[i] = e;
        if (in && a.cell) a.cell[i] = cell;
        uint32_t cn = 0u, lo = 0u, hi = 0u;
        unsigned long long sm = 0ull;
        if (cell >= 0) {
            cn = 1u;
            sm = (unsigned long long)(long long)__float2int_rn(__fmul_rn(e, kWallFix));
            hi = float_to_ordered(e);
            lo = ~hi;
        }
        if (surf_merge_runs(cell, cn, sm, lo, hi)) {   // (lanes of one run share the cell, hence lcell)
            if (lcell >= 0) {
                atomicAdd(&s_cnt[lcell], cn);
                atomicAdd(&s_sum[lcell], sm);
                atomicMax(&s_lo[lcell], lo);
                atomicMax(&s_hi[lcell], hi);
            } else {
                wall_global_add(T, (uint64_t)cell, cn, sm, lo, hi);
            }
        }
    };
    if constexpr (kMasked) {   // the slot's mask word rides with the slot's loads (wk: wave-uniform, < n <= 2^32)
        stream_points_with<kWallThreads, kWallUnroll>(
            a.pts, a.labels, n, [&](uint64_t wk) { return wk < n ? m.words[__builtin_amdgcn_readfirstlane((uint32_t)(wk >> 6))] : 0ull; },
            point);
    } else {
        stream_points<kWallThreads, kWallUnroll>(a.pts, a.labels, n,
                                                 [&](uint64_t i, bool in, const float4 &q, uint32_t lab) { point(i, in, q, lab, 0ull); });
    }
    __syncthreads();
    // flush the touched window cells, lane <-> cell (contiguous in the map: the window is whole stations).  A touched
    // cell is inside the map (only mapped points reach the table), so base + c is in range although base may not be.
    const int64_t base = (a.anchor + (int64_t)a.win_first) * (int64_t)nsec;
    for (uint32_t c = threadIdx.x; c < wcells; c += kWallThreads) {
        const uint32_t cn = s_cnt[c];
        if (!cn) continue;
        wall_global_add(T, (uint64_t)(base + (int64_t)c), cn, s_sum[c], s_lo[c], s_hi[c]);
    }
    // class counts: one atomic per class and block
    block_class_counts<kWallThreads>(cls, [&](uint32_t k, unsigned long long v) {
        if (v && k < 4u) atomicAdd(&T.totals[k], v);
        if constexpr (kMasked) {   // skipped | mapped, outside, beyond_gate, plane
            if (v) atomicAdd(&m.ctr[k == (uint32_t)kCls - 1u ? 4u : 5u + k], v);
        }
    });
}

__global__ __launch_bounds__(kWallThreads) void k_wall_add(WallArgs a)
{
    wall_add<false>(a, WallMask<false>(), WallArcArg<false>());
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_masked(WallArgs a, WallMask<true> m)
{
    wall_add<true>(a, m, WallArcArg<false>());
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_arc(WallArgs a, WallArcArg<true> c)
{
    wall_add<false>(a, WallMask<false>(), c);
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_arc_masked(WallArgs a, WallMask<true> m, WallArcArg<true> c)
{
    wall_add<true>(a, m, c);
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_clothoid(WallArgs a, WallClothoidArg c)
{
    wall_add<false>(a, WallMask<false>(), c);
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_clothoid_masked(WallArgs a, WallMask<true> m, WallClothoidArg c)
{
    wall_add<true>(a, m, c);
}

// ---- the small kernels: convert / copy out a window, merge a raw window, clear, count ----

constexpr int kWallSmallThreads = 256;

__global__ __launch_bounds__(kWallSmallThreads) void k_wall_read(WallTable T, uint64_t first, uint64_t n, gm_surface_cell *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kWallSmallThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWallSmallThreads) {
        const uint64_t c = first + i;
        const uint32_t cn = T.cnt[c];
        gm_surface_cell r;
        if (cn) {
            r.count = cn;
            r.mean = (float)(((double)(long long)T.sum[c] * 0x1p-20) / (double)cn);
            r.min = ordered_to_float(~T.lo[c]);
            r.max = ordered_to_float(T.hi[c]);
        } else {
            r.count = 0u;
            r.mean = r.min = r.max = __builtin_nanf("");
        }
        out[i] = r;
    }
}

__global__ __launch_bounds__(kWallSmallThreads) void k_wall_read_raw(WallTable T, uint64_t first, uint64_t n, gm_wall_raw_cell *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kWallSmallThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWallSmallThreads) {
        const uint64_t c = first + i;
        gm_wall_raw_cell r;
        r.sum = (int64_t)T.sum[c];
        r.count = T.cnt[c];
        r.min_key = T.lo[c];
        r.max_key = T.hi[c];
        r.reserved = 0u;
        out[i] = r;
    }
}

__global__ __launch_bounds__(kWallSmallThreads) void k_wall_merge_raw(WallTable T, uint64_t first, uint64_t n, const gm_wall_raw_cell *in)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kWallSmallThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWallSmallThreads) {
        const uint64_t c = first + i;
        const gm_wall_raw_cell r = in[i];
        if (!r.count) continue;
        // (the caller has synchronised: no add runs beside this launch, and each cell has one thread)
        T.sum[c] += (unsigned long long)r.sum;
        T.cnt[c] += r.count;
        T.lo[c] = T.lo[c] > r.min_key ? T.lo[c] : r.min_key;
        T.hi[c] = T.hi[c] > r.max_key ? T.hi[c] : r.max_key;
    }
}

__global__ __launch_bounds__(kWallSmallThreads) void k_wall_clear(WallTable T, uint64_t first, uint64_t n, uint32_t totals_too)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kWallSmallThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWallSmallThreads) {
        const uint64_t c = first + i;
        T.sum[c] = 0ull; T.cnt[c] = 0u; T.lo[c] = 0u; T.hi[c] = 0u;
    }
    if (totals_too && blockIdx.x == 0 && threadIdx.x < kWallTotals) T.totals[threadIdx.x] = 0ull;
}

// cells with count > 0 -> totals[4] (zeroed by the caller on the same stream)
__global__ __launch_bounds__(kWallSmallThreads) void k_wall_count(WallTable T, uint64_t n)
{
    uint32_t hit = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * kWallSmallThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWallSmallThreads)
        hit += T.cnt[i] ? 1u : 0u;
    hit = wave_sum(hit);
    if (lane_id() == 0 && hit) atomicAdd(&T.totals[4], (unsigned long long)hit);
}

static uint32_t small_blocks(uint64_t n)
{
    const uint64_t b = (n + kWallSmallThreads - 1) / kWallSmallThreads;
    return (uint32_t)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

size_t wall_table_bytes(uint64_t ncell) { return (size_t)(((20 * ncell + 7) & ~(uint64_t)7) + 8 * kWallTotals); }

// One block per kWallPointsPerBlock points, but a small frame is spread over up to kWallSmallBlocks blocks of at least
// kWallMinPointsPerBlock points: a block's fixed cost (zeroing the window, the flush) is paid per block, its share of the
// stream shrinks with the grid; 50-120 blocks measured best on the 0.1 M and 1 M frames.
uint32_t wall_blocks(uint32_t n_cap, uint32_t points_per_block)
{
    const uint64_t n = n_cap;
    uint64_t b;
    if (points_per_block) {
        b = (n + points_per_block - 1) / points_per_block;
    } else {
        b = (n + kWallPointsPerBlock - 1) / kWallPointsPerBlock;
        const uint64_t small = (n + kWallMinPointsPerBlock - 1) / kWallMinPointsPerBlock;
        const uint64_t spread = small < kWallSmallBlocks ? small : kWallSmallBlocks;
        b = b > spread ? b : spread;
    }
    return (uint32_t)(b < 1 ? 1 : (b > kWallMaxBlocks ? kWallMaxBlocks : b));
}

// the add's one front: the instantiation of the axis' kind, masked where a mask is given
void launch_wall_add(const WallArgs &a, const WallAxis &axis, const unsigned long long *mask, unsigned long long *ctr, uint32_t n_cap,
                     uint32_t points_per_block, hipStream_t s)
{
    const dim3 grid(wall_blocks(n_cap, points_per_block)), block(kWallThreads);
    const WallArcArg<true> arc{axis.ax.arc};
    const WallClothoidArg cl{axis.ax};
    WallMask<true> m;
    m.words = mask;
    m.ctr = ctr;
    if (axis.kind == kAxisClothoid) {
        if (mask) hipLaunchKernelGGL(k_wall_add_clothoid_masked, grid, block, 0, s, a, m, cl);
        else hipLaunchKernelGGL(k_wall_add_clothoid, grid, block, 0, s, a, cl);
    } else if (axis.kind == kAxisArc) {
        if (mask) hipLaunchKernelGGL(k_wall_add_arc_masked, grid, block, 0, s, a, m, arc);
        else hipLaunchKernelGGL(k_wall_add_arc, grid, block, 0, s, a, arc);
    } else {
        if (mask) hipLaunchKernelGGL(k_wall_add_masked, grid, block, 0, s, a, m);
        else hipLaunchKernelGGL(k_wall_add, grid, block, 0, s, a);
    }
}

void launch_wall_read(const WallTable &T, uint64_t first, uint64_t n, gm_surface_cell *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_read, dim3(small_blocks(n)), dim3(kWallSmallThreads), 0, s, T, first, n, out);
}
void launch_wall_read_raw(const WallTable &T, uint64_t first, uint64_t n, gm_wall_raw_cell *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_read_raw, dim3(small_blocks(n)), dim3(kWallSmallThreads), 0, s, T, first, n, out);
}
void launch_wall_merge_raw(const WallTable &T, uint64_t first, uint64_t n, const gm_wall_raw_cell *in, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_merge_raw, dim3(small_blocks(n)), dim3(kWallSmallThreads), 0, s, T, first, n, in);
}
void launch_wall_clear(const WallTable &T, uint64_t first, uint64_t n, bool totals_too, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_clear, dim3(small_blocks(n)), dim3(kWallSmallThreads), 0, s, T, first, n, totals_too ? 1u : 0u);
}
void launch_wall_count(const WallTable &T, uint64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_count, dim3(small_blocks(n)), dim3(kWallSmallThreads), 0, s, T, n);
}

}  // namespace gm
