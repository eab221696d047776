// k_wall_regions.hip -- BUILD-DEFINED EXTENSION: connected deviation regions of the persistent wall map
// (gm_wall_map_regions), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/regions_np.py.  Connected components of the
// flagged cells of a station window, positive and negative cells apart, on the labelling core of gm_gridcc.hpp (which
// states the union-find and the memory ordering of the seams launch):
//   1. k_wall_region_tiles    one block per tile of ts x tk <= 4096 window cells.  Reads sum and count (and the
//      baseline's), 12 or 24 B per cell, computes d and the sign, labels the tile (cc_label_tile on the signs) and writes
//      d of the flagged cells.  Class counts: one atomic per class and block.
//   2. k_wall_region_seams    one thread per border cell (cc_seam); cells join when both are flagged with one sign.
//   3. k_wall_region_flatten  cc_flatten.  The component count goes to the host, which sizes the accumulators.
//   4. k_wall_region_reduce   every flagged cell adds into the record of its root's slot with integer atomics only (add:
//      cells, sum_d, points; max: the four extents, minima kept inverted; one 64-bit max of |d| << 32 | ~cell: the peak).
//      Runs of one slot in consecutive lanes are merged in the wave first (wave_runs, gm_device.hpp).
//   5. k_wall_region_select   one thread per slot: components of >= min_cells cells become gm_wall_region records, in
//      slot order (the host sorts the copied list by label).
//   6. k_wall_region_labels   only when the caller asks for cell_labels, per chunk of the staging buffer.
// No floating point anywhere.
#include <string.h>

#include "gm_internal.hpp"
#include "gm_gridcc.hpp"

namespace gm {

static_assert(sizeof(WallRegionAcc) == 64 && sizeof(gm_wall_region) == 64, "64-byte records");

// ---- 1. tiles ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_tiles(WallRegionArgs a)
{
    __shared__ uint32_t L[kWallRegionTileCells];
    __shared__ int8_t S[kWallRegionTileCells];
    __shared__ uint32_t s_cls[4];
    const uint32_t ts = a.ts, tk = a.tk, nsec = a.nsec, cells = ts * tk;   // <= kWallRegionTileCells (the host checks)
    const uint32_t j0 = (blockIdx.x / a.tiles_k) * ts, k0 = (blockIdx.x % a.tiles_k) * tk;
    if (threadIdx.x < 4) s_cls[threadIdx.x] = 0u;
    uint32_t cls[4] = {0u, 0u, 0u, 0u};   // flagged_pos, flagged_neg, unusable, empty
    for (uint32_t l = threadIdx.x; l < cells; l += kCcThreads) {
        const uint32_t j = j0 + l / tk, k = k0 + l % tk;
        int sign = 0;
        if (j < a.n && k < nsec) {
            const uint32_t w = j * nsec + k;
            const uint64_t c = a.first + w;
            const uint32_t cn = a.map.cnt[c];
            uint32_t bn = 0u;
            bool usable = cn >= a.min_count;
            if (a.has_base) {
                bn = a.base.cnt[c];
                usable = usable && bn >= a.min_count;
            }
            long long d = 0;
            if (usable) {   // (min_count >= 1: no division by zero)
                d = (long long)a.map.sum[c] / (long long)cn;
                if (a.has_base)   // (two's complement wrap, never reached by gated residuals)
                    d = (long long)((unsigned long long)d - (unsigned long long)((long long)a.base.sum[c] / (long long)bn));
                sign = d >= a.T ? 1 : (d <= -a.T ? -1 : 0);
            }
            if (sign > 0) ++cls[0];
            else if (sign < 0) ++cls[1];
            else if (!usable && (cn | bn)) ++cls[2];
            else if (!usable) ++cls[3];
            if (sign) a.d[w] = d;
            else a.parent[w] = kCcNone;
        }
        S[l] = (int8_t)sign;
        L[l] = l;
    }
    cc_label_tile(L, S, cells, tk, a.conn8 != 0u, a.parent, [=](uint32_t r, uint32_t c) { return (j0 + r) * nsec + k0 + c; });
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = wave_sum(cls[k]);
        if (lane_id() == 0 && v) atomicAdd(&s_cls[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cls[threadIdx.x]) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)s_cls[threadIdx.x]);
}

// ---- 2. seams ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_seams(WallRegionArgs a)
{
    const uint64_t count = cc_seam_count(a.n, a.nsec, a.tiles_s, a.tiles_k);
    for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kCcThreads)
        cc_seam(i, a.n, a.nsec, a.ts, a.tk, a.tiles_k, a.conn8 != 0u, 0u, [&a](uint32_t x, uint32_t y) {
            // window cells x and y join when both are flagged with one sign (d is of the launch before)
            if (cc_joinable(a.parent, x, y) && (a.d[x] > 0) == (a.d[y] > 0)) cc_union(a.parent, x, y);
        });
}

// ---- 3. flatten ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_flatten(WallRegionArgs a)
{
    cc_flatten(a.parent, a.slot, (uint64_t)a.n * a.nsec, &a.ctr[4]);
}

// ---- 4. reduce ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_reduce(WallRegionArgs a)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    const uint32_t nsec = a.nsec, half = nsec / 2u;
    const int lane = lane_id();
    for (uint64_t w0 = (uint64_t)blockIdx.x * kCcThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < total;
         w0 += (uint64_t)gridDim.x * kCcThreads) {
        const uint64_t w = w0 + lane;
        int slot = -1;
        uint32_t cells = 0u, smin = 0u, smax = 0u, kmin = 0u, kmax = 0u, tmin = 0u, tmax = 0u;
        unsigned long long sum = 0ull, pts = 0ull, peak = 0ull;
        if (w < total) {
            const uint32_t r = a.parent[w];
            if (r != kCcNone) {
                slot = (int)a.slot[r];
                const uint64_t c = a.first + w;
                const uint32_t j = (uint32_t)(c / nsec), k = (uint32_t)(c % nsec), t = k + half < nsec ? k + half : k + half - nsec;
                const long long d = a.d[w];
                const unsigned long long mag = d < 0 ? 0ull - (unsigned long long)d : (unsigned long long)d;
                cells = 1u;
                smin = ~j; smax = j; kmin = ~k; kmax = k; tmin = ~t; tmax = t;
                sum = (unsigned long long)d;
                pts = a.map.cnt[c];
                peak = ((mag > 0xFFFFFFFFull ? 0xFFFFFFFFull : mag) << 32) | (uint32_t)~(uint32_t)c;
                if (r == (uint32_t)w) a.acc[slot].label = (uint32_t)c;   // the root alone
            }
        }
        const WaveRuns run = wave_runs(slot);
        if (run.any) {
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t oc = __shfl_down(cells, o, kWave), o1 = __shfl_down(smin, o, kWave), o2 = __shfl_down(smax, o, kWave),
                               o3 = __shfl_down(kmin, o, kWave), o4 = __shfl_down(kmax, o, kWave), o5 = __shfl_down(tmin, o, kWave),
                               o6 = __shfl_down(tmax, o, kWave);
                const unsigned long long os = __shfl_down(sum, o, kWave), op = __shfl_down(pts, o, kWave),
                                         ok = __shfl_down(peak, o, kWave);
                if (run.lane + o <= run.tail) {
                    cells += oc; sum += os; pts += op;
                    smin = smin > o1 ? smin : o1; smax = smax > o2 ? smax : o2;
                    kmin = kmin > o3 ? kmin : o3; kmax = kmax > o4 ? kmax : o4;
                    tmin = tmin > o5 ? tmin : o5; tmax = tmax > o6 ? tmax : o6;
                    peak = peak > ok ? peak : ok;
                }
            }
        }
        if (slot >= 0 && !run.dup) {
            WallRegionAcc *r = &a.acc[slot];
            atomicAdd(&r->cells, cells);
            atomicAdd(&r->sum_d, sum);
            atomicAdd(&r->points, pts);
            atomicMax(&r->st_min_inv, smin); atomicMax(&r->st_max, smax);
            atomicMax(&r->k_min_inv, kmin); atomicMax(&r->k_max, kmax);
            atomicMax(&r->t_min_inv, tmin); atomicMax(&r->t_max, tmax);
            atomicMax(&r->peak_key, peak);
        }
    }
}

// ---- 5. select ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_select(WallRegionArgs a)
{
    for (uint32_t s = blockIdx.x * kCcThreads + threadIdx.x; s < a.ncomp; s += gridDim.x * kCcThreads) {
        const WallRegionAcc r = a.acc[s];
        if (r.cells < a.min_cells) continue;
        const uint32_t at = (uint32_t)atomicAdd(&a.ctr[5], 1ull);   // (< ncomp: one per slot at the most)
        const uint32_t pc = ~(uint32_t)r.peak_key;
        const long long pd = a.d[pc - a.first];
        gm_wall_region g;
        g.label = r.label;
        g.sign = pd > 0 ? 1 : -1;
        g.cells = r.cells;
        g.station_min = ~r.st_min_inv; g.station_max = r.st_max;
        g.sector_min = ~r.k_min_inv; g.sector_max = r.k_max;
        g.sector_min_turned = ~r.t_min_inv; g.sector_max_turned = r.t_max;
        g.peak_cell = pc;
        g.peak = pd;
        g.sum_d = (long long)r.sum_d;
        g.points = r.points;
        a.out[at] = g;
    }
}

// ---- 6. labels ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_labels(WallRegionArgs a, uint64_t first, uint64_t n, int32_t *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kCcThreads) {
        const uint32_t r = a.parent[first + i];
        int32_t lab = -1;
        if (r != kCcNone && a.acc[a.slot[r]].cells >= a.min_cells) lab = (int32_t)(a.first + r);
        out[i] = lab;
    }
}

void launch_wall_region_label(const WallRegionArgs &a, hipStream_t s)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    hipLaunchKernelGGL(k_wall_region_tiles, dim3(a.tiles_s * a.tiles_k), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_seams, dim3(cc_blocks(cc_seam_count(a.n, a.nsec, a.tiles_s, a.tiles_k))), dim3(kCcThreads),
                       0, s, a);
    hipLaunchKernelGGL(k_wall_region_flatten, dim3(cc_blocks(total)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_region_reduce(const WallRegionArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_reduce, dim3(cc_blocks((uint64_t)a.n * a.nsec)), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_select, dim3(cc_blocks(a.ncomp)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_region_labels(const WallRegionArgs &a, uint64_t first, uint64_t n, int32_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_labels, dim3(cc_blocks(n)), dim3(kCcThreads), 0, s, a, first, n, out);
}

}  // namespace gm
