// k_wall_regions.hip -- BUILD-DEFINED EXTENSION: connected deviation regions of the persistent wall map
// (gm_wall_map_regions), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/regions_np.py.  Connected components of the
// flagged cells of a station window on a grid whose sector index wraps, by a union-find in a FIXED number of launches
// (no "propagate until nothing changes": a snake-shaped component would need thousands of rounds):
//   1. k_wall_region_tiles    one block per tile of ts x tk <= 4096 window cells.  Reads sum and count (and the
//      baseline's), 12 or 24 B per cell, computes d and the sign, and labels the tile with a union-find in LDS (left, up
//      and, for 8-connectivity, the two upper diagonals; no wrap inside a tile).  Writes one u32 parent per window cell
//      -- the window-local index of the cell's tile root, the smallest index of its tile component; kWallRegionNone for
//      a cell that is not flagged -- and d of the flagged cells.  Class counts: one atomic per class and block.
//   2. k_wall_region_seams    one thread per border cell: the last sector column of every tile column against the next
//      column (the last one against sector 0: the seam), the last station row of every tile row against the next row,
//      with the diagonal pairs for 8-connectivity.  Lock-free merge: find both roots, atomicMin the larger root's parent
//      to the smaller, retry on a lost race.  Blocks of this launch read parents other blocks are changing, so EVERY
//      access to the parent array in this kernel is an agent-scope atomic (a plain load may be served stale from L1 or
//      another XCD's L2).  A parent only ever decreases and stays inside the component, so the root of a finished
//      forest is the component's smallest index: the label.
//   3. k_wall_region_flatten  every flagged cell finds its root and stores it; roots take a region slot from a counter
//      (one atomic per wave).  The component count goes to the host, which sizes the accumulators.
//   4. k_wall_region_reduce   every flagged cell adds into the record of its root's slot with integer atomics only (add:
//      cells, sum_d, points; max: the four extents, minima kept inverted; one 64-bit max of |d| << 32 | ~cell: the peak).
//      Runs of one slot in consecutive lanes are merged in the wave first.
//   5. k_wall_region_select   one thread per slot: components of >= min_cells cells become gm_wall_region records, in
//      slot order (the host sorts the copied list by label).
//   6. k_wall_region_labels   only when the caller asks for cell_labels, per chunk of the staging buffer.
// Launch boundaries order everything but the parents inside launch 2.  No floating point anywhere.
#include <string.h>

#include "gm_internal.hpp"
#include "gm_unionfind.hpp"   // wr_load, wr_lds_find / wr_lds_union (tiles), wr_find / wr_union (seams)

namespace gm {

static_assert(sizeof(WallRegionAcc) == 64 && sizeof(gm_wall_region) == 64, "64-byte records");
constexpr int kWrThreads = 256;
constexpr uint32_t kWrMaxBlocks = 8192;

// ---- 1. tiles ----

__global__ __launch_bounds__(kWrThreads) void k_wall_region_tiles(WallRegionArgs a)
{
    __shared__ uint32_t L[kWallRegionTileCells];
    __shared__ int8_t S[kWallRegionTileCells];
    __shared__ uint32_t s_cls[4];
    const uint32_t ts = a.ts, tk = a.tk, nsec = a.nsec, cells = ts * tk;   // <= kWallRegionTileCells (the host checks)
    const uint32_t j0 = (blockIdx.x / a.tiles_k) * ts, k0 = (blockIdx.x % a.tiles_k) * tk;
    if (threadIdx.x < 4) s_cls[threadIdx.x] = 0u;
    uint32_t cls[4] = {0u, 0u, 0u, 0u};   // flagged_pos, flagged_neg, unusable, empty
    for (uint32_t l = threadIdx.x; l < cells; l += kWrThreads) {
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
            else a.parent[w] = kWallRegionNone;
        }
        S[l] = (int8_t)sign;
        L[l] = l;
    }
    __syncthreads();
    for (uint32_t l = threadIdx.x; l < cells; l += kWrThreads) {
        const int s = S[l];
        if (!s) continue;
        const uint32_t jl = l / tk, kl = l % tk;
        if (kl > 0 && S[l - 1] == s) wr_lds_union(L, l, l - 1);
        if (jl > 0) {
            if (S[l - tk] == s) wr_lds_union(L, l, l - tk);
            if (a.conn8) {
                if (kl > 0 && S[l - tk - 1] == s) wr_lds_union(L, l, l - tk - 1);
                if (kl + 1 < tk && S[l - tk + 1] == s) wr_lds_union(L, l, l - tk + 1);
            }
        }
    }
    __syncthreads();
    // (tile-local and window-local indices are both row-major in (j, k): the smallest of one is the smallest of the other)
    for (uint32_t l = threadIdx.x; l < cells; l += kWrThreads) {
        if (!S[l]) continue;
        const uint32_t r = wr_lds_find(L, l);
        a.parent[(j0 + l / tk) * nsec + k0 + l % tk] = (j0 + r / tk) * nsec + k0 + r % tk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = wave_sum(cls[k]);
        if (lane_id() == 0 && v) atomicAdd(&s_cls[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cls[threadIdx.x]) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)s_cls[threadIdx.x]);
}

// ---- 2. seams ----

// joins window cells x and y when both are flagged with one sign
__device__ __forceinline__ void wr_join(const WallRegionArgs &a, uint32_t x, uint32_t y)
{
    if (x == y || wr_load(&a.parent[x]) == kWallRegionNone || wr_load(&a.parent[y]) == kWallRegionNone) return;
    if ((a.d[x] > 0) != (a.d[y] > 0)) return;   // (d is of the launch before)
    wr_union(a.parent, x, y);
}

__global__ __launch_bounds__(kWrThreads) void k_wall_region_seams(WallRegionArgs a)
{
    const uint32_t nsec = a.nsec;
    const uint64_t n_vert = (uint64_t)a.tiles_k * a.n, n_hor = (uint64_t)(a.tiles_s - 1u) * nsec;
    for (uint64_t i = (uint64_t)blockIdx.x * kWrThreads + threadIdx.x; i < n_vert + n_hor; i += (uint64_t)gridDim.x * kWrThreads) {
        if (i < n_vert) {   // the last column of tile column b against the next column, the seam for the last
            const uint32_t b = (uint32_t)(i % a.tiles_k), j = (uint32_t)(i / a.tiles_k);
            const uint32_t end = (b + 1u) * a.tk, k = (end < nsec ? end : nsec) - 1u, k2 = k + 1u < nsec ? k + 1u : 0u;
            const uint32_t x = j * nsec + k;
            wr_join(a, x, j * nsec + k2);
            if (a.conn8) {
                if (j > 0u) wr_join(a, x, (j - 1u) * nsec + k2);
                if (j + 1u < a.n) wr_join(a, x, (j + 1u) * nsec + k2);
            }
        } else {            // the last row of tile row b against the next row
            const uint64_t h = i - n_vert;
            const uint32_t b = (uint32_t)(h / nsec), k = (uint32_t)(h % nsec), j = (b + 1u) * a.ts - 1u;   // j + 1 < n
            const uint32_t x = j * nsec + k, y = (j + 1u) * nsec;
            wr_join(a, x, y + k);
            if (a.conn8) {
                wr_join(a, x, y + (k + 1u < nsec ? k + 1u : 0u));
                wr_join(a, x, y + (k > 0u ? k - 1u : nsec - 1u));
            }
        }
    }
}

// ---- 3. flatten ----

__global__ __launch_bounds__(kWrThreads) void k_wall_region_flatten(WallRegionArgs a)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    const int lane = lane_id();
    // wave-uniform trips (the slot ranks come from a ballot)
    for (uint64_t w0 = (uint64_t)blockIdx.x * kWrThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < total;
         w0 += (uint64_t)gridDim.x * kWrThreads) {
        const uint64_t w = w0 + lane;
        bool root = false;
        if (w < total) {
            uint32_t x = wr_load(&a.parent[w]);
            if (x != kWallRegionNone) {
                // (other threads store roots meanwhile: every value ever stored is an ancestor, so the walk still ends at
                // the root)
                for (;;) {
                    const uint32_t y = wr_load(&a.parent[x]);
                    if (y == x) break;
                    x = y;
                }
                root = x == (uint32_t)w;
                if (!root) __hip_atomic_store(&a.parent[w], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const unsigned long long m = __ballot(root);
        if (m) {
            unsigned long long base = 0ull;
            if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(&a.ctr[4], (unsigned long long)__popcll(m));
            base = __shfl(base, (int)__builtin_ctzll(m), kWave);
            if (root) a.slot[w] = (uint32_t)base + (uint32_t)__popcll(m & lanemask_lt());
        }
    }
}

// ---- 4. reduce ----

__global__ __launch_bounds__(kWrThreads) void k_wall_region_reduce(WallRegionArgs a)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    const uint32_t nsec = a.nsec, half = nsec / 2u;
    const int lane = lane_id();
    for (uint64_t w0 = (uint64_t)blockIdx.x * kWrThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < total;
         w0 += (uint64_t)gridDim.x * kWrThreads) {
        const uint64_t w = w0 + lane;
        int slot = -1;
        uint32_t cells = 0u, smin = 0u, smax = 0u, kmin = 0u, kmax = 0u, tmin = 0u, tmax = 0u;
        unsigned long long sum = 0ull, pts = 0ull, peak = 0ull;
        if (w < total) {
            const uint32_t r = a.parent[w];
            if (r != kWallRegionNone) {
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
        // runs of one slot in consecutive lanes -> the run's head lane (surf_merge_runs' segmented reduction)
        const int prev = __shfl_up(slot, 1, kWave);
        const bool dup = lane > 0 && slot >= 0 && prev == slot;
        const unsigned long long dmask = __ballot(dup);
        if (dmask) {
            const unsigned long long above = lane < kWave - 1 ? (~dmask & (~0ull << (lane + 1))) : 0ull;
            const int tail = above ? __ffsll((long long)above) - 2 : kWave - 1;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t oc = __shfl_down(cells, o, kWave), o1 = __shfl_down(smin, o, kWave), o2 = __shfl_down(smax, o, kWave),
                               o3 = __shfl_down(kmin, o, kWave), o4 = __shfl_down(kmax, o, kWave), o5 = __shfl_down(tmin, o, kWave),
                               o6 = __shfl_down(tmax, o, kWave);
                const unsigned long long os = __shfl_down(sum, o, kWave), op = __shfl_down(pts, o, kWave),
                                         ok = __shfl_down(peak, o, kWave);
                if (lane + o <= tail) {
                    cells += oc; sum += os; pts += op;
                    smin = smin > o1 ? smin : o1; smax = smax > o2 ? smax : o2;
                    kmin = kmin > o3 ? kmin : o3; kmax = kmax > o4 ? kmax : o4;
                    tmin = tmin > o5 ? tmin : o5; tmax = tmax > o6 ? tmax : o6;
                    peak = peak > ok ? peak : ok;
                }
            }
        }
        if (slot >= 0 && !dup) {
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

__global__ __launch_bounds__(kWrThreads) void k_wall_region_select(WallRegionArgs a)
{
    for (uint32_t s = blockIdx.x * kWrThreads + threadIdx.x; s < a.ncomp; s += gridDim.x * kWrThreads) {
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

__global__ __launch_bounds__(kWrThreads) void k_wall_region_labels(WallRegionArgs a, uint64_t first, uint64_t n, int32_t *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kWrThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWrThreads) {
        const uint32_t r = a.parent[first + i];
        int32_t lab = -1;
        if (r != kWallRegionNone && a.acc[a.slot[r]].cells >= a.min_cells) lab = (int32_t)(a.first + r);
        out[i] = lab;
    }
}

static uint32_t wr_blocks(uint64_t n)
{
    const uint64_t b = (n + kWrThreads - 1) / kWrThreads;
    return (uint32_t)(b < 1 ? 1 : (b > kWrMaxBlocks ? kWrMaxBlocks : b));
}

void launch_wall_region_label(const WallRegionArgs &a, hipStream_t s)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    hipLaunchKernelGGL(k_wall_region_tiles, dim3(a.tiles_s * a.tiles_k), dim3(kWrThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_seams, dim3(wr_blocks((uint64_t)a.tiles_k * a.n + (uint64_t)(a.tiles_s - 1u) * a.nsec)),
                       dim3(kWrThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_flatten, dim3(wr_blocks(total)), dim3(kWrThreads), 0, s, a);
}
void launch_wall_region_reduce(const WallRegionArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_reduce, dim3(wr_blocks((uint64_t)a.n * a.nsec)), dim3(kWrThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_select, dim3(wr_blocks(a.ncomp)), dim3(kWrThreads), 0, s, a);
}
void launch_wall_region_labels(const WallRegionArgs &a, uint64_t first, uint64_t n, int32_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_labels, dim3(wr_blocks(n)), dim3(kWrThreads), 0, s, a, first, n, out);
}

}  // namespace gm
