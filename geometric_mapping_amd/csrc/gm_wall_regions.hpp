// gm_wall_regions.hpp -- the one statement of the two region kernels that read a cell of a map (tiles: sum and count, and
// the baseline's; reduce: the count of a flagged cell) for k_wall_regions.hip (a map's window: the cells are the map's own)
// and k_wall_regions_joint.hip (an alignment's window: the cells of its pieces, one element map each).  include/gm_hip.h
// states both rules; everything behind the read -- d, the sign, the classes, the tile's labels, the accumulators -- is the
// same code for both, and seams, flatten, select and labels never see a cell of a map.  The reader is a compile-time
// parameter: the map's instantiation holds no trace of the piece table.
//
// A reader says where window cell (row j, sector k) lies:
//   open(a, j0)        once per block, ahead of the cells: j0 is the first window row the block reads
//   at(a, j, k, w, c)  the tables and the index of the cell in them (w = j nsec + k); false: no such cell.  One thread's
//                      rows never decrease between two calls.
// and the reduce asks it for the count of one flagged cell alone (count).
#pragma once

#include "gm_internal.hpp"
#include "gm_gridcc.hpp"

namespace gm {

struct WrCell {
    const unsigned long long *sum, *base_sum;
    const uint32_t *cnt, *base_cnt;
    uint64_t c;
};

// a map's window: cell w of the window is cell first + w of the map
struct WrMapCells {
    __device__ __forceinline__ void open(const WallRegionArgs &, uint32_t) {}
    __device__ __forceinline__ bool at(const WallRegionArgs &a, uint32_t, uint32_t, uint32_t w, WrCell &c) const
    {
        c.sum = a.map.sum; c.cnt = a.map.cnt;
        c.base_sum = a.base.sum; c.base_cnt = a.base.cnt;
        c.c = a.first + w;
        return true;
    }
    static __device__ __forceinline__ uint32_t count(const WallRegionArgs &a, uint64_t w, uint32_t) { return a.map.cnt[a.first + w]; }
};

// the last piece that starts at or before window row j: every index is < n_pieces (>= 1), whatever the table holds
__device__ __forceinline__ uint32_t wr_piece_of(const WallRegionPiece *pieces, uint32_t n_pieces, uint32_t j)
{
    uint32_t lo = 0u, hi = n_pieces;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pieces[mid].row0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// An alignment's window: the piece of the block's first row by binary search, once per block; from there each thread
// walks forward as its rows advance.  The piece is checked (p < n_pieces, row - row0 < rows) before anything is read
// through it, and the host has checked station0 + rows <= the element map's stations: every index is inside its table.
struct WrPieceCells {
    uint32_t p, row0, rows, station0;
    const unsigned long long *sum, *base_sum;
    const uint32_t *cnt, *base_cnt;
    __device__ __forceinline__ void load(const WallRegionArgs &a)
    {
        rows = 0u;
        if (p < a.n_pieces) {
            const WallRegionPiece &q = a.pieces[p];
            row0 = q.row0; rows = q.rows; station0 = q.station0;
            sum = q.map.sum; cnt = q.map.cnt;
            base_sum = q.base.sum; base_cnt = q.base.cnt;
        }
    }
    __device__ __forceinline__ void open(const WallRegionArgs &a, uint32_t j0)
    {
        __shared__ uint32_t s_piece;
        if (threadIdx.x == 0) s_piece = wr_piece_of(a.pieces, a.n_pieces, j0);
        __syncthreads();
        p = s_piece;
        row0 = 0u; station0 = 0u;
        sum = base_sum = nullptr; cnt = base_cnt = nullptr;
        load(a);
    }
    __device__ __forceinline__ bool at(const WallRegionArgs &a, uint32_t j, uint32_t k, uint32_t, WrCell &c)
    {
        while (p < a.n_pieces && (j < row0 || j - row0 >= rows)) {   // (j >= row0 of the piece found: the rows ascend)
            ++p;
            load(a);
        }
        if (p >= a.n_pieces) return false;   // (a gapless table over the window's rows: not reached)
        c.sum = sum; c.cnt = cnt; c.base_sum = base_sum; c.base_cnt = base_cnt;
        c.c = (uint64_t)(station0 + (j - row0)) * a.nsec + k;
        return true;
    }
    // the count of one flagged cell: its piece by binary search, for the flagged cells alone
    static __device__ __forceinline__ uint32_t count(const WallRegionArgs &a, uint64_t w, uint32_t k)
    {
        const uint32_t j = (uint32_t)w / a.nsec;   // (w < 2^26: the size rule)
        const WallRegionPiece &q = a.pieces[wr_piece_of(a.pieces, a.n_pieces, j)];
        if (j < q.row0 || j - q.row0 >= q.rows) return 0u;   // (not reached either)
        return q.map.cnt[(uint64_t)(q.station0 + (j - q.row0)) * a.nsec + k];
    }
};

// ---- 1. tiles ----

template <class Cells>
__device__ __forceinline__ void wr_tiles(const WallRegionArgs a)
{
    __shared__ uint32_t L[kWallRegionTileCells];
    __shared__ int8_t S[kWallRegionTileCells];
    __shared__ uint32_t s_cls[4];
    const uint32_t ts = a.ts, tk = a.tk, nsec = a.nsec, cells = ts * tk;   // <= kWallRegionTileCells (the host checks)
    const uint32_t j0 = (blockIdx.x / a.tiles_k) * ts, k0 = (blockIdx.x % a.tiles_k) * tk;
    if (threadIdx.x < 4) s_cls[threadIdx.x] = 0u;
    Cells rd;
    rd.open(a, j0);
    uint32_t cls[4] = {0u, 0u, 0u, 0u};   // flagged_pos, flagged_neg, unusable, empty
    for (uint32_t l = threadIdx.x; l < cells; l += kCcThreads) {
        const uint32_t j = j0 + l / tk, k = k0 + l % tk;
        int sign = 0;
        WrCell at;
        if (j < a.n && k < nsec && rd.at(a, j, k, j * nsec + k, at)) {
            const uint32_t w = j * nsec + k;
            const uint64_t c = at.c;
            const uint32_t cn = at.cnt[c];
            uint32_t bn = 0u;
            bool usable = cn >= a.min_count;
            if (a.has_base) {
                bn = at.base_cnt[c];
                usable = usable && bn >= a.min_count;
            }
            long long d = 0;
            if (usable) {   // (min_count >= 1: no division by zero)
                d = (long long)at.sum[c] / (long long)cn;
                if (a.has_base)   // (two's complement wrap, never reached by gated residuals)
                    d = (long long)((unsigned long long)d - (unsigned long long)((long long)at.base_sum[c] / (long long)bn));
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

// ---- 4. reduce ----

template <class Cells>
__device__ __forceinline__ void wr_reduce(const WallRegionArgs a)
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
                pts = Cells::count(a, w, k);
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

}  // namespace gm
