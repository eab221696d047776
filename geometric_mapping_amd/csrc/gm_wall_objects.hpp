// gm_wall_objects.hpp -- the one statement of a row's decode and of the three kernels that read a row (bin, reduce, rows)
// for k_wall_objects.hip (a map's rows: cell is the map's cell) and k_wall_objects_joint.hip (an alignment's rows: cell is
// side << 24 | cell, decoded through the by-value side table onto the global station grid).  include/gm_hip.h states both
// rules; everything behind the decode -- blocks, window, planes, accumulators -- is the same code for both, and tiles,
// seams, flatten, blocks and select never see a cell.  kJoint is a compile-time switch: the map's instantiation holds no
// trace of the side table.
#pragma once

#include "gm_internal.hpp"
#include "gm_gridcc.hpp"

namespace gm {

// side's entry of a by-value table of GM_WALL_JOINT_MAX_SIDES words; side < 4 has been checked: selects, no indexed load
__device__ __forceinline__ uint32_t wo_side_word(const uint32_t (&t)[4], uint32_t side)
{
    return side == 0u ? t[0] : (side == 1u ? t[1] : (side == 2u ? t[2] : t[3]));
}

// A row's index in the per-block arrays, kWallObjectRejected or kWallObjectOutside; p = x y z delta, q = e cell index row.
// j: the row's station -- the map's own, or the global station G = first[side] + j of an alignment's row; side: 0 on a map.
template <bool kJoint>
__device__ __forceinline__ uint32_t wo_decode(const WallObjectArgs &a, uint64_t i, uint4 &p, uint4 &q, long long &dq, uint32_t &j,
                                              uint32_t &k, uint32_t &side)
{
    const uint4 *r = reinterpret_cast<const uint4 *>(a.rows + i);
    p = r[0];
    q = r[1];
    dq = wall_check_fix(__uint_as_float(p.w));
    j = 0u; k = 0u; side = 0u;
    uint32_t c, first = 0u;
    if constexpr (kJoint) {
        side = GM_WALL_ROW_SIDE(q.y);
        if (side >= a.sides.n_sides) return kWallObjectRejected;   // before the side picks anything (n_sides <= 4)
        c = GM_WALL_ROW_CELL(q.y);
        if (wall_object_rejected(p.x, p.y, p.z, q.x, (int32_t)c, dq, wo_side_word(a.sides.cells, side))) return kWallObjectRejected;
        first = wo_side_word(a.sides.first, side);
    } else {
        c = q.y;
        if (wall_object_rejected(p.x, p.y, p.z, q.x, (int32_t)c, dq, a.cells)) return kWallObjectRejected;
    }
    j = first + c / a.nsec;   // (< total <= 2^32 - 1: the host refuses a longer alignment)
    k = c % a.nsec;
    const uint32_t J = j / a.bs;
    if (J < a.J0 || J - a.J0 >= a.nJ) return kWallObjectOutside;
    return (dq > 0 ? a.NB : 0u) + (J - a.J0) * a.NK + k / a.bk;   // < 2 NB
}

// ---- 2. bin ----

template <bool kJoint>
__device__ __forceinline__ void wo_bin(const WallObjectArgs a)
{
    uint32_t rej = 0u, outside = 0u;
    uint32_t per_side[4] = {0u, 0u, 0u, 0u};   // (joint) the rows of each side that are not rejected
    for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < a.n_rows; i += (uint64_t)gridDim.x * kCcThreads) {
        uint4 p, q;
        long long dq;
        uint32_t j, k, side;
        const uint32_t b = wo_decode<kJoint>(a, i, p, q, dq, j, k, side);
        if (b == kWallObjectRejected) ++rej;
        else if (b == kWallObjectOutside) ++outside;
        else atomicAdd(&a.cnt[b], 1u);
        if constexpr (kJoint) {
            if (b != kWallObjectRejected) {
#pragma unroll
                for (uint32_t s = 0; s < 4u; ++s) per_side[s] += side == s ? 1u : 0u;
            }
        }
    }
    rej = wave_sum(rej);
    outside = wave_sum(outside);
    if constexpr (kJoint) {
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) per_side[s] = wave_sum(per_side[s]);
    }
    if (lane_id() == 0) {
        if (rej) atomicAdd(&a.ctr[0], (unsigned long long)rej);
        if (outside) atomicAdd(&a.ctr[1], (unsigned long long)outside);
        if constexpr (kJoint) {
#pragma unroll
            for (uint32_t s = 0; s < 4u; ++s)
                if (per_side[s]) atomicAdd(&a.ctr[kWallObjectSideRows + s], (unsigned long long)per_side[s]);
        }
    }
}

// ---- 7. reduce ----

template <bool kJoint>
__device__ __forceinline__ void wo_reduce(const WallObjectArgs a)
{
    const uint32_t nsec = a.nsec, half = nsec / 2u;
    const int lane = lane_id();
    for (uint64_t i0 = (uint64_t)blockIdx.x * kCcThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); i0 < a.n_rows;
         i0 += (uint64_t)gridDim.x * kCcThreads) {
        const uint64_t i = i0 + lane;
        int slot = -1;
        uint32_t pts = 0u, smin = 0u, smax = 0u, kmin = 0u, kmax = 0u, tmin = 0u, tmax = 0u;
        uint32_t key[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // ~ordered(x, y, z), ordered(x, y, z), ~ordered(e), ordered(e)
        unsigned long long sum = 0ull, sx = 0ull, sy = 0ull, sz = 0ull, peak = 0ull;
        if (i < a.n_rows) {
            uint4 p, q;
            long long dq;
            uint32_t j, k, side;
            const uint32_t b = wo_decode<kJoint>(a, i, p, q, dq, j, k, side);
            const uint32_t r = b < kWallObjectOutside ? a.parent[b] : kCcNone;
            if (r != kCcNone) {
                slot = (int)a.slot[r];
                const uint32_t t = k + half < nsec ? k + half : k + half - nsec;
                const unsigned long long mag = dq < 0 ? 0ull - (unsigned long long)dq : (unsigned long long)dq;
                pts = 1u;
                smin = ~j; smax = j; kmin = ~k; kmax = k; tmin = ~t; tmax = t;
                const uint32_t ox = float_to_ordered(__uint_as_float(p.x)), oy = float_to_ordered(__uint_as_float(p.y)),
                               oz = float_to_ordered(__uint_as_float(p.z)), oe = float_to_ordered(__uint_as_float(q.x));
                key[0] = ~ox; key[1] = ~oy; key[2] = ~oz; key[3] = ox; key[4] = oy; key[5] = oz; key[6] = ~oe; key[7] = oe;
                sum = (unsigned long long)dq;
                sx = (unsigned long long)wall_object_fix16(__uint_as_float(p.x));
                sy = (unsigned long long)wall_object_fix16(__uint_as_float(p.y));
                sz = (unsigned long long)wall_object_fix16(__uint_as_float(p.z));
                peak = ((mag > 0xFFFFFFFFull ? 0xFFFFFFFFull : mag) << 32) | (uint32_t)~q.z;
            }
        }
        const WaveRuns run = wave_runs(slot);
        if (run.any) {
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t oc = __shfl_down(pts, o, kWave), o1 = __shfl_down(smin, o, kWave), o2 = __shfl_down(smax, o, kWave),
                               o3 = __shfl_down(kmin, o, kWave), o4 = __shfl_down(kmax, o, kWave), o5 = __shfl_down(tmin, o, kWave),
                               o6 = __shfl_down(tmax, o, kWave);
                uint32_t ok[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) ok[c] = __shfl_down(key[c], o, kWave);
                const unsigned long long os = __shfl_down(sum, o, kWave), ox = __shfl_down(sx, o, kWave), oy = __shfl_down(sy, o, kWave),
                                         oz = __shfl_down(sz, o, kWave), op = __shfl_down(peak, o, kWave);
                if (run.lane + o <= run.tail) {
                    pts += oc; sum += os; sx += ox; sy += oy; sz += oz;
                    smin = smin > o1 ? smin : o1; smax = smax > o2 ? smax : o2;
                    kmin = kmin > o3 ? kmin : o3; kmax = kmax > o4 ? kmax : o4;
                    tmin = tmin > o5 ? tmin : o5; tmax = tmax > o6 ? tmax : o6;
#pragma unroll
                    for (int c = 0; c < 8; ++c) key[c] = key[c] > ok[c] ? key[c] : ok[c];
                    peak = peak > op ? peak : op;
                }
            }
        }
        if (slot >= 0 && !run.dup) {
            WallObjectAcc *r = &a.acc[slot];
            atomicAdd(&r->points, (unsigned long long)pts);
            atomicAdd(&r->sum_delta, sum);
            atomicAdd(&r->sum_x, sx); atomicAdd(&r->sum_y, sy); atomicAdd(&r->sum_z, sz);
            atomicMax(&r->st_min_inv, smin); atomicMax(&r->st_max, smax);
            atomicMax(&r->k_min_inv, kmin); atomicMax(&r->k_max, kmax);
            atomicMax(&r->t_min_inv, tmin); atomicMax(&r->t_max, tmax);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMax(&r->box_min_inv[c], key[c]);
                atomicMax(&r->box_max[c], key[3 + c]);
            }
            atomicMax(&r->e_min_inv, key[6]); atomicMax(&r->e_max, key[7]);
            atomicMax(&r->peak_key, peak);
        }
    }
}

// ---- 9. rows ----

template <bool kJoint>
__device__ __forceinline__ void wo_rows(const WallObjectArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; i < a.n_rows; i += (uint64_t)gridDim.x * kCcThreads) {
        uint4 p, q;
        long long dq;
        uint32_t j, k, side;
        const uint32_t b = wo_decode<kJoint>(a, i, p, q, dq, j, k, side);
        const uint32_t r = b < kWallObjectOutside ? a.parent[b] : kCcNone;
        a.object_of_row[i] = r != kCcNone ? a.pos[a.slot[r]] : -1;
    }
}

// k_wall_objects_joint.hip: the joint instantiations, launched by k_wall_objects.hip's launch fronts when a.sides.n_sides > 0
void launch_wall_object_bin_joint(const WallObjectArgs &a, hipStream_t s);
void launch_wall_object_reduce_joint(const WallObjectArgs &a, hipStream_t s);
void launch_wall_object_rows_joint(const WallObjectArgs &a, hipStream_t s);

}  // namespace gm
