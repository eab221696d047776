// gm_wall_align.hpp -- what the align kernels of a single map (k_wall_align.hip) and of a wall alignment
// (k_wall_align_joint.hip) share: the bin kernels' block shape and run merge, and the two halves of the values kernels --
// the patch's value f and a map cell's value m.  The score kernel is k_wall_align.hip's alone: it never sees the axis.
#pragma once

#include "gm_internal.hpp"
#include "gm_point_stream.hpp"

namespace gm {

constexpr int kAlignBinThreads = 1024;
constexpr int kAlignBinUnroll = 2;
constexpr uint32_t kAlignCells = GM_WALL_ALIGN_MAX_PATCH_CELLS;
constexpr int kAlignThreads = 256;

// runs of one patch cell folded into the run's head lane (gm_device.hpp: wave_runs and its ladder)
__device__ __forceinline__ bool align_merge_runs(int cell, uint32_t &cn, unsigned long long &sm)
{
    const WaveRuns r = wave_runs(cell);
    if (r.any) {
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t ocn = __shfl_down(cn, o, kWave);
            const unsigned long long osm = __shfl_down(sm, o, kWave);
            if (r.lane + o <= r.tail) { cn += ocn; sm += osm; }
        }
    }
    return cell >= 0 && !r.dup;
}

// The f half of a values kernel: patch cell i (< 2P n_sectors) becomes f[i]; returns whether the cell is usable.
__device__ __forceinline__ uint32_t align_patch_value(const uint32_t *p_cnt, const unsigned long long *p_sum, uint32_t min_frame_count,
                                                      int32_t *f, uint32_t i)
{
    const uint32_t cn = p_cnt[i];
    int32_t v = kWallAlignNone;
    uint32_t usable = 0u;
    if (cn >= min_frame_count) {
        v = (int32_t)((long long)p_sum[i] / (long long)cn);   // |v| <= 2^23
        usable = 1u;
    }
    f[i] = v;
    return usable;
}
// the closing count of the f half: one atomic per wave into the usable-cells word
__device__ __forceinline__ void align_patch_usable(uint32_t usable, unsigned long long *ctr5)
{
    usable = wave_sum(usable);
    if (lane_id() == 0 && usable) atomicAdd(ctr5, (unsigned long long)usable);
}
// The m of map cell g (< the map's n_stations * n_sectors): the count first, the sum only for a usable cell.
__device__ __forceinline__ int32_t align_map_value(const WallTable &t, uint64_t g, uint32_t min_count)
{
    const uint32_t cn = t.cnt[g];
    if (cn < min_count) return kWallAlignNone;
    const long long q = (long long)t.sum[g] / (long long)cn;
    return q > kWallAlignSat ? kWallAlignSat : (q < -kWallAlignSat ? -kWallAlignSat : (int32_t)q);
}

}  // namespace gm
