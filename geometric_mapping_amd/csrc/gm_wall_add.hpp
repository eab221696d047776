// gm_wall_add.hpp -- what the kernels that add points to a wall map share (k_wall.hip's k_wall_add*, k_wall_joint.hip's
// k_wall_add_joint): the launch shape, the fixed-point scale and the map's integer update.
#pragma once

#include "gm_internal.hpp"
#include "gm_point_stream.hpp"

namespace gm {

constexpr int kWallThreads = 1024;
constexpr uint32_t kWallMaxBlocks = 256;          // one per CU
constexpr int kWallUnroll = 2;
constexpr uint32_t kWallCells = GM_SURF_MAX_CELLS;
constexpr float kWallFix = 1048576.0f;   // 2^20, as k_surface.hip

__device__ __forceinline__ void wall_global_add(const WallTable &T, uint64_t c, uint32_t cn, unsigned long long sm, uint32_t lo,
                                                uint32_t hi)
{
    atomicAdd(&T.cnt[c], cn);
    atomicAdd(&T.sum[c], sm);
    atomicMax(&T.lo[c], lo);
    atomicMax(&T.hi[c], hi);
}

// the mask of a checked add (k_wall_add*_masked, k_wall_add_joint_masked): bit i of words set = point i is skipped; the
// unmasked instantiations carry nothing
template <bool kMasked>
struct WallMask {};
template <>
struct WallMask<true> {
    const unsigned long long *words;   // ceil(n / 64) words at least
    unsigned long long *ctr;           // [kWallAddCheckedCounters]
};

}  // namespace gm
