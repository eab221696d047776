// k_wall_joint.hip -- BUILD-DEFINED EXTENSION: the add of a frame that straddles joints of a wall alignment
// (gm_wall_alignment_add_*; include/gm_hip.h states the rule), the device side.
//
// k_wall_add's shape (gm_wall_add.hpp: kWallThreads per block, the wall_blocks grid, one streaming pass, the 80 KiB LDS
// table, the in-wave run merge, integer atomics only), over up to GM_WALL_JOINT_MAX_SIDES element maps at once:
//   1. every point is given its owner by the joint planes (gm_wall_joint.hpp states the rule; the planes in LDS);
//   2. the point runs its owner's chain and no other: a loop over the sides, wave-uniform, each trip joint_side_chain
//      (gm_wall_joint.hpp: wall_chain exactly as k_wall_add, k_wall_add_arc and k_wall_add_clothoid instantiate it).  A
//      wave whose lanes have different owners runs each of their chains once, under the lanes' mask; the side's frame
//      stays in scalar registers;
//   3. the run merge on the key side << 24 | cell (two sides have equal cell indices; a cell is < 2^24), every shuffle
//      wave-uniform; the run's head lane adds to the LDS table when the cell lies in its side's window -- the table's
//      GM_SURF_MAX_CELLS cells are dealt to the sides in order by the host -- and to the owner's map otherwise;
//   4. one flush per side, and the class counts to the owner's totals: a wave counts its points per (side, class) by
//      ballot into lane side * 4 + class, and the block's rows are summed by block_row_sums.
#include "gm_wall_add.hpp"
#include "gm_wall_joint.hpp"   // the side, the joint planes, the side's chain

namespace gm {

constexpr int kJointSides = GM_WALL_JOINT_MAX_SIDES;
constexpr int kJointCls = 4 * kJointSides;   // (side, class): mapped, outside, beyond_gate, plane per side

// kMasked (gm_wall_alignment_add_*_checked; k_wall_mark sets the bits): wall_add<kMasked>'s rule (k_wall.hip) over the sides.
// Bit i of m.words set = point i is SKIPPED, decided before its owner matters: it still runs its owner's chain (the stage
// call's residual), but takes cell -1 and no class ahead of the run merge, and reaches neither a table nor a side's totals.
// One wave-uniform 8-byte load of the mask per trip; the call's counts -- skipped, then the four classes summed over the
// sides -- go to m.ctr[4 ..], beside the mask block.  The unmasked instantiation carries none of it and keeps its name and
// its arguments.
template <bool kMasked>
__device__ __forceinline__ void wall_add_joint(const WallJointArgs &a, const WallMask<kMasked> m)
{
    constexpr int kRows = kJointCls + (kMasked ? 1 : 0);   // masked: row kJointCls counts the skipped points
    __shared__ unsigned long long s_sum[kWallCells];
    __shared__ uint32_t s_cnt[kWallCells];
    __shared__ uint32_t s_lo[kWallCells];
    __shared__ uint32_t s_hi[kWallCells];
    __shared__ uint32_t s_cls[kRows][kWallThreads / kWave];
    // the joint planes, read per point from LDS (a broadcast): 18 scalar registers less beside the sides' frames, which
    // keeps the kernel free of scalar spills
    __shared__ JointPlaneLds s_plane;
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    const uint32_t nsec = a.grid.n_sectors;
    const uint32_t nside = a.n_sides;
    const uint32_t wcells = a.lds_cells;   // <= kWallCells (the host deals the windows)
    const int lane = lane_id();

    for (uint32_t c = threadIdx.x; c < wcells; c += kWallThreads) { s_sum[c] = 0ull; s_cnt[c] = 0u; s_lo[c] = 0u; s_hi[c] = 0u; }
    if (threadIdx.x == 0) joint_planes_store(s_plane, a.planes);
    __syncthreads();

    uint32_t mine = 0u;   // lane c < 4 n_sides: this wave's points of class c & 3 owned by side c >> 2
    auto point = [&](uint64_t i, bool in, const float4 &q, uint32_t lab, uint32_t mbit) {
        const bool skip = kMasked && mbit;
        // joint_owner's loop, written out: through the call k_wall_add_joint takes two scalar spills and three vector
        // registers (SGPRs 104 -> 106, VGPRs 105 -> 108), k_wall_add_joint_masked two vector registers (113 -> 115)
        uint32_t owner = nside - 1u;
#pragma unroll
        for (int jn = kJointSides - 2; jn >= 0; --jn) {   // descending: the lowest joint with d < 0 stays
            if ((uint32_t)jn + 1u < nside) {              // (wave-uniform)
                if (joint_behind(q, s_plane[jn])) owner = (uint32_t)jn;
            }
        }
        float e = __builtin_nanf("");
        int cell = -1;      // the owner's cell j * n_sectors + k (< 2^24)
        int lidx = -1;      // the same cell in the block's LDS table, -1 outside the owner's window
        uint32_t kcls = kChainPlane;
#pragma unroll 1
        for (uint32_t s = 0; s < nside; ++s) {   // s is wave-uniform: the side's block is read once per wave
            if (!in || owner != s) continue;
            const WallJointSide &S = a.side[s];
            int64_t j = -1;
            float jl = 0.0f;
            uint32_t kk = 0u;
            const bool mapped = joint_side_chain(q, lab, S, a.grid, a.gate, e, jl, kk, j, kcls);
            if (mapped) {
                cell = (int)((uint32_t)j * nsec + kk);
                const float win_lo = (float)S.win_first, win_hi = (float)(S.win_first + (int32_t)S.win_stations);
                if (jl >= win_lo && jl < win_hi) lidx = (int)(S.lds_first + (uint32_t)((int32_t)jl - S.win_first) * nsec + kk);
            }
            if (a.element) a.element[i] = S.element;
        }
        if (skip) { cell = -1; lidx = -1; }
        if (in && a.res) a.res[i] = e;
        if (in && a.cell) a.cell[i] = cell;
        const uint32_t cidx = in && !skip ? owner * 4u + (kChainMapped - kcls) : 0xFFFFFFFFu;
        for (uint32_t c = 0; c < 4u * nside; ++c) {   // (wave-uniform)
            const uint32_t v = (uint32_t)__popcll(__ballot(cidx == c));
            if ((uint32_t)lane == c) mine += v;
        }
        uint32_t cn = 0u, lo = 0u, hi = 0u;
        unsigned long long sm = 0ull;
        if (cell >= 0) {
            cn = 1u;
            sm = (unsigned long long)(long long)__float2int_rn(__fmul_rn(e, kWallFix));
            hi = float_to_ordered(e);
            lo = ~hi;
        }
        const int key = cell >= 0 ? (int)(owner << 24 | (uint32_t)cell) : -1;
        if (surf_merge_runs(key, cn, sm, lo, hi)) {   // (lanes of one run share side and cell, hence lidx)
            if (lidx >= 0) {
                atomicAdd(&s_cnt[lidx], cn);
                atomicAdd(&s_sum[lidx], sm);
                atomicMax(&s_lo[lidx], lo);
                atomicMax(&s_hi[lidx], hi);
            } else {
#pragma unroll 1
                for (uint32_t s = 0; s < nside; ++s)
                    if (owner == s) wall_global_add(a.side[s].table, (uint64_t)cell, cn, sm, lo, hi);
            }
        }
    };
    uint32_t nskip = 0u;   // wave-uniform: this wave's skipped points
    if constexpr (kMasked) {
        // the slot's mask word rides with the slot's loads (wk: wave-uniform, < n <= 2^32): one scalar 8-byte load per wave
        // and trip; each lane keeps its own bit alone, so no scalar pair stays live across the trip
        stream_points_with<kWallThreads, kWallUnroll>(
            a.pts, a.labels, n,
            [&](uint64_t wk) {
                const unsigned long long mw = wk < n ? m.words[__builtin_amdgcn_readfirstlane((uint32_t)(wk >> 6))] : 0ull;
                nskip += (uint32_t)__popcll(mw);   // (no bit is set at or past n: k_wall_mark's rule)
                return (uint32_t)((mw >> lane) & 1ull);
            },
            point);
    } else {
        stream_points<kWallThreads, kWallUnroll>(a.pts, a.labels, n,
                                                 [&](uint64_t i, bool in, const float4 &q, uint32_t lab) { point(i, in, q, lab, 0u); });
    }
    __syncthreads();
    // one flush per side: the touched cells of its window, lane <-> cell.  A window lies inside its map.
#pragma unroll 1
    for (uint32_t s = 0; s < nside; ++s) {
        const WallJointSide &S = a.side[s];
        const uint32_t wc = S.win_stations * nsec;
        const int64_t base = (S.anchor + (int64_t)S.win_first) * (int64_t)nsec;
        for (uint32_t c = threadIdx.x; c < wc; c += kWallThreads) {
            const uint32_t l = S.lds_first + c;
            const uint32_t cn = s_cnt[l];
            if (!cn) continue;
            wall_global_add(S.table, (uint64_t)(base + (int64_t)c), cn, s_sum[l], s_lo[l], s_hi[l]);
        }
    }
    // class counts: one atomic per (side, class) and block, to the owner's totals
    if (kMasked && lane == kJointCls) mine = nskip;
    if (lane < kRows) s_cls[lane][threadIdx.x / kWave] = mine;
    block_row_sums(s_cls, [&](uint32_t k, unsigned long long v) {
#pragma unroll 1
        for (uint32_t s = 0; s < nside; ++s)
            if (v && (k >> 2) == s) atomicAdd(&a.side[s].table.totals[k & 3u], v);
        if constexpr (kMasked) {   // skipped | mapped, outside, beyond_gate, plane
            if (v) atomicAdd(&m.ctr[k == (uint32_t)kJointCls ? 4u : 5u + (k & 3u)], v);
        }
    });
}

__global__ __launch_bounds__(kWallThreads) void k_wall_add_joint(WallJointArgs a)
{
    wall_add_joint<false>(a, WallMask<false>());
}
__global__ __launch_bounds__(kWallThreads) void k_wall_add_joint_masked(WallJointArgs a, WallMask<true> m)
{
    wall_add_joint<true>(a, m);
}

void launch_wall_add_joint(const WallJointArgs &a, uint32_t n_cap, uint32_t points_per_block, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_add_joint, dim3(wall_blocks(n_cap, points_per_block)), dim3(kWallThreads), 0, s, a);
}
void launch_wall_add_joint_masked(const WallJointArgs &a, const unsigned long long *mask, unsigned long long *ctr, uint32_t n_cap,
                                  uint32_t points_per_block, hipStream_t s)
{
    WallMask<true> m;
    m.words = mask;
    m.ctr = ctr;
    hipLaunchKernelGGL(k_wall_add_joint_masked, dim3(wall_blocks(n_cap, points_per_block)), dim3(kWallThreads), 0, s, a, m);
}

}  // namespace gm
