// k_wall_align_joint.hip -- BUILD-DEFINED EXTENSION: a frame's chainage and roll against a wall alignment
// (gm_wall_alignment_align_*; include/gm_hip.h states the rule), the device side.  The CPU twin is
// tests/wall_alignment_align_np.py.
//
// Three launches per align, as on a single map (k_wall_align.hip):
//   k_wall_align_bin_joint     k_wall_align_bin's skeleton (gm_wall_align.hpp, gm_point_stream.hpp: 1024 threads, one block
//                              per CU, the 96 KiB block-private LDS patch, the in-wave run merge, the integer flush) over up
//                              to GM_WALL_JOINT_MAX_SIDES element maps at once:
//                                1. every point is given its owner by joint_owner (gm_wall_joint.hpp; the planes in LDS);
//                                2. it runs its owner's chain and no other: a wave-uniform loop over the sides, each trip
//                                   joint_side_chain_in under the align's gate with the PATCH as the range:
//                                   jr = row0[owner] + jl in 64-bit integers, in range iff 0 <= jr < 2P.  The side's frame
//                                   stays in scalar registers;
//                                3. the patch cell jr * n_sectors + k is the run merge's key: two sides never share a patch
//                                   row's cell by accident, the patch is one image;
//                                4. the class counts per (side, class): one ballot per pair and point into lane
//                                   side * 4 + class, summed per block by block_row_sums; thread k adds its row to the
//                                   side's word and to the summed class k & 3.
//   k_wall_align_values_joint  k_wall_align_values with the m rows resolved through the pieces: image row r is global
//                              station G = g0 + r, read from the piece with first_row <= G < first_row + n_stations, and
//                              kWallAlignNone where there is none.  Behind the wait on the adds of every piece's map.
//   k_wall_align_score         k_wall_align.hip's, unchanged: it sees f, m and the table alone.
// No floating-point atomics, no ticket, no host round trip.  Every patch index is jr * n_sectors + k with 0 <= jr < 2P,
// k < n_sectors (2P n_sectors <= kAlignCells: the host checks the parameters); every m index is below (2P + 2A) n_sectors;
// every gather index is j * n_sectors + k with 0 <= j < the piece's n_stations; owner < n_sides <= GM_WALL_JOINT_MAX_SIDES;
// every per-point store index is a point index < n.
#include <string.h>

#include "gm_wall_align.hpp"
#include "gm_wall_joint.hpp"   // the side, the owner rule, the side's chain

namespace gm {

constexpr int kAlignJointSides = GM_WALL_JOINT_MAX_SIDES;
constexpr int kAlignJointCls = 4 * kAlignJointSides;   // (side, class): wall_chain's order per side

// The stage call's per-point outputs (each may be nullptr), read from LDS behind the one scalar word that says whether
// there is any: six scalar registers less beside the sides' frames in the frame path (k_wall_check_joint.hip does the same).
struct WallAlignJointOut {
    float *res;
    int32_t *cell;
    int32_t *element;
};

__global__ __launch_bounds__(kAlignBinThreads) void k_wall_align_bin_joint(WallAlignJointArgs a, uint32_t outputs)
{
    __shared__ unsigned long long s_sum[kAlignCells];
    __shared__ uint32_t s_cnt[kAlignCells];
    __shared__ uint32_t s_cls[kAlignJointCls][kAlignBinThreads / kWave];
    __shared__ JointPlaneLds s_plane;
    __shared__ WallAlignJointOut s_out;
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    const uint32_t nsec = a.grid.n_sectors;
    const uint32_t nside = a.n_sides;
    const uint32_t pcells = 2u * a.P * nsec;   // <= kAlignCells (the host checks the parameters)
    const int64_t rows2p = 2 * (int64_t)a.P;
    const int lane = lane_id();

    for (uint32_t c = threadIdx.x; c < pcells; c += kAlignBinThreads) { s_sum[c] = 0ull; s_cnt[c] = 0u; }
    if (threadIdx.x == 0) {
        joint_planes_store(s_plane, a.planes);
        s_out = WallAlignJointOut{a.res, a.cell, a.element};
    }
    __syncthreads();

    uint32_t mine = 0u;   // lane c < 4 n_sides: this wave's points of class c & 3 owned by side c >> 2
    stream_points<kAlignBinThreads, kAlignBinUnroll>(a.pts, a.labels, n, [&](uint64_t i, bool in, const float4 &q, uint32_t lab) {
        const uint32_t owner = joint_owner(q, s_plane, nside);
        float e = __builtin_nanf("");
        int cell = -1;      // jr * n_sectors + k (< 8192)
        uint32_t kcls = kChainPlane;
#pragma unroll 1
        for (uint32_t s = 0; s < nside; ++s) {   // s is wave-uniform: the side's block is read once per wave
            if (!in || owner != s) continue;
            const WallJointSide &S = a.side[s];
            const int64_t row0 = (int64_t)a.row0[s];
            int64_t jr = -1;
            float jl = 0.0f;
            uint32_t kk = 0u;
            const bool binned = joint_side_chain_in(
                q, lab, S, a.grid, a.gate,
                [&](const JointChainArgs &, float x) {
                    jr = fabsf(x) < 4.0e18f ? row0 + (int64_t)x : -1;
                    return jr >= 0 && jr < rows2p;
                },
                e, jl, kk, kcls);
            if (binned) cell = (int)((uint32_t)jr * nsec + kk);
        }
        if (outputs) {   // (wave-uniform: the stage call)
            const WallAlignJointOut o = s_out;
            if (in && o.res) o.res[i] = e;
            if (in && o.cell) o.cell[i] = cell;
            if (in && o.element) o.element[i] = a.side[0].element + (int32_t)owner;   // (the sides are consecutive elements)
        }
        const uint32_t cidx = in ? owner * 4u + kcls : 0xFFFFFFFFu;
        for (uint32_t c = 0; c < 4u * nside; ++c) {   // (wave-uniform)
            const uint32_t v = (uint32_t)__popcll(__ballot(cidx == c));
            if ((uint32_t)lane == c) mine += v;
        }
        uint32_t cn = 0u;
        unsigned long long sm = 0ull;
        if (cell >= 0) {
            cn = 1u;
            sm = (unsigned long long)wall_check_fix(e);
        }
        if (align_merge_runs(cell, cn, sm)) {
            atomicAdd(&s_cnt[cell], cn);
            atomicAdd(&s_sum[cell], sm);
        }
    });
    __syncthreads();
    // flush the touched cells, lane <-> cell
    for (uint32_t c = threadIdx.x; c < pcells; c += kAlignBinThreads) {
        const uint32_t cn = s_cnt[c];
        if (!cn) continue;
        atomicAdd(&a.p_cnt[c], cn);
        atomicAdd(&a.p_sum[c], s_sum[c]);
    }
    // class counts: one atomic per (side, class) and block to the side's word, one to the summed class
    if (lane < kAlignJointCls) s_cls[lane][threadIdx.x / kWave] = mine;
    block_row_sums(s_cls, [&](uint32_t k, unsigned long long v) {
        if (!v) return;
        atomicAdd(&a.ctr[kWallAlignCounters + k], v);
        atomicAdd(&a.ctr[k & 3u], v);
    });
    if (blockIdx.x == 0 && threadIdx.x == kAlignJointCls) a.ctr[4] = n;
}

__global__ __launch_bounds__(kAlignThreads) void k_wall_align_values_joint(WallAlignJointValuesArgs a)
{
    const uint32_t nsec = a.n_sectors;
    const uint32_t pcells = 2u * a.P * nsec;
    const uint32_t mcells = (2u * a.P + 2u * a.A) * nsec;
    uint32_t usable = 0u;
    for (uint32_t i = blockIdx.x * kAlignThreads + threadIdx.x; i < pcells + mcells; i += gridDim.x * kAlignThreads) {
        if (i < pcells) {
            usable += align_patch_value(a.p_cnt, a.p_sum, a.min_frame_count, a.f, i);
        } else {
            const uint32_t c = i - pcells;
            const int64_t G = a.g0 + (int64_t)(c / nsec);   // (|g0| < 2^62: no overflow)
            int32_t v = kWallAlignNone;
#pragma unroll 1
            for (uint32_t p = 0; p < a.n_pieces; ++p) {   // (p is uniform: the piece is read through uniform addresses)
                const WallAlignPiece &pc = a.piece[p];
                const int64_t j = G - pc.first_row;
                if (j >= 0 && j < (int64_t)pc.n_stations)
                    v = align_map_value(pc.table, (uint64_t)j * nsec + c % nsec, a.min_count);   // g < the piece's n_stations * n_sectors
            }
            a.m[c] = v;
        }
    }
    align_patch_usable(usable, &a.ctr[5]);
}

void launch_wall_align_bin_joint(const WallAlignJointArgs &a, uint32_t n_cap, hipStream_t s)
{
    const uint32_t outputs = (a.res || a.cell || a.element) ? 1u : 0u;
    hipLaunchKernelGGL(k_wall_align_bin_joint, dim3(wall_blocks(n_cap, 0u)), dim3(kAlignBinThreads), 0, s, a, outputs);
}

void launch_wall_align_values_joint(const WallAlignJointValuesArgs &a, hipStream_t s)
{
    const uint32_t cells = (4u * a.P + 2u * a.A) * a.n_sectors;
    hipLaunchKernelGGL(k_wall_align_values_joint, dim3((cells + kAlignThreads - 1) / kAlignThreads), dim3(kAlignThreads), 0, s, a);
}

}  // namespace gm
