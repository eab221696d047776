// k_wall_add_checked.hip -- BUILD-DEFINED EXTENSION: an add less the check's changed rows (gm_wall_map_add_*_checked), the
// device side that is its own: k_wall_mark.  The add itself is k_wall_add_masked (k_wall.hip).
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_add_checked_np.py.  One thread per staged
// row, grid-stride in wave-uniform trips.  The row count is the check's device counter (or the stage call's host count),
// clamped to the rows the buffer holds; n_points is the device word n_valid (or the stage call's host count): no host
// round trip.  A row reads its delta and index (two of its eight words), takes its class by wall_mark_class
// (gm_internal.hpp), and a selected row sets bit `index` of the mask with a vector atomicOr on the
// 32-bit word: index < n_points <= the mask's bits, checked by the rule itself before the store.  The four row classes are
// counted by ballots into wave-uniform registers and leave as one integer atomic per class and block (block_row_sums,
// gm_point_stream.hpp).  Thread 0 of block 0 writes n_rows and n_points into the counter block.
#include "gm_internal.hpp"
#include "gm_point_stream.hpp"

namespace gm {

constexpr int kMarkThreads = 256;
constexpr int kMarkWaves = kMarkThreads / kWave;
constexpr uint32_t kMarkMaxBlocks = 64;       // rows are few beside points: a frame's changed points, 32 B each
constexpr uint32_t kMarkRowsPerBlock = 4096;

__global__ __launch_bounds__(kMarkThreads) void k_wall_mark(WallMarkArgs a)
{
    __shared__ uint32_t s_cls[4][kMarkWaves];
    const uint32_t n_points = a.n_ptr ? *a.n_ptr : a.n_host;
    uint32_t n_rows = a.n_rows_ptr ? (uint32_t)*a.n_rows_ptr : a.n_rows_host;
    n_rows = n_rows < a.rows_cap ? n_rows : a.rows_cap;
    const int lane = lane_id();
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};   // wave-uniform: selected negative, selected positive, kept, rejected
    const uint64_t stride = (uint64_t)gridDim.x * kMarkThreads;
    for (uint64_t r0 = (uint64_t)blockIdx.x * kMarkThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); r0 < n_rows; r0 += stride) {
        const uint64_t r = r0 + lane;
        uint32_t cls = 4u;   // past the end
        if (r < n_rows) {
            const float delta = a.rows[r].delta;
            const uint32_t index = a.rows[r].index;
            cls = wall_mark_class(__float_as_uint(delta), wall_check_fix(delta), index, n_points, a.skip, a.S);
            if (cls < 2u) atomicOr(&a.mask[index >> 5], 1u << (index & 31u));
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) cnt[k] += (uint32_t)__popcll(__ballot(cls == k));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_cls[k][threadIdx.x / kWave] = cnt[k];
    }
    block_row_sums(s_cls, [&](uint32_t k, unsigned long long v) {
        if (v) atomicAdd(&a.ctr[k], v);
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctr[9] = n_rows;
        a.ctr[10] = n_points;
    }
}

void launch_wall_mark(const WallMarkArgs &a, uint32_t n_cap, hipStream_t s)
{
    const uint64_t want = ((uint64_t)n_cap + kMarkRowsPerBlock - 1u) / kMarkRowsPerBlock;
    const uint32_t blocks = want < 1u ? 1u : (want > kMarkMaxBlocks ? kMarkMaxBlocks : (uint32_t)want);
    hipLaunchKernelGGL(k_wall_mark, dim3(blocks), dim3(kMarkThreads), 0, s, a);
}

}  // namespace gm
