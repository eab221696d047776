// k_wall_cloud.hip -- BUILD-DEFINED EXTENSION: the persistent wall map as an ordered, decimated point list
// (gm_wall_map_cloud), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_cloud_np.py.  The host walks the
// window in chunks of whole block rows (gm_wall.hip); per chunk:
//   1. k_wall_cloud_merge     (skipped when bs = bk = 1: the table is then the source)  one merged accumulator per block
//      of the chunk -- sum i64, count u64, the two keys, the number of non-empty cells -- into scratch the host has
//      zeroed.  A work item is (block row, segment of up to kWcRows stations, sector), the sector fastest: lanes take
//      consecutive sectors, so the SoA table is read coalesced, and each lane sums its sector over the segment's station
//      rows.  Runs of one block in consecutive lanes are merged in the wave (surf_merge_runs' segmented reduction with a
//      64-bit count: wc_merge_runs); the run's head lane adds what is left with integer atomics.  Integers only: the
//      result does not depend on the grid or the order.
//   2. k_compact<WallCloudPred, WallCloudEmit>  (gm_compact.hpp)  the predicate loads the block's accumulators as its
//      payload and keeps count >= min_count; the emit step builds the 40-byte record at the survivor's rank in the
//      staging buffer: survivors leave in block order from one launch.  The two other classes are counted in LDS and
//      added once per class and block.  The position is fp64 with explicit roundings (__dmul_rn / __dadd_rn: nothing
//      the build flags could contract) on a direction table the host computed; no fp64 trigonometry on the device.
#include <string.h>

#include "gm_compact.hpp"
#include "gm_internal.hpp"
#include "gm_wall_cloud_emit.hpp"

namespace gm {

static_assert(sizeof(gm_wall_cloud_point) == 40, "a 40-byte PointCloud2 row");
constexpr int kWcThreads = 256;
constexpr uint32_t kWcMaxBlocks = 4096;
constexpr uint32_t kWcRows = 32;   // station rows one lane sums: a block of many stations is spread over several lanes

// ---- 1. merge ----

// surf_merge_runs (gm_device.hpp) with a 64-bit count and the number of non-empty cells beside it: runs of one block in
// consecutive lanes -> the run's head lane (wave_runs).  Returns whether this lane still has to add its (merged)
// contribution.
__device__ __forceinline__ bool wc_merge_runs(int blk, unsigned long long &cn, unsigned long long &sm, uint32_t &lo, uint32_t &hi,
                                              uint32_t &cells)
{
    const WaveRuns r = wave_runs(blk);
    if (r.any) {
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned long long ocn = __shfl_down(cn, o, kWave), osm = __shfl_down(sm, o, kWave);
            const uint32_t olo = __shfl_down(lo, o, kWave), ohi = __shfl_down(hi, o, kWave), oce = __shfl_down(cells, o, kWave);
            if (r.lane + o <= r.tail) {
                cn += ocn; sm += osm; cells += oce;
                lo = lo > olo ? lo : olo;
                hi = hi > ohi ? hi : ohi;
            }
        }
    }
    return blk >= 0 && !r.dup;
}

__global__ __launch_bounds__(kWcThreads) void k_wall_cloud_merge(WallCloudArgs a, uint32_t nseg, uint32_t items)
{
    const int lane = lane_id();
    const uint32_t nsec = a.nsec;
    // wave-uniform trips (the run merge shuffles across the wave)
    for (uint32_t w0 = blockIdx.x * kWcThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < items; w0 += gridDim.x * kWcThreads) {
        const uint32_t it = w0 + lane;
        int blk = -1;
        uint32_t cells = 0u, lo = 0u, hi = 0u;
        unsigned long long sm = 0ull, cn = 0ull;
        if (it < items) {
            const uint32_t k = it % nsec, r = it / nsec, seg = r % nseg, jl = r / nseg;
            const uint32_t j0 = (a.J0 + jl) * a.bs;                       // window-relative, < n
            const uint32_t end = a.n - j0 < a.bs ? a.n : j0 + a.bs;       // the block row's stations end here (ragged last row)
            const uint32_t jb = j0 + seg * kWcRows, je = jb + kWcRows;     // (a segment past the ragged end: no trip)
            for (uint32_t j = jb; j < end && j < je; ++j) {
                const uint64_t c = a.first + (uint64_t)j * nsec + k;
                const uint32_t cc = a.map.cnt[c];
                if (cc) {
                    const uint32_t l = a.map.lo[c], h = a.map.hi[c];
                    cn += cc;
                    sm += a.map.sum[c];
                    lo = lo > l ? lo : l;
                    hi = hi > h ? hi : h;
                    ++cells;
                }
            }
            blk = (int)(jl * a.NK + k / a.bk);
        }
        if (wc_merge_runs(blk, cn, sm, lo, hi, cells) && cells) {
            atomicAdd(&a.acc_sum[blk], sm);
            atomicAdd(&a.acc_cnt[blk], cn);
            atomicMax(&a.acc_lo[blk], lo);
            atomicMax(&a.acc_hi[blk], hi);
            atomicAdd(&a.acc_cells[blk], cells);
        }
    }
}

// ---- 2. compact + emit ----
// (WallCloudPred, WallCloudEmit: gm_wall_cloud_emit.hpp, shared with the mesh's vertex pass in k_wall_mesh.hip)

void launch_wall_cloud_merge(const WallCloudArgs &a, hipStream_t s)
{
    const uint32_t nseg = (a.bs + kWcRows - 1u) / kWcRows;
    const uint64_t items = (uint64_t)a.nJ * nseg * a.nsec;   // < 2^25: nJ * bs < 2 n, n * nsec <= 2^24
    uint64_t b = (items + kWcThreads - 1) / kWcThreads;
    b = b < 1 ? 1 : (b > kWcMaxBlocks ? kWcMaxBlocks : b);
    hipLaunchKernelGGL(k_wall_cloud_merge, dim3((uint32_t)b), dim3(kWcThreads), 0, s, a, nseg, (uint32_t)items);
}

// the compaction's one front: the emit step of the axis' kind
void launch_wall_cloud_compact(const WallCloudArgs &a, const WallCloudAxis &axis, const ScanState &st, hipStream_t s)
{
    if (axis.kind == kAxisStraight) wall_cloud_launch(a, WallCloudEmit{a}, st, s);
    else if (axis.kind == kAxisArc) wall_cloud_launch(a, WallCloudEmitArc{a, WallCloudOnArc{axis.arc}}, st, s);
    else wall_cloud_launch(a, WallCloudEmitClothoid{a, WallCloudOnClothoid{wall_cloud_clothoid(axis)}}, st, s);
}

}  // namespace gm
