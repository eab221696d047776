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
// The bodies of tiles and reduce, the two kernels that read a cell of the map, are gm_wall_regions.hpp's, shared with
// k_wall_regions_joint.hip (gm_wall_alignment_regions); here they read the map's own table.  No floating point anywhere.
#include <string.h>

#include "gm_wall_regions.hpp"

namespace gm {

static_assert(sizeof(WallRegionAcc) == 64 && sizeof(gm_wall_region) == 64, "64-byte records");

// ---- 1. tiles ----

__global__ __launch_bounds__(kCcThreads) void k_wall_region_tiles(WallRegionArgs a) { wr_tiles<WrMapCells>(a); }

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

__global__ __launch_bounds__(kCcThreads) void k_wall_region_reduce(WallRegionArgs a) { wr_reduce<WrMapCells>(a); }

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
    if (a.n_pieces) launch_wall_region_tiles_joint(a, s);
    else hipLaunchKernelGGL(k_wall_region_tiles, dim3(a.tiles_s * a.tiles_k), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_seams, dim3(cc_blocks(cc_seam_count(a.n, a.nsec, a.tiles_s, a.tiles_k))), dim3(kCcThreads),
                       0, s, a);
    hipLaunchKernelGGL(k_wall_region_flatten, dim3(cc_blocks(total)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_region_reduce(const WallRegionArgs &a, hipStream_t s)
{
    if (a.n_pieces) launch_wall_region_reduce_joint(a, s);
    else hipLaunchKernelGGL(k_wall_region_reduce, dim3(cc_blocks((uint64_t)a.n * a.nsec)), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_region_select, dim3(cc_blocks(a.ncomp)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_region_labels(const WallRegionArgs &a, uint64_t first, uint64_t n, int32_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_labels, dim3(cc_blocks(n)), dim3(kCcThreads), 0, s, a, first, n, out);
}

}  // namespace gm
