// k_wall_objects.hip -- BUILD-DEFINED EXTENSION: a check's changed points as objects (gm_wall_map_check_objects,
// gm_wall_check_objects), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_objects_np.py.  The staged rows of a
// check are binned into map-anchored blocks of bs x bk cells, the blocks that hold enough rows of one sign are labelled as
// connected components -- positive and negative rows apart, as two PLANES of the same window: plane p's block w lives at
// p * NB + w in every per-block array, and parents index that space, so one union-find serves both -- and every row adds
// into the record of its component.  The labelling is gm_gridcc.hpp's, which states the union-find and the memory
// ordering of the seams launch:
//   1. (memset)               the block counts and the counters.
//   2. k_wall_object_bin      one thread per row: decode, count rejected / outside_window, one integer atomic on cnt.
//   3. k_wall_object_tiles    one workgroup per tile of ts x tk <= 4096 window blocks, plane after plane: flag
//      cnt >= min_block_points and label the tile (cc_label_tile).  Counts the flagged pairs and the sparse rows.
//   4. k_wall_object_seams    one thread per border block and plane (cc_seam); flagged blocks of one plane join.
//   5. k_wall_object_flatten  cc_flatten over the 2 NB pairs.  The component count goes to the host, which sizes the
//      accumulators.
//   6. k_wall_object_blocks   every flagged pair adds 1 to its slot's `blocks`; the root writes label and plane.
//   7. k_wall_object_reduce   one thread per row: its slot through parent and slot, then integer atomics only into the
//      128-byte accumulator (add: points, sum_delta, the three centroid sums; max: the six extents, the eight ordered()
//      keys of box and e, minima kept inverted; one 64-bit max of |dq| << 32 | ~index: the peak).  Runs of one slot in
//      consecutive lanes are merged in the wave first (wave_runs, gm_device.hpp); the loop's trips are wave-uniform, so every lane is
//      present at the shuffles.
//   8. k_wall_object_select   one thread per slot: components of >= min_points rows become gm_wall_object records, in the
//      order the slots come (the host sorts the copied list by label and sign); small / in_object row counts.
//   9. k_wall_object_rows     only when the caller asks for object_of_row, after the host has uploaded slot -> position.
// Every store index is a row index < n_rows, an index < 2 NB or a slot < the component count by construction; nothing is
// clamped.  No floating-point arithmetic after the two fixed-point conversions of a row.
// The decode and the bodies of the three kernels that read a row (bin, reduce, rows) are gm_wall_objects.hpp's, shared with
// k_wall_objects_joint.hip (gm_wall_alignment_check_objects: rows decoded onto the alignment's global stations); the
// launch fronts below pick that file's instantiations when the arguments carry a side table.
#include <stddef.h>
#include <string.h>

#include "gm_wall_objects.hpp"

namespace gm {

static_assert(sizeof(WallObjectAcc) == 128 && sizeof(gm_wall_object) == 128 && sizeof(gm_wall_check_point) == 32, "record sizes");
// k_wall_object_select writes box_min, box_max, e_min, e_max as eight consecutive 32-bit words
static_assert(offsetof(gm_wall_object, box_min) == 88 && offsetof(gm_wall_object, box_max) == 100 && offsetof(gm_wall_object, e_min) == 112 &&
                  offsetof(gm_wall_object, e_max) == 116 && sizeof(float) == sizeof(uint32_t),
              "the eight floats of gm_wall_object are contiguous");

// ---- 2. bin ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_bin(WallObjectArgs a) { wo_bin<false>(a); }

// ---- 3. tiles ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_tiles(WallObjectArgs a)
{
    __shared__ uint32_t L[kWallObjectTileBlocks];
    __shared__ uint8_t S[kWallObjectTileBlocks];
    __shared__ uint32_t s_cls[4];
    const uint32_t ts = a.ts, tk = a.tk, NK = a.NK, cells = ts * tk;   // <= kWallObjectTileBlocks (the host checks)
    const uint32_t j0 = (blockIdx.x / a.tiles_k) * ts, k0 = (blockIdx.x % a.tiles_k) * tk;
    if (threadIdx.x < 4) s_cls[threadIdx.x] = 0u;
    uint32_t cls[3] = {0u, 0u, 0u};   // flagged_neg, flagged_pos, sparse rows
    for (uint32_t plane = 0; plane < 2u; ++plane) {
        const uint32_t base = plane * a.NB;
        for (uint32_t l = threadIdx.x; l < cells; l += kCcThreads) {
            const uint32_t J = j0 + l / tk, K = k0 + l % tk;
            bool flag = false;
            if (J < a.nJ && K < NK) {
                const uint32_t w = base + J * NK + K, c = a.cnt[w];
                flag = c >= a.min_block_points;   // (min_block_points >= 1: an empty block is never flagged)
                if (flag) ++cls[plane];
                else {
                    cls[2] += c;
                    a.parent[w] = kCcNone;
                }
            }
            S[l] = flag ? 1 : 0;
            L[l] = l;
        }
        cc_label_tile(L, S, cells, tk, a.conn8 != 0u, a.parent, [=](uint32_t r, uint32_t c) { return base + (j0 + r) * NK + k0 + c; });
        __syncthreads();   // the next plane reuses L and S
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = wave_sum(cls[k]);
        if (lane_id() == 0 && v) atomicAdd(&s_cls[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cls[threadIdx.x])
        atomicAdd(&a.ctr[threadIdx.x == 2 ? 2 : 5 + threadIdx.x], (unsigned long long)s_cls[threadIdx.x]);
}

// ---- 4. seams ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_seams(WallObjectArgs a)
{
    const uint64_t per = cc_seam_count(a.nJ, a.NK, a.tiles_s, a.tiles_k);
    for (uint64_t g = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; g < 2u * per; g += (uint64_t)gridDim.x * kCcThreads)
        cc_seam(g < per ? g : g - per, a.nJ, a.NK, a.ts, a.tk, a.tiles_k, a.conn8 != 0u, g < per ? 0u : a.NB,
                [&a](uint32_t x, uint32_t y) {   // entries of one plane join when both are flagged
                    if (cc_joinable(a.parent, x, y)) cc_union(a.parent, x, y);
                });
}

// ---- 5. flatten ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_flatten(WallObjectArgs a)
{
    cc_flatten(a.parent, a.slot, 2ull * a.NB, &a.ctr[7]);
}

// ---- 6. blocks ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_blocks(WallObjectArgs a)
{
    const uint64_t total = 2ull * a.NB;
    for (uint64_t w = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; w < total; w += (uint64_t)gridDim.x * kCcThreads) {
        const uint32_t r = a.parent[w];
        if (r == kCcNone) continue;
        WallObjectAcc *acc = &a.acc[a.slot[r]];
        atomicAdd(&acc->blocks, 1u);
        if (r == (uint32_t)w) {   // the root alone
            const uint32_t plane = w >= a.NB ? 1u : 0u;
            acc->label = a.J0 * a.NK + ((uint32_t)w - plane * a.NB);
            acc->plane = plane;
        }
    }
}

// ---- 7. reduce ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_reduce(WallObjectArgs a) { wo_reduce<false>(a); }

// ---- 8. select ----

// the bits of ordered_to_float(o)
__device__ __forceinline__ uint32_t wo_unordered(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }

__global__ __launch_bounds__(kCcThreads) void k_wall_object_select(WallObjectArgs a)
{
    uint32_t small = 0u, in_object = 0u;
    for (uint32_t s = blockIdx.x * kCcThreads + threadIdx.x; s < a.ncomp; s += gridDim.x * kCcThreads) {
        const WallObjectAcc *r = &a.acc[s];
        const unsigned long long pts = r->points;
        if (pts < a.min_points) {
            small += (uint32_t)pts;
            continue;
        }
        in_object += (uint32_t)pts;
        const uint32_t at = (uint32_t)atomicAdd(&a.ctr[8], 1ull);   // (< ncomp: one per slot at the most)
        const unsigned long long key = r->peak_key;
        const long long mag = (long long)(key >> 32);
        const uint32_t plane = r->plane;
        gm_wall_object *g = &a.out[at];
        g->label = r->label;
        g->sign = plane ? 1 : -1;
        g->blocks = r->blocks;
        g->peak_index = ~(uint32_t)key;
        g->station_min = ~r->st_min_inv; g->station_max = r->st_max;
        g->sector_min = ~r->k_min_inv; g->sector_max = r->k_max;
        g->sector_min_turned = ~r->t_min_inv; g->sector_max_turned = r->t_max;
        g->points = pts;
        g->peak = plane ? mag : -mag;   // (a plane holds one sign, and |dq| <= 2^31 is never saturated)
        g->sum_delta = (long long)r->sum_delta;
        g->sum_x = (long long)r->sum_x; g->sum_y = (long long)r->sum_y; g->sum_z = (long long)r->sum_z;
        // The eight floats are decoded and stored as bits through one pointer; the static_assert above pins their layout.
        // Workaround, to be removed with a later compiler: with `g->box_min[c] = ordered_to_float(~r->box_min_inv[c]);
        // g->box_max[c] = ordered_to_float(r->box_max[c]);` in this loop, hipcc of ROCm 7.2.0 (clang 22.0.0git, roc-7.2.0
        // 26014) -O3 --offload-arch=gfx950 dies with a segmentation fault in "AMDGPU DAG->DAG Pattern Instruction
        // Selection" (MachineRegisterInfo::constrainRegClass) on this kernel; this kernel alone in a file reproduces it.
        uint32_t *fb = reinterpret_cast<uint32_t *>(g->box_min);   // box_min[3] box_max[3] e_min e_max
        for (int c = 0; c < 3; ++c) {
            fb[c] = wo_unordered(~r->box_min_inv[c]);
            fb[3 + c] = wo_unordered(r->box_max[c]);
        }
        fb[6] = wo_unordered(~r->e_min_inv);
        fb[7] = wo_unordered(r->e_max);
        g->reserved = 0ull;
        a.out_slot[at] = s;
    }
    small = wave_sum(small);
    in_object = wave_sum(in_object);
    if (lane_id() == 0) {
        if (small) atomicAdd(&a.ctr[3], (unsigned long long)small);
        if (in_object) atomicAdd(&a.ctr[4], (unsigned long long)in_object);
    }
}

// ---- 9. rows ----

__global__ __launch_bounds__(kCcThreads) void k_wall_object_rows(WallObjectArgs a) { wo_rows<false>(a); }

void launch_wall_object_label(const WallObjectArgs &a, hipStream_t s)
{
    if (a.sides.n_sides) launch_wall_object_bin_joint(a, s);
    else hipLaunchKernelGGL(k_wall_object_bin, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_object_tiles, dim3(a.tiles_s * a.tiles_k), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_object_seams, dim3(cc_blocks(2u * cc_seam_count(a.nJ, a.NK, a.tiles_s, a.tiles_k))), dim3(kCcThreads),
                       0, s, a);
    hipLaunchKernelGGL(k_wall_object_flatten, dim3(cc_blocks(2ull * a.NB)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_object_reduce(const WallObjectArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_object_blocks, dim3(cc_blocks(2ull * a.NB)), dim3(kCcThreads), 0, s, a);
    if (a.sides.n_sides) launch_wall_object_reduce_joint(a, s);
    else hipLaunchKernelGGL(k_wall_object_reduce, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
    hipLaunchKernelGGL(k_wall_object_select, dim3(cc_blocks(a.ncomp)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_object_rows(const WallObjectArgs &a, hipStream_t s)
{
    if (a.sides.n_sides) launch_wall_object_rows_joint(a, s);
    else hipLaunchKernelGGL(k_wall_object_rows, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
}

}  // namespace gm
