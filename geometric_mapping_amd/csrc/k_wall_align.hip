// k_wall_align.hip -- BUILD-DEFINED EXTENSION: a frame's chainage and roll against the persistent wall map
// (gm_wall_map_align_*), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_align_np.py.  Three launches per align,
// everything from a point's residual on in integers:
//   k_wall_align_bin     k_wall_add on a patch instead of the map: the same point stream and class counts
//                        (gm_point_stream.hpp) and chain head (wall_chain, gm_device.hpp) under the patch's range, the
//                        in-wave run merge, LDS integer atomics into a block-private patch table of 2P x n_sectors <= 8192
//                        cells (sum i64, count u32: 96 KiB of static LDS, one block per CU), then a flush of the touched
//                        cells into the zeroed (map, slot) patch with integer device atomics.  The point count is the
//                        device word.
//   k_wall_align_values  the patch becomes the int32 image f, the map rows [j_f - P - A, j_f + P + A) the int32 image m;
//                        an unusable cell, and a row outside the map, is kWallAlignNone.  Behind the wait on the adds.
//   k_wall_align_score   the hot kernel: one block per (station shift a, run of `rows` patch rows).  It stages the run of
//                        f and the matching rows of m in LDS (64 KiB hold both whole images), a thread owns (k, b) pairs
//                        (and, when there are fewer pairs than threads, a share of the rows), so the sector wrap is an LDS
//                        index and never a global gather.  Partials: LDS integer atomics per b, then one integer device
//                        atomic per field, b and block into the zeroed table.  Integer sums: the table does not depend on
//                        `rows`, the grid or the order blocks run in.
// No floating-point atomics, no ticket, no host round trip.  Every patch index is jr * n_sectors + k with 0 <= jr < 2P,
// k < n_sectors; every m index is below (2P + 2A) n_sectors; every table index below (2A + 1)(2B + 1).
#include <string.h>

#include "gm_wall_align.hpp"   // the bin kernels' shape and run merge, the halves of the values kernels

namespace gm {

constexpr uint32_t kAlignMaxB = 2 * GM_WALL_ALIGN_MAX_SHIFT + 1;

static_assert(sizeof(gm_wall_align_score) == 24, "the 24-byte score record");

__global__ __launch_bounds__(kAlignBinThreads) void k_wall_align_bin(WallAlignArgs a)
{
    __shared__ unsigned long long s_sum[kAlignCells];
    __shared__ uint32_t s_cnt[kAlignCells];
    const WallArgs &w = a.w;
    const uint32_t n = w.n_ptr ? *w.n_ptr : w.n_host;
    const uint32_t nsec = w.n_sectors;
    const uint32_t pcells = 2u * a.P * nsec;   // <= kAlignCells (the host checks the parameters)
    const float p_lo = -(float)a.P, p_hi = (float)a.P;

    for (uint32_t c = threadIdx.x; c < pcells; c += kAlignBinThreads) { s_sum[c] = 0ull; s_cnt[c] = 0u; }
    __syncthreads();

    uint32_t cls[4] = {0u, 0u, 0u, 0u};   // plane, beyond_gate, outside_patch, binned: wall_chain's order
    stream_points<kAlignBinThreads, kAlignBinUnroll>(w.pts, w.labels, n, [&](uint64_t i, bool in, const float4 &q, uint32_t lab) {
        float e = __builtin_nanf("");
        int cell = -1;      // jr * n_sectors + k (< 8192)
        float jl;
        uint32_t kk;
        if (in && wall_chain(q, lab, w, WallArcArg<false>(), [&](float s) { return s >= p_lo && s < p_hi; },
                             [&](uint32_t k) { ++cls[k]; }, e, jl, kk))
            cell = (int)((uint32_t)((int32_t)jl + (int32_t)a.P) * nsec + kk);
        if (in && w.res) w.res[i] = e;
        if (in && w.cell) w.cell[i] = cell;
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
    // class counts: one atomic per class and block
    block_class_counts<kAlignBinThreads>(cls, [&](uint32_t k, unsigned long long v) {
        if (v) atomicAdd(&a.ctr[k], v);
    });
    if (blockIdx.x == 0 && threadIdx.x == 4) a.ctr[4] = n;
}

__global__ __launch_bounds__(kAlignThreads) void k_wall_align_values(WallAlignArgs a)
{
    const WallArgs &w = a.w;
    const uint32_t nsec = w.n_sectors;
    const uint32_t pcells = 2u * a.P * nsec;
    const uint32_t mcells = (2u * a.P + 2u * a.A) * nsec;
    const int64_t j0 = w.anchor - (int64_t)a.P - (int64_t)a.A;   // (|anchor| < 4e18: no overflow)
    const int64_t nst = (int64_t)w.n_stations;
    uint32_t usable = 0u;
    for (uint32_t i = blockIdx.x * kAlignThreads + threadIdx.x; i < pcells + mcells; i += gridDim.x * kAlignThreads) {
        if (i < pcells) {
            usable += align_patch_value(a.p_cnt, a.p_sum, a.min_frame_count, a.f, i);
        } else {
            const uint32_t c = i - pcells;
            const int64_t j = j0 + (int64_t)(c / nsec);
            int32_t v = kWallAlignNone;
            if (j >= 0 && j < nst) v = align_map_value(w.table, (uint64_t)j * nsec + c % nsec, a.min_count);   // g < n_stations * n_sectors
            a.m[c] = v;
        }
    }
    align_patch_usable(usable, &a.ctr[5]);
}

__global__ __launch_bounds__(kAlignThreads) void k_wall_align_score(WallAlignArgs a)
{
    __shared__ int32_t s_f[kAlignCells];
    __shared__ int32_t s_m[kAlignCells];
    __shared__ unsigned long long s_ssd[kAlignMaxB], s_sd[kAlignMaxB];
    __shared__ uint32_t s_n[kAlignMaxB];
    const uint32_t nsec = a.w.n_sectors;
    const uint32_t nb = 2u * a.B + 1u, rows2p = 2u * a.P;
    const uint32_t chunks = (rows2p + a.rows - 1u) / a.rows;
    const uint32_t ia = blockIdx.x / chunks;                  // a + A, 0 .. 2A
    const uint32_t r0 = (blockIdx.x - ia * chunks) * a.rows;  // the run's first patch row
    const uint32_t nr = rows2p - r0 < a.rows ? rows2p - r0 : a.rows;
    const uint32_t cells = nr * nsec;                         // <= kAlignCells
    const int32_t *gf = a.f + (size_t)r0 * nsec;
    const int32_t *gm = a.m + (size_t)(r0 + ia) * nsec;       // patch row jr at shift a: the image's row jr + a + A
    for (uint32_t i = threadIdx.x; i < cells; i += kAlignThreads) { s_f[i] = gf[i]; s_m[i] = gm[i]; }
    for (uint32_t i = threadIdx.x; i < nb; i += kAlignThreads) { s_ssd[i] = 0ull; s_sd[i] = 0ull; s_n[i] = 0u; }
    __syncthreads();

    const uint32_t pairs = nsec * nb;
    const uint32_t share = pairs < (uint32_t)kAlignThreads ? kAlignThreads / pairs : 1u;   // threads per pair
    const long long C = a.C;
    for (uint32_t item = threadIdx.x; item < pairs * share; item += kAlignThreads) {
        const uint32_t rl = item / pairs, p = item - rl * pairs;
        const uint32_t bi = p / nsec, k = p - bi * nsec;      // b + B, the patch sector
        int32_t kk = (int32_t)k + (int32_t)bi - (int32_t)a.B; // (k + b) mod n_sectors: |b| < n_sectors
        if (kk < 0) kk += (int32_t)nsec;
        else if (kk >= (int32_t)nsec) kk -= (int32_t)nsec;
        unsigned long long ssd = 0ull;
        long long sd = 0;
        uint32_t cnt = 0u;
        for (uint32_t r = rl; r < nr; r += share) {
            const int32_t fv = s_f[r * nsec + k], mv = s_m[r * nsec + (uint32_t)kk];
            if (fv == kWallAlignNone || mv == kWallAlignNone) continue;
            long long d = (long long)fv - (long long)mv;
            d = d > C ? C : (d < -C ? -C : d);
            ssd += (unsigned long long)(d * d);
            sd += d;
            ++cnt;
        }
        if (cnt) {
            atomicAdd(&s_ssd[bi], ssd);
            atomicAdd(&s_sd[bi], (unsigned long long)sd);
            atomicAdd(&s_n[bi], cnt);
        }
    }
    __syncthreads();
    for (uint32_t bi = threadIdx.x; bi < nb; bi += kAlignThreads) {
        const uint32_t cnt = s_n[bi];
        if (!cnt) continue;
        gm_wall_align_score *rec = a.table + (size_t)ia * nb + bi;
        atomicAdd(reinterpret_cast<unsigned long long *>(&rec->ssd), s_ssd[bi]);
        atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum_d), s_sd[bi]);
        atomicAdd(&rec->n, cnt);
    }
}

uint32_t wall_align_default_rows(uint32_t n_sectors)
{
    const uint32_t r = 512u / (n_sectors ? n_sectors : 1u);
    return r < 8u ? 8u : r;
}

void launch_wall_align_bin(const WallAlignArgs &a, uint32_t n_cap, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_align_bin, dim3(wall_blocks(n_cap, 0u)), dim3(kAlignBinThreads), 0, s, a);
}

void launch_wall_align_values(const WallAlignArgs &a, hipStream_t s)
{
    const uint32_t cells = (4u * a.P + 2u * a.A) * a.w.n_sectors;
    hipLaunchKernelGGL(k_wall_align_values, dim3((cells + kAlignThreads - 1) / kAlignThreads), dim3(kAlignThreads), 0, s, a);
}

void launch_wall_align_score(const WallAlignArgs &a, hipStream_t s)
{
    const uint32_t chunks = (2u * a.P + a.rows - 1u) / a.rows;
    hipLaunchKernelGGL(k_wall_align_score, dim3((2u * a.A + 1u) * chunks), dim3(kAlignThreads), 0, s, a);
}

}  // namespace gm
