// gm_gridcc.hpp -- connected components on a grid whose column index wraps, in a fixed number of launches: the labelling
// core shared by k_wall_regions.hip (cells of a station window) and k_wall_objects.hip (blocks of a window, two planes in
// one index space).  Device-only but for cc_blocks.  The __global__ kernels stay in their files: they load and classify,
// call the step here, and count.
//
// The union-find.  A parent only ever decreases and stays inside its component, so the root of a finished forest is the
// component's smallest index: the label.  kCcNone marks an element that is not flagged.
//   tiles    cc_label_tile: one workgroup labels its tile in LDS (cc_lds_find / cc_lds_union) and writes one parent per
//            flagged element, the global index of its tile root.
//   seams    cc_seam: one thread per border element joins it to its neighbours across the tile edge, and across the seam
//            where the last column meets column 0.  Lock-free: find both roots, atomicMin the larger root's parent to the
//            smaller, retry on a lost race (cc_find / cc_union).  Workgroups of this launch read parents other workgroups
//            are changing, so EVERY access to the parent array in it is an agent-scope atomic: a plain load may be served
//            stale from L1 or another XCD's L2.  Nothing else of the launch is read while it is written.
//   flatten  cc_flatten: every flagged element finds its root and stores it; roots take a slot from a counter, one atomic
//            per wave.  Other threads store roots meanwhile, hence atomics again; launch boundaries order the rest.
// The segmented reduction of the *_reduce kernels starts from wave_runs (gm_device.hpp).
#pragma once
#include "gm_internal.hpp"

namespace gm {

constexpr int kCcThreads = 256;
constexpr uint32_t kCcMaxBlocks = 8192;
constexpr uint32_t kCcNone = 0xFFFFFFFFu;   // parent of an element that is not flagged

// the grid of a grid-stride launch over n elements
inline uint32_t cc_blocks(uint64_t n)
{
    const uint64_t b = (n + kCcThreads - 1) / kCcThreads;
    return (uint32_t)(b < 1 ? 1 : (b > kCcMaxBlocks ? kCcMaxBlocks : b));
}

// ---- union-find ----

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t cc_lds_find(uint32_t *L, uint32_t x)
{
    for (;;) {
        const uint32_t y = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (y == x) return x;
        x = y;
    }
}
__device__ __forceinline__ void cc_lds_union(uint32_t *L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cc_lds_find(L, a);
        b = cc_lds_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&L[a], b);   // a was a root when read; old != a: another wave linked it meanwhile
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ uint32_t cc_find(uint32_t *p, uint32_t x)
{
    for (;;) {
        const uint32_t y = cc_load(&p[x]);
        if (y == x) return x;
        const uint32_t z = cc_load(&p[y]);
        if (z == y) return y;
        atomicMin(&p[x], z);   // path halving: z is an ancestor of x, below its parent
        x = z;
    }
}
__device__ __forceinline__ void cc_union(uint32_t *p, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cc_find(p, a);
        b = cc_find(p, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&p[a], b);
        if (old == a) return;
        a = old;   // a lost its root to another thread: what it pointed to still has to meet b
    }
}

// ---- tiles ----

// The workgroup's tile of `cells` = rows x tk elements, row-major: the caller has stored S[l] (0: not flagged; neighbours
// are joined when their S are equal) and L[l] = l.  Left, up and, for 8-connectivity, the two upper diagonals; no wrap
// inside a tile.  Writes parent[at(row, col)] = at(the tile root's row, col) for the flagged elements; `at` maps
// tile-local to global and is row-major too, so the smallest local index of a component is its smallest global one.
// L and S may be rewritten after one more barrier.
template <class T, class At>
__device__ __forceinline__ void cc_label_tile(uint32_t *L, const T *S, uint32_t cells, uint32_t tk, bool conn8, uint32_t *parent, At at)
{
    __syncthreads();
    for (uint32_t l = threadIdx.x; l < cells; l += kCcThreads) {
        const T s = S[l];
        if (!s) continue;
        const uint32_t jl = l / tk, kl = l % tk;
        if (kl > 0 && S[l - 1] == s) cc_lds_union(L, l, l - 1);
        if (jl > 0) {
            if (S[l - tk] == s) cc_lds_union(L, l, l - tk);
            if (conn8) {
                if (kl > 0 && S[l - tk - 1] == s) cc_lds_union(L, l, l - tk - 1);
                if (kl + 1 < tk && S[l - tk + 1] == s) cc_lds_union(L, l, l - tk + 1);
            }
        }
    }
    __syncthreads();
    for (uint32_t l = threadIdx.x; l < cells; l += kCcThreads) {
        if (!S[l]) continue;
        const uint32_t r = cc_lds_find(L, l);
        parent[at(l / tk, l % tk)] = at(r / tk, r % tk);
    }
}

// ---- seams ----

// border elements of one plane of n rows x nk columns cut into tiles of ts x tk: one per row and tile column (its last
// column against the next, the seam for the last), then one per column and tile row but the last (against the next row)
__host__ __device__ inline uint64_t cc_seam_count(uint32_t n, uint32_t nk, uint32_t tiles_s, uint32_t tiles_k)
{
    return (uint64_t)tiles_k * n + (uint64_t)(tiles_s - 1u) * nk;
}
// both flagged and not the same element (a ring of one column meets itself at the seam)
__device__ __forceinline__ bool cc_joinable(const uint32_t *parent, uint32_t x, uint32_t y)
{
    return x != y && cc_load(&parent[x]) != kCcNone && cc_load(&parent[y]) != kCcNone;
}
// Border element i < cc_seam_count of the plane at index `base`: join(x, y) for every pair across the edge, with the
// diagonal pairs for 8-connectivity.  join tests the pair (cc_joinable, and whatever else it must share) and calls cc_union.
template <class Join>
__device__ __forceinline__ void cc_seam(uint64_t i, uint32_t n, uint32_t nk, uint32_t ts, uint32_t tk, uint32_t tiles_k, bool conn8,
                                        uint32_t base, Join join)
{
    const uint64_t n_vert = (uint64_t)tiles_k * n;
    if (i < n_vert) {   // the last column of tile column b against the next column, the seam for the last
        const uint32_t b = (uint32_t)(i % tiles_k), j = (uint32_t)(i / tiles_k);
        const uint32_t end = (b + 1u) * tk, k = (end < nk ? end : nk) - 1u, k2 = k + 1u < nk ? k + 1u : 0u;
        const uint32_t x = base + j * nk + k;
        join(x, base + j * nk + k2);
        if (conn8) {
            if (j > 0u) join(x, base + (j - 1u) * nk + k2);
            if (j + 1u < n) join(x, base + (j + 1u) * nk + k2);
        }
    } else {            // the last row of tile row b against the next row
        const uint64_t h = i - n_vert;
        const uint32_t b = (uint32_t)(h / nk), k = (uint32_t)(h % nk), j = (b + 1u) * ts - 1u;   // j + 1 < n
        const uint32_t x = base + j * nk + k, y = base + (j + 1u) * nk;
        join(x, y + k);
        if (conn8) {
            join(x, y + (k + 1u < nk ? k + 1u : 0u));
            join(x, y + (k > 0u ? k - 1u : nk - 1u));
        }
    }
}

// ---- flatten ----

// the whole kernel body: a grid-stride loop over parent[0 .. total) in wave-uniform trips (the slot ranks come from a ballot)
__device__ __forceinline__ void cc_flatten(uint32_t *parent, uint32_t *slot, uint64_t total, unsigned long long *counter)
{
    const int lane = lane_id();
    for (uint64_t w0 = (uint64_t)blockIdx.x * kCcThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < total;
         w0 += (uint64_t)gridDim.x * kCcThreads) {
        const uint64_t w = w0 + lane;
        bool root = false;
        if (w < total) {
            uint32_t x = cc_load(&parent[w]);
            if (x != kCcNone) {
                // (every value ever stored is an ancestor, so the walk still ends at the root)
                for (;;) {
                    const uint32_t y = cc_load(&parent[x]);
                    if (y == x) break;
                    x = y;
                }
                root = x == (uint32_t)w;
                if (!root) __hip_atomic_store(&parent[w], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const unsigned long long m = __ballot(root);
        if (m) {
            unsigned long long base = 0ull;
            if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(counter, (unsigned long long)__popcll(m));
            base = __shfl(base, (int)__builtin_ctzll(m), kWave);
            if (root) slot[w] = (uint32_t)base + (uint32_t)__popcll(m & lanemask_lt());
        }
    }
}

}  // namespace gm
