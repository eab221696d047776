// k_wall_mesh.hip -- BUILD-DEFINED EXTENSION: the persistent wall map as an indexed triangle mesh (gm_wall_map_mesh), the
// device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_mesh_np.py.  The host (gm_wall.hip)
// walks the window twice:
//   1. vertices: per chunk of whole block rows the cloud's merge and then k_compact<WallCloudPred, WallMeshVertexEmit>.
//      The emit step is the cloud's (gm_wall_cloud_emit.hpp: the same record at the same rank) and stores the survivor's
//      index in the vertex list -- the ranks of the chunks before plus its own -- into a table of one u32 per block of
//      the WINDOW, which the host filled with kWallMeshDead; for a step cut the record's mean goes into a second table
//      beside it.  gm_wall_map_cloud's own instantiation (k_wall_cloud.hip) knows nothing of either.
//   2. triangles: per chunk of whole quad rows k_compact<WallMeshPred, WallMeshEmit> over the chunk's 2 * quads slots.  A
//      lane's slot is (quad, which of its two triangles): lanes take consecutive slots, so a wave covers 32 consecutive
//      quads of a row and each of the four rank loads (and of the three mean loads) of a wave is one contiguous run of
//      the table -- two when the row ends inside the wave, plus the wrapped column.  The table was written by the launches
//      before on the same stream and is read-only here; a quad row's two block rows may come from different vertex chunks.
//      The predicate applies the corner rule and the step cut and keeps the three indices as its payload; the emit step
//      writes the 12-byte record at the slot's rank.  The four class counts are counted per block in LDS (ballots, one
//      LDS atomic per wave and class) and added once per class and block, as WallCloudEmit::finish does.
#include "gm_compact.hpp"
#include "gm_internal.hpp"
#include "gm_wall_cloud_emit.hpp"

namespace gm {

static_assert(sizeof(gm_wall_mesh_triangle) == 12, "three indices");

// ---- 1. vertices ----

// (CloudEmit: WallCloudEmit, or WallCloudEmitArc / WallCloudEmitClothoid on a curved axis; the straight one is not a template
// specialisation, so that its kernel keeps its name)
template <class CloudEmit>
struct WallMeshVertexEmitT {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    CloudEmit cloud;
    uint32_t *rank;        // [NJ * NK] of the window
    float *mean;           // [NJ * NK] or nullptr
    uint32_t rank_base;    // the vertices of the chunks before this one
    __device__ __forceinline__ void prepare() const { cloud.prepare(); }
    __device__ __forceinline__ void finish(uint32_t tile) const { cloud.finish(tile); }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCloudPred::Payload &p) const
    {
        cloud(src, dst, p);
        const uint32_t block = cloud.a.J0 * cloud.a.NK + src;   // of the window: the record's block field
        rank[block] = rank_base + dst;
        if (mean) mean[block] = cloud.a.out[dst].mean;          // (the value this thread has just stored)
    }
};

struct WallMeshVertexEmit : WallMeshVertexEmitT<WallCloudEmit> {};
struct WallMeshVertexEmitArc : WallMeshVertexEmitT<WallCloudEmitArc> {};
struct WallMeshVertexEmitClothoid : WallMeshVertexEmitT<WallCloudEmitClothoid> {};

// ---- 2. triangles ----

// the block's counts of quads_two, quads_one, quads_none, cut_by_step
__device__ __forceinline__ uint32_t *wm_class_counts()
{
    __shared__ uint32_t c[4];
    return c;
}

__device__ __forceinline__ void wm_count(bool mine, int which)
{
    const unsigned long long m = __ballot(mine);
    if (m && lane_id() == (int)__builtin_ctzll(m)) atomicAdd(&wm_class_counts()[which], (uint32_t)__popcll(m));
}

struct WallMeshPred {
    WallMeshArgs a;
    struct Payload { uint32_t v[3]; };
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const
    {
        const uint32_t Q = a.Q0 + (i >> 1), second = i & 1u;
        const uint32_t J = Q / a.NKq, K = Q - J * a.NKq;
        const uint32_t K1 = K + 1u == a.NK ? 0u : K + 1u;         // (K + 1 = NK only when the sectors wrap)
        // corner c of A, B, C, D is block b[c]; J + 1 <= NJ - 1
        const uint32_t b[4] = {J * a.NK + K, (J + 1u) * a.NK + K, (J + 1u) * a.NK + K1, J * a.NK + K1};
        uint32_t r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = a.rank[b[c]];
        uint32_t alive = 0u, dead = 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (r[c] != kWallMeshDead) ++alive;
            else dead = (uint32_t)c;
        }
        // The corner rule.  Every triangle is the cyclic order A, B, C, D with one corner left out: (A, B, C) leaves out D,
        // (A, C, D) leaves out B, a quad of three alive corners leaves out the dead one.
        const bool tri = alive == 4u || (alive == 3u && !second);
        const uint32_t drop = alive == 4u ? (second ? 1u : 3u) : dead;
        const bool d0 = drop == 0u, d01 = drop <= 1u, d3 = drop == 3u;
        p.v[0] = d0 ? r[1] : r[0];
        p.v[1] = d01 ? r[2] : r[1];
        p.v[2] = d3 ? r[2] : r[3];
        // (the lanes past the end of the input are not here: the ballots see the active lanes only)
        wm_count(!second && alive == 4u, 0);
        wm_count(!second && alive == 3u, 1);
        wm_count(!second && alive < 3u, 2);
        bool cut = false;
        if (tri && a.mean) {   // (its corners are alive: their means were written)
            const float m0 = a.mean[d0 ? b[1] : b[0]], m1 = a.mean[d01 ? b[2] : b[1]], m2 = a.mean[d3 ? b[2] : b[3]];
            cut = fabsf(__fsub_rn(m0, m1)) > a.max_step || fabsf(__fsub_rn(m1, m2)) > a.max_step ||
                  fabsf(__fsub_rn(m0, m2)) > a.max_step;
        }
        wm_count(tri && cut, 3);
        return tri && !cut;
    }
};

struct WallMeshEmit {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallMeshArgs a;
    __device__ __forceinline__ void prepare() const
    {
        if (threadIdx.x < 4) wm_class_counts()[threadIdx.x] = 0u;
    }
    __device__ __forceinline__ void finish(uint32_t) const
    {
        __syncthreads();
        if (threadIdx.x < 4) {
            const uint32_t c = wm_class_counts()[threadIdx.x];
            if (c) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)c);
        }
    }
    __device__ __forceinline__ void operator()(uint32_t, uint32_t dst, const WallMeshPred::Payload &p) const
    {
        gm_wall_mesh_triangle t;
        t.v[0] = p.v[0];
        t.v[1] = a.outward ? p.v[2] : p.v[1];
        t.v[2] = a.outward ? p.v[1] : p.v[2];
        a.out[dst] = t;
    }
};

// the vertex pass's one front: the cloud's emit step of the axis' kind, wrapped
void launch_wall_mesh_vertices(const WallCloudArgs &a, const WallCloudAxis &axis, uint32_t *rank, float *mean, uint32_t rank_base,
                               const ScanState &st, hipStream_t s)
{
    if (axis.kind == kAxisStraight) {
        wall_cloud_launch(a, WallMeshVertexEmit{{WallCloudEmit{a}, rank, mean, rank_base}}, st, s);
    } else if (axis.kind == kAxisArc) {
        wall_cloud_launch(a, WallMeshVertexEmitArc{{WallCloudEmitArc{a, WallCloudOnArc{axis.arc}}, rank, mean, rank_base}}, st, s);
    } else {
        const WallCloudEmitClothoid cloud{a, WallCloudOnClothoid{wall_cloud_clothoid(axis)}};
        wall_cloud_launch(a, WallMeshVertexEmitClothoid{{cloud, rank, mean, rank_base}}, st, s);
    }
}

void launch_wall_mesh_triangles(const WallMeshArgs &a, const ScanState &st, hipStream_t s)
{
    const uint32_t slots = 2u * a.nq;   // >= 2, <= 2^21: the quads of a chunk are at most the blocks of a vertex chunk
    WallMeshPred pred{a};
    WallMeshEmit emit{a};
    hipLaunchKernelGGL((k_compact<WallMeshPred, WallMeshEmit>), dim3(compact_grid(slots)), dim3(kCpThreads), 0, s, pred, emit,
                       (const uint32_t *)nullptr, slots, st, reinterpret_cast<uint32_t *>(a.ctr + 4), (uint32_t *)nullptr);
}

}  // namespace gm
