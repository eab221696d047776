// k_wall_check.hip -- BUILD-DEFINED EXTENSION: a frame's changed points against the persistent wall map
// (gm_wall_map_check_*), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_check_np.py.  ONE launch per check:
// k_compact<WallCheckPred, WallCheckEmit> (gm_compact.hpp) over the valid cloud.
//   predicate   16 B of point + 1 B of label read, k_wall_add's chain head (wall_chain, gm_device.hpp) under the check's own gate,
//               then for a mapped point one gather of the cell's accumulators (count first; 8 B of sum or the two keys only
//               for a usable cell) from a table that is hot in L2, and the integer rule (wall_check_rule, shared with the
//               host's gm_wall_check_classify).  A point survives iff it is changed.  The point, e, the cell and delta stay
//               in registers as the payload (8 words per item).  Classes are counted by wave ballots into seven LDS words.
//   emit        the 32-byte row at the survivor's rank in the staging buffer (two 16-byte stores): rows leave in the valid
//               cloud's order from one launch.  Each thread keeps the integer maxima of its own rows; finish() reduces
//               them over the wave and the block.
//   finish      one integer atomic per class and block, one atomicMax per peak and block.
// Nothing is written per point (the stage call's optional outputs apart), nothing to the map.  Every gather index is a
// mapped cell j * n_sectors + k with 0 <= j < n_stations and k < n_sectors; every store index is a rank < n or a point
// index < n.  No floating-point atomics, no LDS table to zero or flush.
#include <string.h>

#include "gm_compact.hpp"
#include "gm_internal.hpp"

namespace gm {

static_assert(sizeof(gm_wall_check_point) == 32, "a 32-byte PointCloud2 row");

// block-shared: the seven class counts, then the two peaks (magnitudes)
__device__ __forceinline__ uint32_t *wk_class_counts()
{
    __shared__ uint32_t c[GM_WALL_CHECK_N_CLS];
    return c;
}
__device__ __forceinline__ unsigned long long *wk_peaks()
{
    __shared__ unsigned long long p[2];
    return p;
}

// the predicate's body: the adds' chain head (wall_chain, gm_device.hpp), straight or on the by-value arc or clothoid block
struct WallCheckPayload { float4 q; long long delta; float e; int cell; };
static_assert(GM_WALL_CHECK_CLS_PLANE == kChainPlane && GM_WALL_CHECK_CLS_BEYOND_GATE == kChainBeyondGate &&
                  GM_WALL_CHECK_CLS_OUTSIDE == kChainOutside, "the check's first classes are wall_chain's");
template <class Axis>
__device__ __forceinline__ bool wall_check_point(const WallCheckArgs &a, const Axis &arc, uint32_t i, WallCheckPayload &p)
{
    const WallArgs &w = a.w;
    p.q = w.pts[i];
    const uint32_t lab = w.labels ? w.labels[i] : 0u;
    if (i == 0u) a.ctr[10] = w.n_ptr ? *w.n_ptr : w.n_host;   // n_points (>= 1 here; the caller's zero stands for 0)
    float e = __builtin_nanf("");
    int cell = -1;
    long long delta = 0;
    uint32_t cls, kk;
    int64_t j;
    float jl;
    if (wall_chain(p.q, lab, w, arc, [&](float s) { return (j = wall_station(w, s)) >= 0; }, [&](uint32_t k) { cls = k; }, e, jl,
                   kk)) {
        cell = (int)((uint32_t)j * w.n_sectors + kk);   // < n_stations * n_sectors <= 2^24
        const uint32_t cn = w.table.cnt[cell];
        long long sum = 0;
        uint32_t lo = 0u, hi = 0u;
        if (cn >= a.min_count) {
            if (a.reference == GM_WALL_CHECK_ENVELOPE) { lo = w.table.lo[cell]; hi = w.table.hi[cell]; }
            else sum = (long long)w.table.sum[cell];
        }
        cls = wall_check_rule(a.reference, a.min_count, a.T, sum, cn, lo, hi, e, delta);
    }
    if (w.res) w.res[i] = e;
    if (w.cell) w.cell[i] = cell;
    if (a.delta) a.delta[i] = delta > 2147483647ll ? 2147483647 : (delta < -2147483648ll ? (int32_t)(-2147483647 - 1) : (int32_t)delta);
    if (a.cls) a.cls[i] = (uint8_t)cls;
    p.e = e;
    p.cell = cell;
    p.delta = delta;
    // (the lanes past the end of the input are not here: the ballots see the active lanes only)
    const int lane = lane_id();
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)GM_WALL_CHECK_N_CLS; ++k) {
        const unsigned long long m = __ballot(cls == k);
        if (m && lane == (int)__builtin_ctzll(m)) atomicAdd(&wk_class_counts()[k], (uint32_t)__popcll(m));
    }
    return cls >= (uint32_t)GM_WALL_CHECK_CLS_CHANGED_POS;
}

struct WallCheckPred {
    WallCheckArgs a;
    using Payload = WallCheckPayload;
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const { return wall_check_point(a, WallArcArg<false>(), i, p); }
};
struct WallCheckPredArc {
    WallCheckArgs a;
    WallArcArg<true> arc;
    using Payload = WallCheckPayload;
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const { return wall_check_point(a, arc, i, p); }
};

struct WallCheckPredClothoid {
    WallCheckArgs a;
    WallClothoidArg cl;
    using Payload = WallCheckPayload;
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const { return wall_check_point(a, cl, i, p); }
};

struct WallCheckEmit {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallCheckArgs a;
    long long q_pos, q_neg;           // this thread's largest / smallest emitted delta
    __device__ __forceinline__ void prepare()
    {
        if (threadIdx.x < (uint32_t)GM_WALL_CHECK_N_CLS) wk_class_counts()[threadIdx.x] = 0u;
        if (threadIdx.x < 2u) wk_peaks()[threadIdx.x] = 0ull;
        q_pos = 0; q_neg = 0;
    }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCheckPred::Payload &p)
    {
        float4 *o = reinterpret_cast<float4 *>(a.out + dst);
        o[0] = make_float4(p.q.x, p.q.y, p.q.z, __fmul_rn((float)p.delta, 0x1p-20f));
        o[1] = make_float4(p.e, __int_as_float(p.cell), __uint_as_float(src), a.row_is_index ? __uint_as_float(src) : p.q.w);
        if (p.delta > q_pos) q_pos = p.delta;
        if (p.delta < q_neg) q_neg = p.delta;
    }
    __device__ __forceinline__ void finish(uint32_t)
    {
        // every thread of the block is here: full waves
        unsigned long long hp = (unsigned long long)q_pos, hn = (unsigned long long)(-q_neg);
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const unsigned long long op = __shfl_xor(hp, o, kWave), on = __shfl_xor(hn, o, kWave);
            hp = hp > op ? hp : op;
            hn = hn > on ? hn : on;
        }
        if (lane_id() == 0) {
            if (hp) atomicMax(&wk_peaks()[0], hp);
            if (hn) atomicMax(&wk_peaks()[1], hn);
        }
        __syncthreads();
        if (threadIdx.x < (uint32_t)GM_WALL_CHECK_N_CLS) {
            const uint32_t c = wk_class_counts()[threadIdx.x];
            if (c) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)c);
        } else if (threadIdx.x < (uint32_t)GM_WALL_CHECK_N_CLS + 2u) {
            const unsigned long long v = wk_peaks()[threadIdx.x - GM_WALL_CHECK_N_CLS];
            if (v) atomicMax(&a.ctr[threadIdx.x], v);
        }
    }
};

void launch_wall_check(const WallCheckArgs &a, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    WallCheckPred pred{a};
    WallCheckEmit emit;
    memset(&emit, 0, sizeof(emit));
    emit.a = a;
    hipLaunchKernelGGL((k_compact<WallCheckPred, WallCheckEmit>), dim3(compact_grid(n_cap ? n_cap : 1u)), dim3(kCpThreads), 0, s, pred,
                       emit, a.w.n_ptr, a.w.n_host, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

void launch_wall_check_arc(const WallCheckArgs &a, const WallArc &arc, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    WallCheckPredArc pred{a, {arc}};
    WallCheckEmit emit;
    memset(&emit, 0, sizeof(emit));
    emit.a = a;
    hipLaunchKernelGGL((k_compact<WallCheckPredArc, WallCheckEmit>), dim3(compact_grid(n_cap ? n_cap : 1u)), dim3(kCpThreads), 0, s,
                       pred, emit, a.w.n_ptr, a.w.n_host, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

void launch_wall_check_clothoid(const WallCheckArgs &a, const WallClothoid &cl, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    WallCheckPredClothoid pred{a, {cl}};
    WallCheckEmit emit;
    memset(&emit, 0, sizeof(emit));
    emit.a = a;
    hipLaunchKernelGGL((k_compact<WallCheckPredClothoid, WallCheckEmit>), dim3(compact_grid(n_cap ? n_cap : 1u)), dim3(kCpThreads), 0,
                       s, pred, emit, a.w.n_ptr, a.w.n_host, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

}  // namespace gm
