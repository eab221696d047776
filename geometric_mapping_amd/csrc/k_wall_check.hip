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

#include "gm_wall_check.hpp"   // the payload, the cell rule, the row, the peaks: shared with k_wall_check_joint.hip

namespace gm {

// the predicate's body: the adds' chain head (wall_chain, gm_device.hpp), straight or on the by-value arc or clothoid block
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
        cls = wall_check_cell(w.table, cell, a.reference, a.min_count, a.T, e, delta);
    }
    if (w.res) w.res[i] = e;
    if (w.cell) w.cell[i] = cell;
    if (a.delta) a.delta[i] = wall_check_delta32(delta);
    if (a.cls) a.cls[i] = (uint8_t)cls;
    p.e = e;
    p.cell = cell;
    p.delta = delta;
    wall_check_count<GM_WALL_CHECK_N_CLS>(cls, 0u);
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
        wall_check_prepare<GM_WALL_CHECK_N_CLS>();
        q_pos = 0; q_neg = 0;
    }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCheckPred::Payload &p)
    {
        wall_check_row(a.out, a.row_is_index, src, dst, p, q_pos, q_neg);
    }
    __device__ __forceinline__ void finish(uint32_t) { wall_check_finish<GM_WALL_CHECK_N_CLS>(a.ctr, a.ctr + GM_WALL_CHECK_N_CLS, q_pos, q_neg); }
};

template <class Pred>
static void wall_check_launch(const Pred &pred, const WallCheckArgs &a, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    WallCheckEmit emit;
    memset(&emit, 0, sizeof(emit));
    emit.a = a;
    hipLaunchKernelGGL((k_compact<Pred, WallCheckEmit>), dim3(compact_grid(n_cap ? n_cap : 1u)), dim3(kCpThreads), 0, s, pred, emit,
                       a.w.n_ptr, a.w.n_host, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

// the check's one front: the predicate of the axis' kind
void launch_wall_check(const WallCheckArgs &a, const WallAxis &axis, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    if (axis.kind == kAxisStraight) wall_check_launch(WallCheckPred{a}, a, n_cap, st, s);
    else if (axis.kind == kAxisArc) wall_check_launch(WallCheckPredArc{a, {axis.ax.arc}}, a, n_cap, st, s);
    else wall_check_launch(WallCheckPredClothoid{a, {axis.ax}}, a, n_cap, st, s);
}

}  // namespace gm
