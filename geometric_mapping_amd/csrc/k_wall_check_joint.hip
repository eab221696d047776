// k_wall_check_joint.hip -- BUILD-DEFINED EXTENSION: the check of a frame that straddles joints of a wall alignment
// (gm_wall_alignment_check_*; include/gm_hip.h states the rule), the device side.
//
// k_wall_check's shape (gm_wall_check.hpp: ONE k_compact launch over the valid cloud, the payload in registers, rows out in
// the cloud's order, integer atomics only), over up to GM_WALL_JOINT_MAX_SIDES element maps at once:
//   1. every point is given its owner by joint_owner (gm_wall_joint.hpp states the rule).  The planes are read from LDS
//      (the emit step's prepare() stores them ahead of the block's barrier), as in k_wall_add_joint and
//      k_wall_locate_joint;
//   2. the point runs its owner's chain and no other: a loop over the sides, wave-uniform, each trip joint_side_chain
//      (gm_wall_joint.hpp: wall_chain exactly as k_wall_check, k_wall_check_arc and k_wall_check_clothoid instantiate it)
//      under the check's gate.  A wave whose lanes have different owners runs each of their chains once, under the lanes'
//      mask; the side's frame stays in scalar registers;
//   3. inside the same trip of the loop a mapped point gathers its cell from the OWNER's table (wall_check_cell: the count
//      first, sum or keys only for a usable cell) and takes the integer rule, and the wave counts its seven classes: one
//      ballot per class over the lanes the side owns, into the side's seven LDS words.  A wave of one owner -- nearly every
//      wave of a frame in frame order -- so pays k_wall_check's seven ballots, not 7 x n_sides, and no register holds a count;
//   4. the payload's cell is side << 24 | cell (a cell is < 2^24); the row, the peaks and the closing atomics are
//      gm_wall_check.hpp's, over 7 x GM_WALL_JOINT_MAX_SIDES class words.
// Nothing is written per point (the stage call's optional outputs apart), nothing to a map.  Every gather index is a mapped
// cell of the owner's map: j * n_sectors + k with 0 <= j < the owner's n_stations and k < n_sectors; every store index is
// a rank < n or a point index < n; owner < n_sides <= GM_WALL_JOINT_MAX_SIDES.
#include <string.h>

#include "gm_wall_check.hpp"
#include "gm_wall_joint.hpp"   // the side, the owner rule, the side's chain

namespace gm {

constexpr int kCheckJointSides = GM_WALL_JOINT_MAX_SIDES;
constexpr int kCheckJointWords = kCheckJointSides * GM_WALL_CHECK_N_CLS;

// The stage call's per-point outputs (each may be nullptr).  The predicate reads them from LDS, behind the one scalar
// word that says whether there is any: ten scalar registers less in the frame path, which keeps the kernel free of scalar
// spills; the stage call pays five broadcast reads per point.
struct WallCheckJointOut {
    float *res;
    int32_t *cell, *delta;
    uint8_t *cls;
    int32_t *element;
};
__device__ __forceinline__ WallCheckJointOut *wkj_out()
{
    __shared__ WallCheckJointOut o;
    return &o;
}
// block-shared: the joint planes
__device__ __forceinline__ JointPlaneLds &wkj_planes()
{
    __shared__ JointPlaneLds pl;
    return pl;
}

struct WallCheckJointPred {
    WallCheckJointArgs a;
    using Payload = WallCheckPayload;
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const
    {
        const uint32_t nside = a.n_sides;
        p.q = a.pts[i];
        const float4 q = p.q;
        const uint32_t lab = a.labels ? a.labels[i] : 0u;
        const uint32_t owner = joint_owner(q, wkj_planes(), nside);
        float e = __builtin_nanf("");
        int cell = -1;      // the owner's cell j * n_sectors + k (< 2^24)
        long long delta = 0;
        uint32_t cls = (uint32_t)GM_WALL_CHECK_CLS_PLANE;
#pragma unroll 1
        for (uint32_t s = 0; s < nside; ++s) {   // s is wave-uniform: the side's block is read once per wave
            if (owner != s) continue;
            const WallJointSide &S = a.side[s];
            int64_t j = -1;
            float jl = 0.0f;
            uint32_t kk = 0u;
            const bool mapped = joint_side_chain(q, lab, S, a.grid, a.gate, e, jl, kk, j, cls);
            if (mapped) {
                cell = (int)((uint32_t)j * a.grid.n_sectors + kk);   // < the owner's n_stations * n_sectors <= 2^24
                cls = wall_check_cell(S.table, cell, a.reference, a.min_count, a.T, e, delta);
            }
            wall_check_count<kCheckJointWords>(cls, s * (uint32_t)GM_WALL_CHECK_N_CLS);   // (the lanes this side owns)
        }
        if (a.outputs) {   // (wave-uniform: the stage call)
            const WallCheckJointOut o = *wkj_out();
            if (o.res) o.res[i] = e;
            if (o.cell) o.cell[i] = cell;
            if (o.delta) o.delta[i] = wall_check_delta32(delta);
            if (o.cls) o.cls[i] = (uint8_t)cls;
            if (o.element) o.element[i] = a.side[0].element + (int32_t)owner;   // (the sides are consecutive elements)
        }
        p.e = e;
        p.cell = cell >= 0 ? (int)(owner << 24 | (uint32_t)cell) : -1;
        p.delta = delta;
        return cls >= (uint32_t)GM_WALL_CHECK_CLS_CHANGED_POS;
    }
};

// What the emit step and finish() read again behind the predicates: parked in LDS by prepare(), so that the eight scalar
// registers are free while the chains run.
struct WallCheckJointTail {
    gm_wall_check_point *out;
    unsigned long long *ctr;          // [kWallCheckJointCounters]
    const uint32_t *n_ptr;            // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t row_is_index;
};
__device__ __forceinline__ WallCheckJointTail *wkj_tail()
{
    __shared__ WallCheckJointTail t;
    return &t;
}

struct WallCheckJointEmit {
    static constexpr bool kHasFinish = true, kHasPrepare = true;
    WallCheckJointTail tail;
    WallCheckJointOut outputs;
    WallJointPlanes planes;
    long long q_pos, q_neg;           // this thread's largest / smallest emitted delta
    __device__ __forceinline__ void prepare()
    {
        wall_check_prepare<kCheckJointWords>();
        if (threadIdx.x == 0) {   // (constant indices: the blocks stay kernel arguments, in scalar registers)
            *wkj_tail() = tail;
            *wkj_out() = outputs;
            joint_planes_store(wkj_planes(), planes);
        }
        q_pos = 0; q_neg = 0;
    }
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallCheckPayload &p)
    {
        wall_check_row(wkj_tail()->out, wkj_tail()->row_is_index, src, dst, p, q_pos, q_neg);
    }
    __device__ __forceinline__ void finish(uint32_t tile)
    {
        const WallCheckJointTail t = *wkj_tail();
        if (tile == 0u && threadIdx.x == 0) t.ctr[10] = t.n_ptr ? *t.n_ptr : t.n_host;   // n_points (>= 1 here; the caller's zero stands for 0)
        wall_check_finish<kCheckJointWords>(t.ctr + kWallCheckCounters, t.ctr + GM_WALL_CHECK_N_CLS, q_pos, q_neg);
    }
};

void launch_wall_check_joint(const WallCheckJointArgs &a, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    WallCheckJointPred pred{a};
    pred.a.outputs = (a.res || a.cell || a.delta || a.cls || a.element) ? 1u : 0u;
    WallCheckJointEmit emit;
    memset(&emit, 0, sizeof(emit));
    emit.tail = WallCheckJointTail{a.out, a.ctr, a.n_ptr, a.n_host, a.row_is_index};
    emit.outputs = WallCheckJointOut{a.res, a.cell, a.delta, a.cls, a.element};
    emit.planes = a.planes;
    hipLaunchKernelGGL((k_compact<WallCheckJointPred, WallCheckJointEmit>), dim3(compact_grid(n_cap ? n_cap : 1u)), dim3(kCpThreads), 0, s,
                       pred, emit, a.n_ptr, a.n_host, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

}  // namespace gm
