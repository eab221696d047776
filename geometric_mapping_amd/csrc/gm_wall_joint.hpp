// gm_wall_joint.hpp -- what the kernels over the sides of a wall alignment's plan share (k_wall_joint.hip's k_wall_add_joint,
// k_wall_check_joint.hip's predicate, k_wall_locate_joint.hip; gm_wall_alignment*.hip fill the arguments): the side, the
// grid and the joint planes of their argument structs, the owner rule, and one trip of the add's and the check's side loop.
// The kernels of a single map (k_wall.hip, k_wall_check.hip, k_wall_locate.hip) do not include it.
#pragma once

#include "gm_internal.hpp"

namespace gm {

// One side of the add and of the check: an element map under the frame its own add computes (add_frame_args).
struct WallJointSide {
    int64_t anchor;            // j_f of this side's own add
    float o[3], a[3], u[3], v[3];   // its frame-local map frame, as WallArgs
    WallClothoid ax;           // its axis block (an arc side fills ax.arc alone, a straight side nothing)
    WallTable table;
    uint32_t n_stations;
    int32_t win_first;         // the add's LDS window, as WallArgs: whole stations of the element (the check reads none of
    uint32_t win_stations;     // the three)
    uint32_t lds_first;        // the window's first cell in the block's LDS table
    int32_t axis;              // kAxisStraight, kAxisArc, kAxisClothoid
    int32_t element;           // the element's index in the alignment
};
struct WallJointGrid {         // one grid for every element of an alignment
    float R, station_length, sector_angle, two_pi;
    uint32_t n_sectors;
};
struct WallJointPlanes {
    float jo[GM_WALL_JOINT_MAX_SIDES - 1][3];   // Jo' of the joint between side i and side i + 1
    float ja[GM_WALL_JOINT_MAX_SIDES - 1][3];   // aJ'
};

// k_wall_joint.hip (gm_wall_alignment_add_*): one launch for a frame that straddles joints of an alignment.  Each point is
// owned by one side (an element map) and runs that side's chain alone.
struct WallJointArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t n_sides;          // 2 .. GM_WALL_JOINT_MAX_SIDES
    uint32_t lds_cells;        // the cells of the LDS table dealt to the sides' windows, <= GM_SURF_MAX_CELLS
    float gate;
    WallJointGrid grid;
    WallJointPlanes planes;
    float *res;                // stage call only (nullptr in the frame path)
    int32_t *cell;
    int32_t *element;
    WallJointSide side[GM_WALL_JOINT_MAX_SIDES];
};
void launch_wall_add_joint(const WallJointArgs &a, uint32_t n_cap, uint32_t points_per_block, hipStream_t s);
// k_wall_add_joint over the points whose mask bit is clear (gm_wall_alignment_add_*_checked): skipped and the four point
// classes, summed over the sides, also go to ctr[4 .. 8]
void launch_wall_add_joint_masked(const WallJointArgs &a, const unsigned long long *mask, unsigned long long *ctr, uint32_t n_cap,
                                  uint32_t points_per_block, hipStream_t s);

// k_wall_check_joint.hip (gm_wall_alignment_check_*): one k_compact launch over the sides of an alignment's plan, every
// point on its owner's chain and against its owner's table.  u64 words: the first kWallCheckCounters as k_wall_check's (the
// seven summed classes are left to the host), then the classes per side [GM_WALL_JOINT_MAX_SIDES][GM_WALL_CHECK_N_CLS].
constexpr int kWallCheckJointCounters = kWallCheckCounters + GM_WALL_JOINT_MAX_SIDES * GM_WALL_CHECK_N_CLS;
struct WallCheckJointArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t n_sides;          // 2 .. GM_WALL_JOINT_MAX_SIDES
    uint32_t reference, min_count;
    uint32_t row_is_index;     // stage call: row = index
    uint32_t outputs;          // set by the launch: one of the five per-point outputs below is wanted
    long long T;
    float gate;                // the check's
    WallJointGrid grid;
    WallJointPlanes planes;
    gm_wall_check_point *out;  // staging, >= n_cap rows
    unsigned long long *ctr;   // [kWallCheckJointCounters], zeroed by the caller on the same stream
    float *res;                // stage call only (nullptr in the frame path)
    int32_t *cell;
    int32_t *delta;
    uint8_t *cls;
    int32_t *element;
    WallJointSide side[GM_WALL_JOINT_MAX_SIDES];
};
void launch_wall_check_joint(const WallCheckJointArgs &a, uint32_t n_cap, const ScanState &st, hipStream_t s);

// k_wall_locate_joint.hip (gm_wall_alignment_locate_*): k_wall_locate over the sides of an alignment's plan, every point on
// its owner's chain.  The fp32 blocks of a pass -- every side's four vectors, the joint planes -- are the images of the
// attached vectors (h: home-section coordinates, fp64) under the pass's state.
struct WallLocateJointBlocks {
    float side[GM_WALL_JOINT_MAX_SIDES][12];        // o', a', n', b' (straight: o', a', u', v')
    WallJointPlanes planes;
};
struct WallLocateJointWork {
    double c[3], d[3], u[3], v[3];   // the state in sensor coordinates, fp64
    double lateral[2], tilt[2];
    double last_step;
    uint32_t status, passes, n_points, pad;
    WallLocateJointBlocks next;      // the blocks of the pass to come, written by the solve of the pass before
    gm_wall_alignment_locate_pass pass[GM_LOCATE_PASSES];
};
struct WallLocateJointSide {
    WallTable table;
    int64_t anchor;            // j_f of this side's own add
    uint32_t n_stations;
    int32_t axis;              // kAxisStraight, kAxisArc, kAxisClothoid
    int32_t element;
    float kappa, rate, un, ub, vn, vb;
};
struct WallLocateJointArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t n_sides;          // 1 .. GM_WALL_JOINT_MAX_SIDES
    uint32_t reference, min_count;
    WallJointGrid grid;
    double gate;               // of pass 0
    double c0[3], d0[3], u0[3], v0[3], s0;   // the start, fp64, not rounded
    WallLocateJointBlocks first;             // the blocks of pass 0
    double h_side[GM_WALL_JOINT_MAX_SIDES][12];      // the attached vectors: a point's h, then three directions' per side
    double h_joint[GM_WALL_JOINT_MAX_SIDES - 1][6];  // h of J, h of aJ
    WallLocateJointSide side[GM_WALL_JOINT_MAX_SIDES];
    WallLocateJointWork *work;
    double *partial;           // [kFitBlocks][kFitRowLen]
    uint32_t *ticket;          // 0 between launches
    float *res;                // stage call only: all three or none (nullptr in the frame path)
    int32_t *cell;
    int32_t *element;
};
void launch_wall_locate_joint(const WallLocateJointArgs &a, hipStream_t s);   // the three passes
// the image of an attached vector h under the state (c, d, u, v): a point or a direction, rounded to fp32 once
__host__ __device__ inline void wall_locate_image(const double *h, bool point, const double *c, const double *d, const double *u,
                                                  const double *v, float *out)
{
    for (int k = 0; k < 3; ++k) {
        const double r = (h[0] * d[k] + h[1] * u[k]) + h[2] * v[k];
        out[k] = (float)(point ? c[k] + r : r);
    }
}
// every block of a pass: the images of a's attached vectors under the state
__host__ __device__ inline void wall_locate_blocks(const WallLocateJointArgs &a, const double *c, const double *d, const double *u,
                                                   const double *v, WallLocateJointBlocks &b)
{
    for (int s = 0; s < GM_WALL_JOINT_MAX_SIDES; ++s)
        for (int q = 0; q < 4; ++q) wall_locate_image(&a.h_side[s][3 * q], q == 0, c, d, u, v, &b.side[s][3 * q]);
    for (int j = 0; j < GM_WALL_JOINT_MAX_SIDES - 1; ++j) {
        wall_locate_image(&a.h_joint[j][0], true, c, d, u, v, b.planes.jo[j]);
        wall_locate_image(&a.h_joint[j][3], false, c, d, u, v, b.planes.ja[j]);
    }
}

// k_wall_align_joint.hip (gm_wall_alignment_align_*): k_wall_align_bin and k_wall_align_values over an alignment; the score
// kernel is k_wall_align.hip's, on a WallAlignArgs that carries the images and the table alone.
// u64 words: the first kWallAlignCounters as k_wall_align_bin's (plane, beyond_gate, outside_patch, binned summed over the
// sides, n_points, patch_cells_usable), then the four classes per side [GM_WALL_JOINT_MAX_SIDES][4].
constexpr int kWallAlignJointCounters = kWallAlignCounters + GM_WALL_JOINT_MAX_SIDES * 4;
struct WallAlignJointArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t n_sides;          // 1 .. GM_WALL_JOINT_MAX_SIDES
    uint32_t P;                // half_patch_stations
    float gate;                // the align's
    WallJointGrid grid;
    WallJointPlanes planes;
    int32_t row0[GM_WALL_JOINT_MAX_SIDES];   // patch row of the side's anchor station: jr = row0 + jl
    unsigned long long *ctr;   // [kWallAlignJointCounters]  } one block, zeroed by the caller on the same stream
    unsigned long long *p_sum; // [2P n_sectors] the patch   }
    uint32_t *p_cnt;           // [2P n_sectors]             }
    float *res;                // stage call only (nullptr in the frame path)
    int32_t *cell;
    int32_t *element;
    WallJointSide side[GM_WALL_JOINT_MAX_SIDES];   // (table, window fields unused)
};
// an element the map image's rows meet
struct WallAlignPiece {
    WallTable table;
    int64_t first_row;         // the global station of the element's station 0
    uint32_t n_stations;
    uint32_t pad;
};
struct WallAlignJointValuesArgs {
    uint32_t P, A, n_sectors, min_count, min_frame_count;
    uint32_t n_pieces;         // 0 .. GM_WALL_ALIGN_MAX_PIECES
    int64_t g0;                // the image's first global row G_f - P - A
    unsigned long long *ctr;   // [kWallAlignJointCounters]
    const unsigned long long *p_sum;
    const uint32_t *p_cnt;
    int32_t *f;                // [2P n_sectors]
    int32_t *m;                // [(2P + 2A) n_sectors]
    WallAlignPiece piece[GM_WALL_ALIGN_MAX_PIECES];
};
void launch_wall_align_bin_joint(const WallAlignJointArgs &a, uint32_t n_cap, hipStream_t s);
void launch_wall_align_values_joint(const WallAlignJointValuesArgs &a, hipStream_t s);   // behind the wait on the adds

// ---- device side ----

// The joint planes of a block in LDS, Jo' then aJ' per joint: the kernels read them per point from there (a broadcast), 18
// scalar registers less beside the sides' frames.  One thread stores them ahead of the block's barrier.
using JointPlaneLds = float[GM_WALL_JOINT_MAX_SIDES - 1][6];
__device__ __forceinline__ void joint_planes_store(JointPlaneLds &pl, const WallJointPlanes &p)
{
#pragma unroll
    for (int jn = 0; jn < GM_WALL_JOINT_MAX_SIDES - 1; ++jn)
#pragma unroll
        for (int k = 0; k < 3; ++k) { pl[jn][k] = p.jo[jn][k]; pl[jn][3 + k] = p.ja[jn][k]; }
}

// The owner of a point: d_i = (p - Jo'_i).aJ'_i for the joint planes in ascending order, the side before the first d_i < 0,
// the last of the nside sides if there is none.
// joint_behind: d < 0 for one plane pl (Jo', then aJ').
__device__ __forceinline__ bool joint_behind(const float4 &q, const float (&pl)[6])
{
    const float qx = __fsub_rn(q.x, pl[0]), qy = __fsub_rn(q.y, pl[1]), qz = __fsub_rn(q.z, pl[2]);
    const float aj[3] = {pl[3], pl[4], pl[5]};
    return surf_dot3(qx, qy, qz, aj) < 0.0f;
}
// kGuard false: the planes past the plan's last joint are read too, for a caller that has made their d never < 0
// (k_wall_locate_joint.hip says how).  k_wall_joint.hip writes this loop out over joint_behind, and says why.
template <bool kGuard = true>
__device__ __forceinline__ uint32_t joint_owner(const float4 &q, const JointPlaneLds &planes, uint32_t nside)
{
    uint32_t owner = nside - 1u;
#pragma unroll
    for (int jn = GM_WALL_JOINT_MAX_SIDES - 2; jn >= 0; --jn) {   // descending: the lowest joint with d < 0 stays
        if (!kGuard || (uint32_t)jn + 1u < nside) {               // (wave-uniform)
            if (joint_behind(q, planes[jn])) owner = (uint32_t)jn;
        }
    }
    return owner;
}

// what wall_chain and wall_station read of WallArgs, of one side
struct JointChainArgs {
    float o[3], a[3], u[3], v[3];
    float R, station_length, gate, sector_angle, two_pi;
    uint32_t n_sectors, n_stations;
    int64_t anchor;
};

// One trip of a side loop, for the lanes side S owns: S's chain under the call's gate, behind a wave-uniform switch on the
// side's axis kind in front of the three chain heads of gm_device.hpp (wall_chain, exactly as the kernels of a single map
// instantiate it).  S is read through uniform addresses: the side's frame stays in scalar registers.  in_range(w, jl) is
// the caller's range rule on the side's JointChainArgs w.  Returns whether the point passed gate and range; e, jl, kk are
// wall_chain's, cls the chain's class (kChain*).
template <class InRange>
__device__ __forceinline__ bool joint_side_chain_in(const float4 &q, uint32_t lab, const WallJointSide &S, const WallJointGrid &g,
                                                    float gate, InRange in_range_of, float &e, float &jl, uint32_t &kk, uint32_t &cls)
{
    JointChainArgs w;
    for (int k = 0; k < 3; ++k) { w.o[k] = S.o[k]; w.a[k] = S.a[k]; w.u[k] = S.u[k]; w.v[k] = S.v[k]; }
    w.R = g.R; w.station_length = g.station_length; w.gate = gate; w.sector_angle = g.sector_angle; w.two_pi = g.two_pi;
    w.n_sectors = g.n_sectors; w.n_stations = S.n_stations; w.anchor = S.anchor;
    auto in_range = [&](float x) { return in_range_of(w, x); };
    auto count = [&](uint32_t k) { cls = k; };
    if (S.axis == kAxisClothoid) return wall_chain(q, lab, w, WallClothoidArg{S.ax}, in_range, count, e, jl, kk);
    if (S.axis == kAxisArc) return wall_chain(q, lab, w, WallArcArg<true>{S.ax.arc}, in_range, count, e, jl, kk);
    return wall_chain(q, lab, w, WallArcArg<false>(), in_range, count, e, jl, kk);
}
// The add's and the check's trip: the range is the side's map (wall_station).  Returns whether the point is mapped; j the
// map's station of a mapped point.
__device__ __forceinline__ bool joint_side_chain(const float4 &q, uint32_t lab, const WallJointSide &S, const WallJointGrid &g, float gate,
                                                 float &e, float &jl, uint32_t &kk, int64_t &j, uint32_t &cls)
{
    return joint_side_chain_in(q, lab, S, g, gate, [&](const JointChainArgs &w, float x) { return (j = wall_station(w, x)) >= 0; }, e, jl,
                               kk, cls);
}

}  // namespace gm
