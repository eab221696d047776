// gm_wall_alignment.hpp -- the wall alignment's object and what its call families share (gm_wall_alignment.hip: create,
// destroy, map, info, sync and the add; gm_wall_alignment_locate.hip; gm_wall_alignment_check.hip: the check and the checked
// add; gm_wall_alignment_objects.hip: a check's objects; gm_wall_alignment_regions.hip: the regions of a window): the plan of a call and its refusals, the sides of a plan as the joint kernels take them, the add's arguments.
#pragma once

#include "gm_wall_joint.hpp"
#include "gm_wall_map.hpp"

struct gm_wall_alignment {
    gm_ctx *ctx = nullptr;
    gm::wall::Alignment A;
    std::vector<gm_wall_map *> maps;   // one per element, owned (they are also in ctx->walls)
    gm::wall::PointOutputs pt;         // the per-point outputs of the stage calls across a joint: the alignment's own, not a map's
    // gm_wall_alignment_locate_*: the state of one (alignment, slot), its device blocks allocated by the first locate that is
    // not an element map's own; the pending results are what the element maps' adds wait for (gm_wall_map::al_locates)
    struct LocateSlot {
        gm::DevArray<gm::WallLocateJointWork> work;     // the state between the passes, the result behind them
        gm::DevArray<double> partial;                   // [kFitBlocks][kFitRowLen] partial rows of a pass
        gm::DevArray<uint32_t> ticket;                  // last-block ticket of the passes (0 between launches)
        gm::HostArray<gm::WallLocateJointWork> h_work;  // pinned copy, valid once the result has been waited for
        gm_wall_alignment_locate_start start;           // what the result is composed from
        gm_wall_map *own = nullptr;                     // the last locate was this element map's own (one straight side)
        bool have = false;
    };
    std::vector<LocateSlot> locates;            // per slot of ctx
    std::vector<gm::wall::PendingResult> locate_res;
    // gm_wall_alignment_check_* and _add_*_checked: the state of one (alignment, slot).  The device blocks are allocated by
    // the first call that is not an element map's own; the pending checks are what the element maps' adds wait for
    // (gm_wall_map::al_checks)
    struct CheckSlot {
        gm::DevArray<gm_wall_check_point> stage;    // the changed rows of the last check across a joint, in order
        gm::wall::ScanRecords scan;                 // the check's own chained scan
        gm::DevArray<unsigned long long> ctr;       // device [kWallCheckJointCounters]
        gm::HostArray<unsigned long long> h_ctr;    // pinned copy, valid once the result has been waited for
        gm::DevArray<unsigned long long> blk;       // the checked add: [kWallAddCheckedCounters] | one mask bit per point
        gm::HostArray<unsigned long long> h_add;    // pinned copy of its counters
        gm_wall_alignment_add_info plan;            // of the last check
        gm_wall_map *own = nullptr;                 // the last check was this element map's own (one side)
        uint32_t own_epoch = 0;                     // ... and that map's scan epoch behind it: a later check there replaces the rows
        uint32_t status = 0;
        long long T = 0;
        uint64_t cloud_seq = 0;                     // the slot's cloud_seq at the enqueue
        bool have = false;
        uint32_t add_status = 0;                    // of the last checked add
        long long S = 0;
    };
    std::vector<CheckSlot> checks;              // per slot of ctx
    std::vector<gm::wall::PendingResult> check_res, add_res;
    // gm_wall_alignment_align_*: the state of one (alignment, slot).  The device blocks are allocated by the first align that
    // is not an element map's own; the pending aligns are what the element maps' adds wait for (gm_wall_map::al_aligns)
    struct AlignSlot {
        gm::DevArray<uint8_t> zeroed;               // counters | score table | patch sums | patch counts: one zero-fill per align
        gm::DevArray<int32_t> f, m;                 // the two value images
        gm::HostArray<uint8_t> h_res;               // pinned copy of counters | score table, valid once the result has been waited for
        gm_wall_align_params prm;                   // of the last align
        double pose[12];                            // the caller's pose of that align
        gm_wall_alignment_align_plan_info plan;     // its plan
        uint32_t n_shifts = 0;                      // (2A + 1)(2B + 1)
        gm_wall_map *own = nullptr;                 // the last align was this element map's own (one straight side)
        bool have = false;
    };
    std::vector<AlignSlot> aligns;              // per slot of ctx
    std::vector<gm::wall::PendingResult> align_res;
    // gm_wall_alignment_check_objects / _rows: the tile and the scratch, allocated by the first call
    gm::wall::ObjectScratch ob;
    // gm_wall_alignment_regions: the scratch, allocated by the first call (the tile is element map 0's); what a baseline is
    // compared by: the template and the element list as the create was given them
    gm::wall::RegionScratch rg;
    gm::HostArray<gm::WallRegionPiece> rg_pieces_host;   // pinned: the table of the call in progress
    gm_wall_params tpl;
    std::vector<gm_wall_element> elements;
    // the checked add's stage call: the uploaded rows and its block
    gm::DevArray<gm_wall_check_point> ac_rows;
    gm::DevArray<unsigned long long> ac_blk;
};

namespace gm {
namespace wall {

// A refusal of a plan (alignment_add_plan, alignment_locate_start) as the call's failure.
gm_status joint_refusal(gm_ctx *ctx, gm_status st);
// The plan of an add or a check under `pose`; side[k]: the element map of the plan's side k.
gm_status joint_plan(gm_wall_alignment *al, const double pose[12], gm_wall_alignment_add_info &plan,
                     gm_wall_map *(&side)[GM_WALL_JOINT_MAX_SIDES]);
// The sides of a plan of two or more as the add's and the check's kernel take them: each side under the frame its own
// map's add computes (add_frame_args of each element map, unchanged; win_first and win_stations: that map's own window),
// the grid from side 0, the joint planes.
gm_status joint_sides(gm_wall_map *const (&map)[GM_WALL_JOINT_MAX_SIDES], const double pose[12], const gm_wall_alignment_add_info &plan,
                      WallJointSide (&side)[GM_WALL_JOINT_MAX_SIDES], WallJointGrid &grid, WallJointPlanes &planes);
// the point fields of a joint kernel's arguments: frame_points' or a stage call's upload's
template <class JointArgs>
void joint_points(JointArgs &a, const WallArgs &w)
{
    a.pts = w.pts; a.labels = w.labels; a.n_ptr = w.n_ptr; a.n_host = w.n_host;
}

// a stage call's upload for a joint kernel: the point fields, and residual, cell and element where they are wanted
template <class JointArgs>
gm_status joint_upload(StageCall &sc, const float *xyz, const uint8_t *labels, JointArgs &a)
{
    WallArgs w;
    memset(&w, 0, sizeof(w));
    GMW_OK(sc.upload(xyz, labels, w));
    joint_points(a, w);
    a.res = w.res; a.cell = w.cell; a.element = sc.out.dev_element();
    return GM_OK;
}

// The sides of an add under `pose`: the plan, and for two or more sides the kernel's arguments but for the points.
// One side: side[0] is the map the add goes to, by its own add.
struct JointAdd {
    gm_wall_alignment_add_info plan;
    WallJointArgs ja;
    gm_wall_map *side[GM_WALL_JOINT_MAX_SIDES] = {};
};
gm_status joint_add_args(gm_wall_alignment *al, const double pose[12], JointAdd &j);

}  // namespace wall
}  // namespace gm
