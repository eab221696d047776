// gm_wall_alignment.hip -- C ABI of the wall alignment (gm_wall_alignment_*; include/gm_hip.h states the rule): the calls
// on a context.  Host logic only: the element maps, the sides of an add, their per-add frames (add_frame_args of each
// element map, unchanged), the deal of the LDS table, and the locate (gm_wall_alignment_locate_*): its arguments, the
// scratch of an (alignment, slot), enqueue, result and pose; the check (gm_wall_alignment_check_*) and the add less its
// selected rows (gm_wall_alignment_add_*_checked) alike.  The kernels are k_wall_joint.hip's, k_wall_locate_joint.hip's,
// k_wall_check_joint.hip's and k_wall_add_checked.hip's mark; the device-free calls are in gm_wall_alignment_host.hip.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

struct gm_wall_alignment {
    gm_ctx *ctx = nullptr;
    Alignment A;
    std::vector<gm_wall_map *> maps;   // one per element, owned (they are also in ctx->walls)
    // the stage call's per-point outputs (gm_wall_alignment_add_points across a joint): all three are the alignment's own
    DevArray<float> pt_res;
    DevArray<int32_t> pt_cell, pt_element;
    // gm_wall_alignment_locate_*: the state of one (alignment, slot), allocated by the first locate that is not an element
    // map's own; the pending results are what the element maps' adds wait for (gm_wall_map::al_locates)
    struct LocateSlot {
        DevArray<WallLocateJointWork> work;     // the state between the passes, the result behind them
        DevArray<double> partial;               // [kFitBlocks][kFitRowLen] partial rows of a pass
        DevArray<uint32_t> ticket;              // last-block ticket of the passes (0 between launches)
        HostArray<WallLocateJointWork> h_work;  // pinned copy, valid once the result has been waited for
        gm_wall_alignment_locate_start start;   // what the result is composed from
        gm_wall_map *own = nullptr;             // the last locate was this element map's own (one straight side)
        bool have = false;
    };
    std::vector<LocateSlot> locates;            // per slot of ctx
    std::vector<PendingResult> locate_res;
    // gm_wall_alignment_check_* and _add_*_checked: the state of one (alignment, slot).  The device blocks are allocated by
    // the first call that is not an element map's own; the pending checks are what the element maps' adds wait for
    // (gm_wall_map::al_checks)
    struct CheckSlot {
        DevArray<gm_wall_check_point> stage;    // the changed rows of the last check across a joint, in order
        ScanRecords scan;                       // the check's own chained scan
        DevArray<unsigned long long> ctr;       // device [kWallCheckJointCounters]
        HostArray<unsigned long long> h_ctr;    // pinned copy, valid once the result has been waited for
        DevArray<unsigned long long> blk;       // the checked add: [kWallAddCheckedCounters] | one mask bit per point
        HostArray<unsigned long long> h_add;    // pinned copy of its counters
        gm_wall_alignment_add_info plan;        // of the last check
        gm_wall_map *own = nullptr;             // the last check was this element map's own (one side)
        uint32_t own_epoch = 0;                 // ... and that map's scan epoch behind it: a later check there replaces the rows
        uint32_t status = 0;
        long long T = 0;
        uint64_t cloud_seq = 0;                 // the slot's cloud_seq at the enqueue
        bool have = false;
        uint32_t add_status = 0;                // of the last checked add
        long long S = 0;
    };
    std::vector<CheckSlot> checks;              // per slot of ctx
    std::vector<PendingResult> check_res, add_res;
    // the stage calls' own: two more per-point outputs of a check, the uploaded rows and the block of a checked add
    DevArray<int32_t> pt_delta;
    DevArray<uint8_t> pt_cls;
    DevArray<gm_wall_check_point> ac_rows;
    DevArray<unsigned long long> ac_blk;
};

namespace {

// The sides of an add under `pose`: the plan, and for two or more sides the kernel's arguments but for the points.
// One side: side[0] is the map the add goes to, by its own add.
struct JointAdd {
    gm_wall_alignment_add_info plan;
    WallJointArgs ja;
    gm_wall_map *side[GM_WALL_JOINT_MAX_SIDES] = {};
};

gm_status joint_add_args(gm_wall_alignment *al, const double pose[12], JointAdd &j)
{
    gm_ctx *ctx = al->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment: NULL pose");
    const gm_status st = alignment_add_plan(al->A, pose, ctx->cfg.boxFilterBound, &j.plan);
    if (st == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, st, "gm_wall_alignment: the frame's reach meets more than GM_WALL_JOINT_MAX_SIDES elements");
    if (st != GM_OK) return gm_fail(ctx, st, "gm_wall_alignment: bad pose, or a pose too far along the axis");
    const uint32_t ns = j.plan.n_sides;
    memset(&j.ja, 0, sizeof(j.ja));
    uint32_t left = GM_SURF_MAX_CELLS;
    for (uint32_t k = 0; k < ns; ++k) {
        gm_wall_map *m = al->maps[j.plan.side_element[k]];
        j.side[k] = m;
        if (ns < 2u) break;   // (the map's own add computes its frame)
        WallArgs w;
        WallClothoid ax;
        memset(&ax, 0, sizeof(ax));
        GMW_OK(add_frame_args(m, pose, nullptr, w, nullptr, &ax));
        WallJointSide &S = j.ja.side[k];
        S.anchor = w.anchor;
        for (int c = 0; c < 3; ++c) { S.o[c] = w.o[c]; S.a[c] = w.a[c]; S.u[c] = w.u[c]; S.v[c] = w.v[c]; }
        S.ax = ax;
        S.table = w.table;
        S.n_stations = w.n_stations;
        S.axis = m->is_clothoid() ? kAxisClothoid : (m->is_arc() ? kAxisArc : kAxisStraight);
        S.element = (int32_t)j.plan.side_element[k];
        // the window: the stations of the map's own window that lie in the element, cut to what the table has left
        const int64_t lo = std::max<int64_t>(w.anchor + w.win_first, 0);
        const int64_t hi = std::min<int64_t>(w.anchor + w.win_first + (int64_t)w.win_stations, (int64_t)w.n_stations);
        const uint32_t nsec = w.n_sectors;
        const uint32_t nst = (uint32_t)std::min<int64_t>(std::max<int64_t>(hi - lo, 0), (int64_t)(left / nsec));
        S.win_first = nst ? (int32_t)(lo - w.anchor) : 0;
        S.win_stations = nst;
        S.lds_first = GM_SURF_MAX_CELLS - left;
        left -= nst * nsec;
        if (k == 0u) {
            j.ja.n_sectors = nsec;
            j.ja.R = w.R; j.ja.station_length = w.station_length; j.ja.gate = w.gate;
            j.ja.sector_angle = w.sector_angle; j.ja.two_pi = w.two_pi;
        }
    }
    j.ja.n_sides = ns;
    j.ja.lds_cells = GM_SURF_MAX_CELLS - left;
    for (uint32_t k = 0; k + 1u < ns; ++k)
        for (int c = 0; c < 3; ++c) { j.ja.jo[k][c] = j.plan.joint_o[k][c]; j.ja.ja[k][c] = j.plan.joint_a[k][c]; }
    return GM_OK;
}

// The start of a locate under `pose`, and for a plan that is not one straight side the kernel's arguments but for the
// points and the scratch.  own: the element map whose own locate the call is.
struct JointLocate {
    gm_wall_alignment_locate_start start;
    WallLocateJointArgs a;
    gm_wall_map *own = nullptr;
    gm_wall_map *side[GM_WALL_JOINT_MAX_SIDES] = {};
};

gm_status joint_locate_args(gm_wall_alignment *al, const double pose[12], const gm_wall_locate_params &lp, JointLocate &j)
{
    gm_ctx *ctx = al->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment: NULL pose");
    const gm_status st = alignment_locate_start(al->A, pose, ctx->cfg.boxFilterBound, &j.start);
    if (st == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, st, "gm_wall_alignment: the frame's reach meets more than GM_WALL_JOINT_MAX_SIDES elements");
    if (st != GM_OK) return gm_fail(ctx, st, "gm_wall_alignment: bad pose, or a pose too far along the axis");
    const gm_wall_alignment_locate_start &S = j.start;
    const uint32_t ns = S.add.n_sides;
    for (uint32_t k = 0; k < ns; ++k) j.side[k] = al->maps[S.add.side_element[k]];
    if (ns == 1u && S.side_kind[0] == GM_WALL_ELEMENT_STRAIGHT) {
        j.own = j.side[0];
        return GM_OK;
    }
    WallLocateJointArgs &a = j.a;
    memset(&a, 0, sizeof(a));
    const gm_wall_map *m0 = j.side[0];
    a.n_sides = ns;
    a.n_sectors = m0->prm.n_sectors;
    a.reference = lp.reference;
    a.min_count = lp.min_count;
    a.R = (float)m0->frame.R;
    a.station_length = (float)m0->prm.station_length;
    a.sector_angle = (float)(kTwoPi / (double)m0->prm.n_sectors);
    a.two_pi = (float)kTwoPi;
    a.gate = lp.gate;
    a.s0 = S.s0;
    for (int c = 0; c < 3; ++c) { a.c0[c] = S.c[c]; a.d0[c] = S.d[c]; a.u0[c] = S.u[c]; a.v0[c] = S.v[c]; }
    memcpy(a.h_side, S.side, sizeof(a.h_side));
    memcpy(a.h_joint, S.joint, sizeof(a.h_joint));
    wall_locate_blocks(a, S.c, S.d, S.u, S.v, a.first);
    for (uint32_t k = 0; k < ns; ++k) {
        WallLocateJointSide &sd = a.side[k];
        sd.table = j.side[k]->table;
        sd.anchor = S.add.side_anchor[k];
        sd.n_stations = j.side[k]->prm.n_stations;
        sd.axis = S.side_kind[k] == GM_WALL_ELEMENT_CLOTHOID ? kAxisClothoid : (S.side_kind[k] == GM_WALL_ELEMENT_ARC ? kAxisArc : kAxisStraight);
        sd.element = (int32_t)S.add.side_element[k];
        sd.kappa = S.side_axis[k][0]; sd.rate = S.side_axis[k][1];
        sd.un = S.side_axis[k][2]; sd.ub = S.side_axis[k][3]; sd.vn = S.side_axis[k][4]; sd.vb = S.side_axis[k][5];
    }
    return GM_OK;
}

// the per-slot state of the alignment's locates, on the first of them (no device memory: vectors of empty owners); the
// element maps learn where the pending results are
gm_wall_alignment::LocateSlot &locate_slot(gm_wall_alignment *al, uint32_t slot)
{
    if (al->locates.empty()) {
        al->locates.resize(al->ctx->n_slots);
        al->locate_res.resize(al->ctx->n_slots);
        for (gm_wall_map *m : al->maps) m->al_locates = &al->locate_res;
    }
    return al->locates[slot];
}

// the scratch of (alignment, slot); a new ticket is zeroed on `s`
gm_status joint_locate_prepare(gm_wall_alignment *al, uint32_t slot, hipStream_t s, WallLocateJointArgs &a)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::LocateSlot &l = locate_slot(al, slot);
    GMW_OK(al->locate_res[slot].ensure(ctx));
    GMW_HIP(ctx, l.work.reserve(1));
    GMW_HIP(ctx, l.h_work.reserve(1));
    GMW_HIP(ctx, l.partial.reserve((uint64_t)kFitBlocks * kFitRowLen));
    if (!l.ticket) {
        GMW_HIP(ctx, l.ticket.reserve(1));
        GMW_HIP(ctx, hipMemsetAsync(l.ticket.p, 0, 4, s));
    }
    a.work = l.work.p;
    a.partial = l.partial.p;
    a.ticket = l.ticket.p;
    return GM_OK;
}

// the three passes, the copy of the result and the event behind them
gm_status joint_locate_enqueue(gm_wall_alignment *al, uint32_t slot, const JointLocate &j, hipStream_t s)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::LocateSlot &l = al->locates[slot];
    launch_wall_locate_joint(j.a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_work.p, l.work.p, sizeof(WallLocateJointWork), hipMemcpyDeviceToHost, s));
    GMW_OK(al->locate_res[slot].record(ctx, s));
    l.start = j.start;
    l.own = nullptr;
    l.have = true;
    return GM_OK;
}

void locate_info_head(const gm_wall_alignment_locate_start &S, gm_wall_alignment_locate_info *info)
{
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_locate_info);
    info->anchor_station = S.add.side_anchor[S.home];
    info->element = S.add.element;
    info->n_sides = S.add.n_sides;
    for (uint32_t k = 0; k < S.add.n_sides; ++k) {
        info->side_element[k] = S.add.side_element[k];
        info->side_kind[k] = S.side_kind[k];
        info->side_anchor[k] = S.add.side_anchor[k];
        for (int q = 0; q < 6; ++q) info->side_axis[k][q] = S.side_axis[k][q];
    }
}

// an element map's own locate as the alignment's info: the shared fields byte for byte
void locate_info_of_map(const gm_wall_alignment_locate_start &S, const gm_wall_locate_info &li, gm_wall_alignment_locate_info *info)
{
    locate_info_head(S, info);
    static_assert(offsetof(gm_wall_alignment_locate_info, element) == offsetof(gm_wall_locate_info, pass), "the shared head");
    memcpy(info, &li, offsetof(gm_wall_locate_info, pass));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_locate_info);
    for (int k = 0; k < GM_LOCATE_PASSES; ++k) {
        memcpy(&info->pass[k], &li.pass[k], sizeof(gm_wall_locate_pass));
        if ((uint32_t)k < li.passes || ((li.status & GM_LOCATE_FAILED_MASK) && (uint32_t)k == li.passes))
            memcpy(info->pass[k].side[0], li.pass[k].o, 12 * sizeof(float));
    }
}

// the result of (alignment, slot), waited for: the device's record, and the pose composed in fp64
gm_status joint_locate_result(gm_wall_alignment *al, uint32_t slot, gm_wall_alignment_locate_info *info)
{
    gm_wall_alignment::LocateSlot &l = al->locates[slot];
    GMW_OK(al->locate_res[slot].wait(al->ctx));
    const WallLocateJointWork &wk = *l.h_work.p;
    const gm_wall_alignment_locate_start &S = l.start;
    locate_info_head(S, info);
    info->status = wk.status;
    info->passes = wk.passes;
    info->n_points = wk.n_points;
    for (int k = 0; k < GM_LOCATE_PASSES; ++k) info->pass[k] = wk.pass[k];
    if (wk.status & GM_LOCATE_FAILED_MASK) {
        const double nan = __builtin_nan("");
        for (int k = 0; k < 12; ++k) info->pose[k] = nan;
        info->lateral[0] = info->lateral[1] = info->tilt[0] = info->tilt[1] = nan;
        return GM_OK;
    }
    if (wk.last_step > GM_FIT_STEP_BOUND) info->status |= GM_LOCATE_NOT_CONVERGED;
    for (int k = 0; k < 2; ++k) { info->lateral[k] = wk.lateral[k]; info->tilt[k] = wk.tilt[k]; }
    for (int r = 0; r < 3; ++r) {   // Rm' = a d^T + u u'^T + v v'^T, tr' = o_f - Rm' c
        double rc = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double e = S.a[r] * wk.d[c] + S.fu[r] * wk.u[c] + S.fv[r] * wk.v[c];
            info->pose[4 * r + c] = e;
            rc += e * wk.c[c];
        }
        info->pose[4 * r + 3] = S.o_f[r] - rc;
    }
    return GM_OK;
}

// the slot's last locate was the element map's own
void locate_note_own(gm_wall_alignment *al, uint32_t slot, const JointLocate &j)
{
    gm_wall_alignment::LocateSlot &l = locate_slot(al, slot);
    l.start = j.start;
    l.own = j.own;
    l.have = true;
}

// ---- gm_wall_alignment_check_* ----

// The plan of a check under `pose`, and for two or more sides the kernel's arguments but for the points and the scratch:
// each side's frame is the one its own map's check computes (the add's, the gate apart).  One side: side[0] is the map the
// check goes to, by its own check.
struct JointCheck {
    gm_wall_alignment_add_info plan;
    WallCheckJointArgs a;
    gm_wall_map *side[GM_WALL_JOINT_MAX_SIDES] = {};
};

gm_status joint_check_args(gm_wall_alignment *al, const double pose[12], const gm_wall_check_params &cp, JointCheck &j)
{
    gm_ctx *ctx = al->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment: NULL pose");
    const gm_status st = alignment_add_plan(al->A, pose, ctx->cfg.boxFilterBound, &j.plan);
    if (st == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, st, "gm_wall_alignment: the frame's reach meets more than GM_WALL_JOINT_MAX_SIDES elements");
    if (st != GM_OK) return gm_fail(ctx, st, "gm_wall_alignment: bad pose, or a pose too far along the axis");
    const uint32_t ns = j.plan.n_sides;
    for (uint32_t k = 0; k < ns; ++k) j.side[k] = al->maps[j.plan.side_element[k]];
    if (ns < 2u) return GM_OK;   // (the map's own check computes its frame)
    WallCheckJointArgs &a = j.a;
    a.n_sides = ns;
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    for (uint32_t k = 0; k < ns; ++k) {
        gm_wall_map *m = j.side[k];
        WallArgs w;
        WallClothoid ax;
        memset(&ax, 0, sizeof(ax));
        GMW_OK(add_frame_args(m, pose, nullptr, w, nullptr, &ax));
        WallCheckJointSide &S = a.side[k];
        S.anchor = w.anchor;
        for (int c = 0; c < 3; ++c) { S.o[c] = w.o[c]; S.a[c] = w.a[c]; S.u[c] = w.u[c]; S.v[c] = w.v[c]; }
        S.ax = ax;
        S.table = w.table;
        S.n_stations = w.n_stations;
        S.axis = m->is_clothoid() ? kAxisClothoid : (m->is_arc() ? kAxisArc : kAxisStraight);
        S.element = (int32_t)j.plan.side_element[k];
        if (k == 0u) {
            a.n_sectors = w.n_sectors;
            a.R = w.R; a.station_length = w.station_length; a.sector_angle = w.sector_angle; a.two_pi = w.two_pi;
        }
    }
    a.gate = (float)cp.gate;   // the check's own, rounded once
    for (uint32_t k = 0; k + 1u < ns; ++k)
        for (int c = 0; c < 3; ++c) { a.jo[k][c] = j.plan.joint_o[k][c]; a.ja[k][c] = j.plan.joint_a[k][c]; }
    return GM_OK;
}

// the per-slot state of the alignment's checks, on the first of them (no device memory: vectors of empty owners); the
// element maps learn where the pending results are
gm_wall_alignment::CheckSlot &check_slot(gm_wall_alignment *al, uint32_t slot)
{
    if (al->checks.empty()) {
        al->checks.resize(al->ctx->n_slots);
        al->check_res.resize(al->ctx->n_slots);
        al->add_res.resize(al->ctx->n_slots);
        for (gm_wall_map *m : al->maps) m->al_checks = &al->check_res;
    }
    return al->checks[slot];
}

// The scratch of (alignment, slot) for a check of up to n_cap points, and everything a launch on `s` needs before it:
// zeroed counters, a fresh scan state, the buffers in `a`.
gm_status joint_check_prepare(gm_wall_alignment *al, uint32_t slot, uint32_t n_cap, hipStream_t s, ScanState &st, WallCheckJointArgs &a)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::CheckSlot &c = check_slot(al, slot);
    GMW_OK(al->check_res[slot].ensure(ctx));
    GMW_HIP(ctx, c.ctr.reserve(kWallCheckJointCounters));
    GMW_HIP(ctx, c.h_ctr.reserve(kWallCheckJointCounters));
    if (c.stage.cap < n_cap || !c.scan.holds(n_cap)) {
        GMW_OK(al->check_res[slot].wait(ctx));   // the slot's last check may still be writing the old blocks
        GMW_OK(al->add_res[slot].wait(ctx));     // ... and a checked add behind it still reading the rows
        c.have = false;                          // (its rows go with the block)
    }
    GMW_HIP(ctx, c.stage.reserve(n_cap));
    GMW_OK(c.scan.reserve(ctx, n_cap, s));
    st = c.scan.next(s);
    a.out = c.stage.p;
    a.ctr = c.ctr.p;
    GMW_HIP(ctx, hipMemsetAsync(c.ctr.p, 0, kWallCheckJointCounters * 8, s));
    return GM_OK;
}

// the launch, the copy of its counters and the event behind both
gm_status joint_check_enqueue(gm_wall_alignment *al, uint32_t slot, const JointCheck &j, long long T, uint32_t n_cap,
                              const ScanState &st, hipStream_t s)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::CheckSlot &c = al->checks[slot];
    launch_wall_check_joint(j.a, n_cap, st, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(c.h_ctr.p, c.ctr.p, kWallCheckJointCounters * 8, hipMemcpyDeviceToHost, s));
    GMW_OK(al->check_res[slot].record(ctx, s));
    c.plan = j.plan;
    c.own = nullptr;
    c.status = j.plan.status;
    c.T = T;
    c.cloud_seq = ctx->slots[slot].cloud_seq;
    c.have = true;
    return GM_OK;
}

// the slot's last check was the element map's own
void check_note_own(gm_wall_alignment *al, uint32_t slot, const JointCheck &j)
{
    gm_wall_alignment::CheckSlot &c = check_slot(al, slot);
    c.plan = j.plan;
    c.own = j.side[0];
    c.own_epoch = j.side[0]->checks[slot].scan.epoch;
    c.cloud_seq = al->ctx->slots[slot].cloud_seq;
    c.have = true;
}

// an element map's own check as the alignment's info: the shared fields byte for byte, its classes as side 0's
void check_info_of_map(const gm_wall_check_info &ci, gm_wall_alignment_check_info *info)
{
    static_assert(offsetof(gm_wall_alignment_check_info, n_sides) == sizeof(gm_wall_check_info), "the shared head");
    memset(info, 0, sizeof(*info));
    memcpy(info, &ci, sizeof(ci));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_check_info);
    info->n_sides = 1u;
    const uint32_t cls[GM_WALL_CHECK_N_CLS] = {ci.plane, ci.beyond_gate, ci.outside, ci.unsurveyed, ci.unchanged, ci.changed_pos, ci.changed_neg};
    for (int k = 0; k < GM_WALL_CHECK_N_CLS; ++k) info->side_class[0][k] = cls[k];
}

// the result of (alignment, slot) of a check across a joint, waited for
gm_status joint_check_result(gm_wall_alignment *al, uint32_t slot, gm_wall_alignment_check_info *info, gm_wall_check_point *points,
                             uint32_t capacity, uint32_t *n_out)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::CheckSlot &c = al->checks[slot];
    GMW_OK(al->check_res[slot].wait(ctx));
    const unsigned long long *h = c.h_ctr.p;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->struct_size = (uint32_t)sizeof(gm_wall_alignment_check_info);
        info->status = c.status;
        info->threshold_q = c.T;
        info->n_points = (uint32_t)h[10];
        info->n_sides = c.plan.n_sides;
        uint32_t sum[GM_WALL_CHECK_N_CLS] = {};
        for (uint32_t k = 0; k < c.plan.n_sides; ++k)
            for (int q = 0; q < GM_WALL_CHECK_N_CLS; ++q) {
                info->side_class[k][q] = (uint32_t)h[kWallCheckCounters + k * GM_WALL_CHECK_N_CLS + q];
                sum[q] += info->side_class[k][q];
            }
        info->plane = sum[GM_WALL_CHECK_CLS_PLANE];
        info->beyond_gate = sum[GM_WALL_CHECK_CLS_BEYOND_GATE];
        info->outside = sum[GM_WALL_CHECK_CLS_OUTSIDE];
        info->unsurveyed = sum[GM_WALL_CHECK_CLS_UNSURVEYED];
        info->unchanged = sum[GM_WALL_CHECK_CLS_UNCHANGED];
        info->changed_pos = sum[GM_WALL_CHECK_CLS_CHANGED_POS];
        info->changed_neg = sum[GM_WALL_CHECK_CLS_CHANGED_NEG];
        info->peak_pos = (int64_t)h[7];
        info->peak_neg = (int64_t)(0ull - h[8]);
    }
    const uint32_t got = (uint32_t)h[9];
    if (n_out) *n_out = got;
    if (!points && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment check: NULL points with a capacity");
    if (!points) return GM_OK;   // a count query
    if (got > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_alignment check: point buffer too small");
    if (got) {   // on a map's own stream: the slot's may be busy with the next frame
        hipStream_t ms = al->maps[0]->stream;
        GMW_HIP(ctx, hipMemcpyAsync(points, c.stage.p, (size_t)got * sizeof(gm_wall_check_point), hipMemcpyDeviceToHost, ms));
        GMW_HIP(ctx, hipStreamSynchronize(ms));
    }
    return GM_OK;
}

// ---- gm_wall_alignment_add_*_checked ----

// the masked add of the plan `j` on `s` behind the mark: across a joint the one launch over all sides, else the side's own
// masked kernel under its own per-add frame
gm_status joint_add_masked(gm_wall_alignment *al, JointAdd &j, const double pose[12], const WallArgs &pts, float *res, int32_t *cell,
                           int32_t *element, unsigned long long *blk, uint32_t n_cap, hipStream_t s)
{
    const unsigned long long *mask = blk + kWallAddCheckedCounters;
    if (j.plan.n_sides >= 2u) {
        j.ja.pts = pts.pts; j.ja.labels = pts.labels; j.ja.n_ptr = pts.n_ptr; j.ja.n_host = pts.n_host;
        j.ja.res = res; j.ja.cell = cell; j.ja.element = element;
        launch_wall_add_joint_masked(j.ja, mask, blk, n_cap, j.side[0]->points_per_block, s);
    } else {
        gm_wall_map *m = j.side[0];
        WallArgs w;
        WallClothoid ax;
        memset(&ax, 0, sizeof(ax));
        GMW_OK(add_frame_args(m, pose, nullptr, w, nullptr, &ax));
        w.pts = pts.pts; w.labels = pts.labels; w.n_ptr = pts.n_ptr; w.n_host = pts.n_host;
        w.res = res; w.cell = cell;
        if (m->is_clothoid()) launch_wall_add_clothoid_masked(w, ax, mask, blk, n_cap, m->points_per_block, s);
        else if (m->is_arc()) launch_wall_add_arc_masked(w, ax.arc, mask, blk, n_cap, m->points_per_block, s);
        else launch_wall_add_masked(w, mask, blk, n_cap, m->points_per_block, s);
    }
    GMW_HIP(al->ctx, hipGetLastError());
    return GM_OK;
}

void free_alignment(gm_wall_alignment *al, bool maps_too)
{
    for (std::vector<PendingResult> *v : {&al->locate_res, &al->check_res, &al->add_res})
        for (PendingResult &r : *v) r.release();   // nothing may still be writing the alignment's blocks
    for (gm_wall_map *m : al->maps) { m->al_locates = nullptr; m->al_checks = nullptr; }
    if (maps_too)
        for (gm_wall_map *m : al->maps) gm_wall_map_destroy(m);
    delete al;
}

}  // namespace

namespace gm {
void gm_wall_alignment_free_all(gm_ctx *ctx)
{
    for (gm_wall_alignment *al : ctx->alignments) free_alignment(al, false);   // (gm_wall_free_all frees the maps)
    ctx->alignments.clear();
}
}  // namespace gm

extern "C" {

gm_status gm_wall_alignment_create(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                   gm_wall_alignment **alignment)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!alignment) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_create: NULL alignment");
    *alignment = nullptr;
    gm_wall_alignment *al = new gm_wall_alignment;
    al->ctx = ctx;
    const gm_status st = alignment_build(params, elements, n, al->A);
    if (st != GM_OK) {
        delete al;
        return gm_fail(ctx, st,
                       "gm_wall_alignment_create: NULL, no or too many elements, a struct_size or reserved mismatch, an unknown kind, or an "
                       "element outside the limits of its map");
    }
    for (const AlignElem &E : al->A.el) {
        gm_wall_map *m = nullptr;
        gm_status ms;
        if (E.kind == GM_WALL_ELEMENT_CLOTHOID) ms = gm_wall_map_create_clothoid(ctx, &E.p, &E.cl, &m);
        else if (E.kind == GM_WALL_ELEMENT_ARC) ms = gm_wall_map_create_arc(ctx, &E.p, &E.arc, &m);
        else ms = gm_wall_map_create(ctx, &E.p, &m);
        if (ms != GM_OK) {
            free_alignment(al, true);
            return ms;
        }
        al->maps.push_back(m);
    }
    ctx->alignments.push_back(al);
    *alignment = al;
    return GM_OK;
}

void gm_wall_alignment_destroy(gm_wall_alignment *alignment)
{
    if (!alignment) return;
    std::vector<gm_wall_alignment *> &v = alignment->ctx->alignments;
    v.erase(std::remove(v.begin(), v.end(), alignment), v.end());
    free_alignment(alignment, true);
}

gm_status gm_wall_alignment_map(gm_wall_alignment *alignment, uint32_t i, gm_wall_map **map)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    if (!map || i >= alignment->maps.size()) return gm_fail(alignment->ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_map: NULL map or no such element");
    *map = alignment->maps[i];
    return GM_OK;
}

gm_status gm_wall_alignment_add_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                      gm_wall_alignment_add_info *info)
{
    if (!alignment || !ctx) return GM_ERR_INVALID_ARG;
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(alignment->maps[0], ctx, slot, "gm_wall_alignment_add_frame", [] { return true; }, sl));
    JointAdd j;
    GMW_OK(joint_add_args(alignment, pose, j));
    if (info) *info = j.plan;
    if (j.plan.n_sides < 2u) return gm_wall_map_add_frame(j.side[0], ctx, slot, pose, nullptr);
    GMW_OK(set_device(ctx));
    WallArgs w;
    frame_points(ctx, *sl, w);
    j.ja.pts = w.pts; j.ja.labels = w.labels; j.ja.n_ptr = w.n_ptr; j.ja.n_host = w.n_host;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], slot, sl->stream));
    launch_wall_add_joint(j.ja, sl->n_in, j.side[0]->points_per_block, sl->stream);
    GMW_HIP(ctx, hipGetLastError());
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) {
        j.side[k]->pending[slot] = 1;
        ++j.side[k]->frames;
    }
    return GM_OK;
}

gm_status gm_wall_alignment_add_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                       const double pose[12], gm_wall_alignment_add_info *info, float *residual, int32_t *cell,
                                       int32_t *element)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_add_points: NULL xyz");
    JointAdd j;
    GMW_OK(joint_add_args(alignment, pose, j));
    if (info) *info = j.plan;
    if (j.plan.n_sides < 2u) {
        GMW_OK(gm_wall_map_add_points(j.side[0], xyz, n, labels, pose, nullptr, residual, cell));
        if (element)
            for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.plan.side_element[0];
        return GM_OK;
    }
    // (the staging slot is the context's; the per-point outputs are staged in the alignment's own buffers, not a map's)
    StageCall sc{j.side[0], n, nullptr, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    if (residual) GMW_HIP(ctx, alignment->pt_res.reserve(n));
    if (cell) GMW_HIP(ctx, alignment->pt_cell.reserve(n));
    if (element) GMW_HIP(ctx, alignment->pt_element.reserve(n));
    WallArgs w;
    memset(&w, 0, sizeof(w));
    GMW_OK(sc.upload(xyz, labels, w));
    j.ja.pts = w.pts; j.ja.labels = w.labels; j.ja.n_ptr = w.n_ptr; j.ja.n_host = w.n_host;
    j.ja.res = residual ? alignment->pt_res.p : nullptr;
    j.ja.cell = cell ? alignment->pt_cell.p : nullptr;
    j.ja.element = element ? alignment->pt_element.p : nullptr;
    hipStream_t s = sc.sl->stream;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], 0, s));   // (the staging slot is slot 0)
    launch_wall_add_joint(j.ja, n, j.side[0]->points_per_block, s);
    GMW_HIP(ctx, hipGetLastError());
    if (residual && n) GMW_HIP(ctx, hipMemcpyAsync(residual, alignment->pt_res.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cell && n) GMW_HIP(ctx, hipMemcpyAsync(cell, alignment->pt_cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (element && n) GMW_HIP(ctx, hipMemcpyAsync(element, alignment->pt_element.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) ++j.side[k]->frames;
    return GM_OK;
}

gm_status gm_wall_alignment_sync(gm_wall_alignment *alignment)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    for (gm_wall_map *m : alignment->maps) GMW_OK(gm_wall_map_sync(m));
    for (std::vector<PendingResult> *v : {&alignment->locate_res, &alignment->check_res, &alignment->add_res})
        for (PendingResult &r : *v) GMW_OK(r.wait(alignment->ctx));
    return GM_OK;
}

gm_status gm_wall_alignment_locate_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                         const gm_wall_locate_params *prm)
{
    if (!alignment || !ctx) return GM_ERR_INVALID_ARG;
    const gm_wall_locate_params lp = params_or(prm, gm_wall_locate_default_params);
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(alignment->maps[0], ctx, slot, "gm_wall_alignment_locate_frame", [&] { return locate_prm_ok(lp); }, sl));
    JointLocate j;
    GMW_OK(joint_locate_args(alignment, pose, lp, j));
    if (j.own) {
        GMW_OK(gm_wall_map_locate_frame(j.own, ctx, slot, pose, &lp));
        locate_note_own(alignment, slot, j);
        return GM_OK;
    }
    GMW_OK(set_device(ctx));
    GMW_OK(joint_locate_prepare(alignment, slot, sl->stream, j.a));
    for (uint32_t k = 0; k < j.start.add.n_sides; ++k) GMW_OK(wait_adds(j.side[k], slot, sl->stream));
    WallArgs w;
    frame_points(ctx, *sl, w);
    j.a.pts = w.pts; j.a.labels = w.labels; j.a.n_ptr = w.n_ptr; j.a.n_host = w.n_host;
    return joint_locate_enqueue(alignment, slot, j, sl->stream);
}

gm_status gm_wall_alignment_get_locate(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_locate_info *info)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_get_locate: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (alignment->locates.empty() || !alignment->locates[slot].have)
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_get_locate: no locate was enqueued on this alignment and slot");
    GMW_OK(set_device(ctx));
    const gm_wall_alignment::LocateSlot &l = alignment->locates[slot];
    if (l.own) {
        gm_wall_locate_info li;
        GMW_OK(gm_wall_map_get_locate(l.own, slot, &li));
        locate_info_of_map(l.start, li, info);
        return GM_OK;
    }
    return joint_locate_result(alignment, slot, info);
}

gm_status gm_wall_alignment_locate_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                          const double pose[12], const gm_wall_locate_params *prm,
                                          gm_wall_alignment_locate_info *info, float *residual, int32_t *cell, int32_t *element)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_locate_points: NULL info");
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_locate_points: NULL xyz");
    const gm_wall_locate_params lp = params_or(prm, gm_wall_locate_default_params);
    if (!locate_prm_ok(lp))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_locate_points: struct_size mismatch or a parameter outside its limits");
    JointLocate j;
    GMW_OK(joint_locate_args(alignment, pose, lp, j));
    if (j.own) {
        gm_wall_locate_info li;
        GMW_OK(gm_wall_map_locate_points(j.own, xyz, n, labels, pose, &lp, &li, residual, cell));
        locate_note_own(alignment, 0, j);
        locate_info_of_map(j.start, li, info);
        if (element)
            for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.start.add.side_element[0];
        return GM_OK;
    }
    StageCall sc{j.side[0], n, nullptr, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    const bool outputs = residual || cell || element;   // (the kernel writes all three or none)
    if (outputs) {
        GMW_HIP(ctx, alignment->pt_res.reserve(n ? n : 1u));
        GMW_HIP(ctx, alignment->pt_cell.reserve(n ? n : 1u));
        GMW_HIP(ctx, alignment->pt_element.reserve(n ? n : 1u));
    }
    hipStream_t s = sc.sl->stream;
    GMW_OK(joint_locate_prepare(alignment, 0, s, j.a));
    for (uint32_t k = 0; k < j.start.add.n_sides; ++k) GMW_OK(wait_adds(j.side[k], 0, s));
    WallArgs w;
    memset(&w, 0, sizeof(w));
    GMW_OK(sc.upload(xyz, labels, w));
    j.a.pts = w.pts; j.a.labels = w.labels; j.a.n_ptr = w.n_ptr; j.a.n_host = w.n_host;
    j.a.res = outputs ? alignment->pt_res.p : nullptr;
    j.a.cell = outputs ? alignment->pt_cell.p : nullptr;
    j.a.element = outputs ? alignment->pt_element.p : nullptr;
    GMW_OK(joint_locate_enqueue(alignment, 0, j, s));
    if (residual && n) GMW_HIP(ctx, hipMemcpyAsync(residual, alignment->pt_res.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cell && n) GMW_HIP(ctx, hipMemcpyAsync(cell, alignment->pt_cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (element && n) GMW_HIP(ctx, hipMemcpyAsync(element, alignment->pt_element.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    return joint_locate_result(alignment, 0, info);
}

gm_status gm_wall_alignment_check_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_check_params *prm, gm_wall_alignment_add_info *plan)
{
    if (!alignment || !ctx) return GM_ERR_INVALID_ARG;
    const gm_wall_check_params cp = params_or(prm, gm_wall_check_default_params);
    JointCheck j;
    memset(&j.a, 0, sizeof(j.a));
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(alignment->maps[0], ctx, slot, "gm_wall_alignment_check_frame", [&] { return check_prm_ok(cp, j.a.T); }, sl));
    GMW_OK(joint_check_args(alignment, pose, cp, j));
    if (plan) *plan = j.plan;
    if (j.plan.n_sides < 2u) {
        GMW_OK(gm_wall_map_check_frame(j.side[0], ctx, slot, pose, &cp, nullptr));
        check_note_own(alignment, slot, j);
        return GM_OK;
    }
    GMW_OK(set_device(ctx));
    const uint32_t n_cap = sl->n_in ? sl->n_in : 1u;
    ScanState scan;
    GMW_OK(joint_check_prepare(alignment, slot, n_cap, sl->stream, scan, j.a));
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(wait_adds(j.side[k], slot, sl->stream));
    WallArgs w;
    frame_points(ctx, *sl, w);
    j.a.pts = w.pts; j.a.labels = w.labels; j.a.n_ptr = w.n_ptr; j.a.n_host = w.n_host;
    return joint_check_enqueue(alignment, slot, j, j.a.T, n_cap, scan, sl->stream);
}

gm_status gm_wall_alignment_get_check(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_check_info *info,
                                      gm_wall_check_point *points, uint32_t capacity, uint32_t *n_out)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (alignment->checks.empty() || !alignment->checks[slot].have)
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_get_check: no check was enqueued on this alignment and slot");
    GMW_OK(set_device(ctx));
    const gm_wall_alignment::CheckSlot &c = alignment->checks[slot];
    if (c.own) {
        gm_wall_check_info ci;
        memset(&ci, 0, sizeof(ci));
        const gm_status st = gm_wall_map_get_check(c.own, slot, &ci, points, capacity, n_out);
        if (info && (st == GM_OK || st == GM_ERR_CAPACITY)) check_info_of_map(ci, info);
        return st;
    }
    return joint_check_result(alignment, slot, info, points, capacity, n_out);
}

gm_status gm_wall_alignment_check_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_check_params *prm, gm_wall_alignment_add_info *plan,
                                         gm_wall_alignment_check_info *info, gm_wall_check_point *points, uint32_t capacity,
                                         uint32_t *n_out, float *residual, int32_t *cell, int32_t *delta, uint8_t *cls,
                                         int32_t *element)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n_out) *n_out = 0;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_points: NULL xyz");
    if (!points && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_points: NULL points with a capacity");
    const gm_wall_check_params cp = params_or(prm, gm_wall_check_default_params);
    JointCheck j;
    memset(&j.a, 0, sizeof(j.a));
    if (!check_prm_ok(cp, j.a.T))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_points: struct_size mismatch or a parameter outside its limits");
    GMW_OK(joint_check_args(alignment, pose, cp, j));
    if (plan) *plan = j.plan;
    if (j.plan.n_sides < 2u) {
        gm_wall_check_info ci;
        memset(&ci, 0, sizeof(ci));
        const gm_status st = gm_wall_map_check_points(j.side[0], xyz, n, labels, pose, &cp, nullptr, &ci, points, capacity, n_out,
                                                      residual, cell, delta, cls);
        if (st != GM_OK && st != GM_ERR_CAPACITY) return st;
        check_note_own(alignment, 0, j);
        if (info) check_info_of_map(ci, info);
        if (element)
            for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.plan.side_element[0];
        return st;
    }
    // (the staging slot is the context's; the per-point outputs are staged in the alignment's own buffers, not a map's)
    StageCall sc{j.side[0], n, nullptr, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    if (residual) GMW_HIP(ctx, alignment->pt_res.reserve(n));
    if (cell) GMW_HIP(ctx, alignment->pt_cell.reserve(n));
    if (delta) GMW_HIP(ctx, alignment->pt_delta.reserve(n));
    if (cls) GMW_HIP(ctx, alignment->pt_cls.reserve(n));
    if (element) GMW_HIP(ctx, alignment->pt_element.reserve(n));
    hipStream_t s = sc.sl->stream;
    const uint32_t n_cap = n ? n : 1u;
    ScanState scan;
    GMW_OK(joint_check_prepare(alignment, 0, n_cap, s, scan, j.a));
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(wait_adds(j.side[k], 0, s));
    WallArgs w;
    memset(&w, 0, sizeof(w));
    GMW_OK(sc.upload(xyz, labels, w));
    j.a.pts = w.pts; j.a.labels = w.labels; j.a.n_ptr = w.n_ptr; j.a.n_host = w.n_host;
    j.a.res = residual ? alignment->pt_res.p : nullptr;
    j.a.cell = cell ? alignment->pt_cell.p : nullptr;
    j.a.delta = delta ? alignment->pt_delta.p : nullptr;
    j.a.cls = cls ? alignment->pt_cls.p : nullptr;
    j.a.element = element ? alignment->pt_element.p : nullptr;
    j.a.row_is_index = 1u;
    GMW_OK(joint_check_enqueue(alignment, 0, j, j.a.T, n_cap, scan, s));
    if (residual && n) GMW_HIP(ctx, hipMemcpyAsync(residual, alignment->pt_res.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cell && n) GMW_HIP(ctx, hipMemcpyAsync(cell, alignment->pt_cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (delta && n) GMW_HIP(ctx, hipMemcpyAsync(delta, alignment->pt_delta.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cls && n) GMW_HIP(ctx, hipMemcpyAsync(cls, alignment->pt_cls.p, (size_t)n, hipMemcpyDeviceToHost, s));
    if (element && n) GMW_HIP(ctx, hipMemcpyAsync(element, alignment->pt_element.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    return joint_check_result(alignment, 0, info, points, capacity, n_out);
}

gm_status gm_wall_alignment_add_frame_checked(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                              const gm_wall_add_checked_params *prm, gm_wall_alignment_add_info *plan)
{
    if (!alignment || !ctx) return GM_ERR_INVALID_ARG;
    const gm_wall_add_checked_params ap = params_or(prm, gm_wall_add_checked_default_params);
    WallMarkArgs mk;
    memset(&mk, 0, sizeof(mk));
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(alignment->maps[0], ctx, slot, "gm_wall_alignment_add_frame_checked",
                           [&] { return add_checked_prm_ok(ap, mk.S); }, sl));
    JointAdd j;
    GMW_OK(joint_add_args(alignment, pose, j));
    if (plan) *plan = j.plan;
    const char *none = "gm_wall_alignment_add_frame_checked: no check was enqueued on this alignment and slot for the frame the slot holds";
    if (alignment->checks.empty()) return gm_fail(ctx, GM_ERR_NOT_READY, none);
    gm_wall_alignment::CheckSlot &c = alignment->checks[slot];
    if (!c.have || c.cloud_seq != sl->cloud_seq) return gm_fail(ctx, GM_ERR_NOT_READY, none);
    if (c.own && (!c.own->checks[slot].res.have || c.own->checks[slot].scan.epoch != c.own_epoch))
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_add_frame_checked: a check on the element map itself has replaced the alignment's rows");
    GMW_OK(set_device(ctx));
    GMW_OK(alignment->add_res[slot].ensure(ctx));
    const uint32_t n_cap = sl->n_in;
    const uint64_t words = add_checked_block_words(n_cap);
    if (c.blk.cap < words || !c.h_add) GMW_OK(alignment->add_res[slot].wait(ctx));   // the slot's last checked add may still be using the old block
    GMW_HIP(ctx, c.h_add.reserve(kWallAddCheckedCounters));
    GMW_HIP(ctx, c.blk.reserve(words));
    // the rows of the alignment's last check on this slot, wherever they are staged
    const WallCheckSlot *oc = c.own ? &c.own->checks[slot] : nullptr;
    mk.rows = oc ? oc->stage.p : c.stage.p;
    mk.n_rows_ptr = (oc ? oc->ctr.p : c.ctr.p) + 9;
    mk.rows_cap = (uint32_t)std::min<uint64_t>(oc ? oc->stage.cap : c.stage.cap, n_cap);   // (a check emits at most one row per point)
    WallArgs w;
    frame_points(ctx, *sl, w);
    mk.n_ptr = w.n_ptr;
    mk.n_host = w.n_host;
    mk.skip = ap.skip;
    hipStream_t s = sl->stream;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], slot, s));
    GMW_HIP(ctx, hipMemsetAsync(c.blk.p, 0, words * 8, s));
    mk.ctr = c.blk.p;
    mk.mask = reinterpret_cast<uint32_t *>(c.blk.p + kWallAddCheckedCounters);
    launch_wall_mark(mk, mk.rows_cap, s);
    GMW_OK(joint_add_masked(alignment, j, pose, w, nullptr, nullptr, nullptr, c.blk.p, n_cap, s));
    GMW_HIP(ctx, hipMemcpyAsync(c.h_add.p, c.blk.p, kWallAddCheckedCounters * 8, hipMemcpyDeviceToHost, s));
    GMW_OK(alignment->add_res[slot].record(ctx, s));
    c.add_status = j.plan.status;
    c.S = mk.S;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) {
        j.side[k]->pending[slot] = 1;
        ++j.side[k]->frames;
    }
    return GM_OK;
}

gm_status gm_wall_alignment_get_add_checked(gm_wall_alignment *alignment, uint32_t slot, gm_wall_add_checked_info *info)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_get_add_checked: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (alignment->add_res.empty() || !alignment->add_res[slot].have)
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_get_add_checked: no checked add was enqueued on this alignment and slot");
    GMW_OK(set_device(ctx));
    GMW_OK(alignment->add_res[slot].wait(ctx));
    const gm_wall_alignment::CheckSlot &c = alignment->checks[slot];
    add_checked_fill_info(info, c.add_status, c.S, c.h_add.p);
    return GM_OK;
}

gm_status gm_wall_alignment_add_points_checked(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                               const double pose[12], const gm_wall_add_checked_params *prm,
                                               const gm_wall_check_point *rows, uint32_t n_rows, gm_wall_alignment_add_info *plan,
                                               gm_wall_add_checked_info *info, float *residual, int32_t *cell, int32_t *element)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_add_points_checked: NULL xyz");
    if (n_rows && !rows) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_add_points_checked: NULL rows");
    const gm_wall_add_checked_params ap = params_or(prm, gm_wall_add_checked_default_params);
    WallMarkArgs mk;
    memset(&mk, 0, sizeof(mk));
    if (!add_checked_prm_ok(ap, mk.S))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_add_points_checked: struct_size mismatch or a parameter outside its limits");
    JointAdd j;
    GMW_OK(joint_add_args(alignment, pose, j));
    if (plan) *plan = j.plan;
    const bool joint = j.plan.n_sides >= 2u;
    StageCall sc{j.side[0], n, nullptr, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    if (residual) GMW_HIP(ctx, alignment->pt_res.reserve(n));
    if (cell) GMW_HIP(ctx, alignment->pt_cell.reserve(n));
    if (element && joint) GMW_HIP(ctx, alignment->pt_element.reserve(n));
    WallArgs w;
    memset(&w, 0, sizeof(w));
    GMW_OK(sc.upload(xyz, labels, w));
    hipStream_t s = sc.sl->stream;
    GMW_HIP(ctx, alignment->ac_rows.reserve(n_rows ? n_rows : 1u));
    if (n_rows) GMW_HIP(ctx, hipMemcpyAsync(alignment->ac_rows.p, rows, (size_t)n_rows * sizeof(gm_wall_check_point), hipMemcpyHostToDevice, s));
    const uint64_t words = add_checked_block_words(n);
    GMW_HIP(ctx, alignment->ac_blk.reserve(words));
    GMW_HIP(ctx, hipMemsetAsync(alignment->ac_blk.p, 0, words * 8, s));
    mk.rows = alignment->ac_rows.p;
    mk.n_rows_host = n_rows;
    mk.rows_cap = n_rows;
    mk.n_host = n;
    mk.skip = ap.skip;
    mk.ctr = alignment->ac_blk.p;
    mk.mask = reinterpret_cast<uint32_t *>(alignment->ac_blk.p + kWallAddCheckedCounters);
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], 0, s));   // (the staging slot is slot 0)
    launch_wall_mark(mk, mk.rows_cap, s);
    GMW_OK(joint_add_masked(alignment, j, pose, w, residual ? alignment->pt_res.p : nullptr, cell ? alignment->pt_cell.p : nullptr,
                            element && joint ? alignment->pt_element.p : nullptr, alignment->ac_blk.p, n, s));
    unsigned long long h[kWallAddCheckedCounters];
    GMW_HIP(ctx, hipMemcpyAsync(h, alignment->ac_blk.p, sizeof(h), hipMemcpyDeviceToHost, s));
    if (residual && n) GMW_HIP(ctx, hipMemcpyAsync(residual, alignment->pt_res.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cell && n) GMW_HIP(ctx, hipMemcpyAsync(cell, alignment->pt_cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (element && joint && n) GMW_HIP(ctx, hipMemcpyAsync(element, alignment->pt_element.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks: h is filled)
    if (element && !joint)
        for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.plan.side_element[0];
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) ++j.side[k]->frames;
    if (info) add_checked_fill_info(info, j.plan.status, mk.S, h);
    return GM_OK;
}

gm_status gm_wall_alignment_info(gm_wall_alignment *alignment, gm_wall_alignment_totals *info)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_info: NULL info");
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_totals);
    info->n_elements = (uint32_t)alignment->maps.size();
    info->chainage_min = alignment->A.el.front().s_start;
    info->chainage_max = alignment->A.el.back().s_end;
    for (gm_wall_map *m : alignment->maps) {
        gm_wall_info i;
        GMW_OK(gm_wall_map_info(m, &i));
        info->n_stations += i.n_stations;
        info->frames += i.frames;
        info->mapped += i.mapped; info->outside += i.outside; info->beyond_gate += i.beyond_gate; info->plane += i.plane;
    }
    return GM_OK;
}

}  // extern "C"
