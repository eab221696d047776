// gm_wall_alignment_check.hip -- C ABI of the wall alignment's check (gm_wall_alignment_check_*) and of the add less its
// selected rows (gm_wall_alignment_add_*_checked; include/gm_hip.h states the rules).  Host logic only: the check's
// arguments over the sides of a plan, the scratch of an (alignment, slot), enqueue and result; the masked add of a plan.
// The kernels are k_wall_check_joint.hip's, k_wall_joint.hip's masked instantiation and k_wall_add_checked.hip's mark; the
// object, the plan, its sides and the add's arguments are gm_wall_alignment.hip's (gm_wall_alignment.hpp), the locate is
// gm_wall_alignment_locate.hip, the device-free calls are in gm_wall_alignment_host.hip.
#include <stddef.h>

#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace {

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
    GMW_OK(joint_plan(al, pose, j.plan, j.side));
    if (j.plan.n_sides < 2u) return GM_OK;   // (the map's own check computes its frame)
    WallCheckJointArgs &a = j.a;
    a.n_sides = j.plan.n_sides;
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    GMW_OK(joint_sides(j.side, pose, j.plan, a.side, a.grid, a.planes));
    a.gate = (float)cp.gate;   // the check's own, rounded once
    return GM_OK;
}

// The scratch of (alignment, slot) for a check of up to n_cap points, and everything a launch on `s` needs before it:
// zeroed counters, a fresh scan state, the buffers in `a`.
gm_status joint_check_prepare(gm_wall_alignment *al, uint32_t slot, uint32_t n_cap, hipStream_t s, ScanState &st, WallCheckJointArgs &a)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::CheckSlot &c = al->checks[slot];
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
    gm_wall_alignment::CheckSlot &c = al->checks[slot];
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
// masked kernel under its own per-add frame.  pts: the points, and the stage call's residual and cell
gm_status joint_add_masked(gm_wall_alignment *al, JointAdd &j, const double pose[12], const WallArgs &pts, int32_t *element,
                           unsigned long long *blk, uint32_t n_cap, hipStream_t s)
{
    const unsigned long long *mask = blk + kWallAddCheckedCounters;
    if (j.plan.n_sides >= 2u) {
        joint_points(j.ja, pts);
        j.ja.res = pts.res; j.ja.cell = pts.cell; j.ja.element = element;
        launch_wall_add_joint_masked(j.ja, mask, blk, n_cap, j.side[0]->points_per_block, s);
    } else {
        gm_wall_map *m = j.side[0];
        WallArgs w;
        WallAxis ax;
        GMW_OK(add_frame_args(m, pose, nullptr, w, nullptr, &ax));
        w.pts = pts.pts; w.labels = pts.labels; w.n_ptr = pts.n_ptr; w.n_host = pts.n_host;
        w.res = pts.res; w.cell = pts.cell;
        launch_wall_add(w, ax, mask, blk, n_cap, m->points_per_block, s);
    }
    GMW_HIP(al->ctx, hipGetLastError());
    return GM_OK;
}

}  // namespace

extern "C" {

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
    joint_points(j.a, w);
    return joint_check_enqueue(alignment, slot, j, j.a.T, n_cap, scan, sl->stream);
}

gm_status gm_wall_alignment_get_check(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_check_info *info,
                                      gm_wall_check_point *points, uint32_t capacity, uint32_t *n_out)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!alignment->checks[slot].have)
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
    StageCall sc{j.side[0], n, alignment->pt, residual, cell, delta, cls, element};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    const uint32_t n_cap = n ? n : 1u;
    ScanState scan;
    GMW_OK(joint_check_prepare(alignment, 0, n_cap, s, scan, j.a));
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(wait_adds(j.side[k], 0, s));
    GMW_OK(joint_upload(sc, xyz, labels, j.a));
    j.a.delta = alignment->pt.dev_delta();
    j.a.cls = alignment->pt.dev_cls();
    j.a.row_is_index = 1u;
    GMW_OK(joint_check_enqueue(alignment, 0, j, j.a.T, n_cap, scan, s));
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
    w.res = nullptr;   // (the frame path has no per-point outputs)
    w.cell = nullptr;
    mk.n_ptr = w.n_ptr;
    mk.n_host = w.n_host;
    mk.skip = ap.skip;
    hipStream_t s = sl->stream;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], slot, s));
    GMW_HIP(ctx, hipMemsetAsync(c.blk.p, 0, words * 8, s));
    mk.ctr = c.blk.p;
    mk.mask = reinterpret_cast<uint32_t *>(c.blk.p + kWallAddCheckedCounters);
    launch_wall_mark(mk, mk.rows_cap, s);
    GMW_OK(joint_add_masked(alignment, j, pose, w, nullptr, c.blk.p, n_cap, s));
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
    if (!alignment->add_res[slot].have)
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
    // (the one side's element is filled on the host)
    StageCall sc{j.side[0], n, alignment->pt, residual, cell, nullptr, nullptr, joint ? element : nullptr};
    GMW_OK(sc.open());
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
    GMW_OK(joint_add_masked(alignment, j, pose, w, alignment->pt.dev_element(), alignment->ac_blk.p, n, s));
    unsigned long long h[kWallAddCheckedCounters];
    GMW_HIP(ctx, hipMemcpyAsync(h, alignment->ac_blk.p, sizeof(h), hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks: h is filled)
    if (element && !joint)
        for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.plan.side_element[0];
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) ++j.side[k]->frames;
    if (info) add_checked_fill_info(info, j.plan.status, mk.S, h);
    return GM_OK;
}

}  // extern "C"
