// gm_wall_alignment_locate.hip -- C ABI of the wall alignment's locate (gm_wall_alignment_locate_*; include/gm_hip.h states
// the rule).  Host logic only: the start of a locate, the kernel's arguments, the scratch of an (alignment, slot), enqueue,
// result and pose.  The kernel is k_wall_locate_joint.hip's; the object, the refusals of a plan and the other call families
// are gm_wall_alignment.hip's (gm_wall_alignment.hpp), the device-free calls gm_wall_alignment_host.hip's.
#include <stddef.h>

#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace {

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
    GMW_OK(joint_refusal(ctx, alignment_locate_start(al->A, pose, ctx->cfg.boxFilterBound, &j.start)));
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
    a.reference = lp.reference;
    a.min_count = lp.min_count;
    a.grid = WallJointGrid{(float)m0->axis.d.R, (float)m0->prm.station_length, (float)(kTwoPi / (double)m0->prm.n_sectors), (float)kTwoPi,
                           m0->prm.n_sectors};
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

// the scratch of (alignment, slot); a new ticket is zeroed on `s`
gm_status joint_locate_prepare(gm_wall_alignment *al, uint32_t slot, hipStream_t s, WallLocateJointArgs &a)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::LocateSlot &l = al->locates[slot];
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
    gm_wall_alignment::LocateSlot &l = al->locates[slot];
    l.start = j.start;
    l.own = j.own;
    l.have = true;
}

}  // namespace

extern "C" {

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
    joint_points(j.a, w);
    return joint_locate_enqueue(alignment, slot, j, sl->stream);
}

gm_status gm_wall_alignment_get_locate(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_locate_info *info)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_get_locate: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!alignment->locates[slot].have)
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
    StageCall sc{j.side[0], n, alignment->pt, residual, cell, nullptr, nullptr, element};
    GMW_OK(sc.open());
    // (the kernel writes all three outputs or none, into buffers that are there for no point too)
    const uint32_t all = kPtRes | kPtCell | kPtElement;
    if (residual || cell || element) GMW_OK(alignment->pt.reserve(ctx, n ? n : 1u, all, all));
    hipStream_t s = sc.sl->stream;
    GMW_OK(joint_locate_prepare(alignment, 0, s, j.a));
    for (uint32_t k = 0; k < j.start.add.n_sides; ++k) GMW_OK(wait_adds(j.side[k], 0, s));
    GMW_OK(joint_upload(sc, xyz, labels, j.a));
    GMW_OK(joint_locate_enqueue(alignment, 0, j, s));
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    return joint_locate_result(alignment, 0, info);
}

}  // extern "C"
