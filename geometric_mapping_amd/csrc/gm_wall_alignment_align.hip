// gm_wall_alignment_align.hip -- C ABI of the wall alignment's align (gm_wall_alignment_align_*; include/gm_hip.h states the
// rule).  Host logic only: the plan of an align and its kernels' arguments over the sides and the pieces, the scratch of
// an (alignment, slot), enqueue and result.  The kernels are k_wall_align_joint.hip's and k_wall_align.hip's score kernel;
// the object, the plan of an add and its sides are gm_wall_alignment.hip's (gm_wall_alignment.hpp), the device-free calls
// (the plan, the selection and the pose) gm_wall_alignment_host.hip's.
#include <stddef.h>

#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace {

// The plan of an align under `pose`, and for a plan that is not an element map's own the kernels' arguments but for the
// points and the scratch.  own: the element map whose own align the call is.
struct JointAlign {
    gm_wall_alignment_align_plan_info plan;
    WallAlignJointArgs bin;
    WallAlignJointValuesArgs val;
    WallAlignArgs score;               // what k_wall_align_score reads: n_sectors, P, A, B, rows, C, f, m, table
    gm_wall_map *own = nullptr;
    gm_wall_map *side[GM_WALL_JOINT_MAX_SIDES] = {};
    gm_wall_map *piece[GM_WALL_ALIGN_MAX_PIECES] = {};
};

gm_status joint_align_args(gm_wall_alignment *al, const double pose[12], const gm_wall_align_params &ap, JointAlign &j)
{
    gm_ctx *ctx = al->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment: NULL pose");
    const gm_status st = alignment_align_plan(al->A, pose, ctx->cfg.boxFilterBound, ap, &j.plan);
    if (st == GM_ERR_UNSUPPORTED && j.plan.add.n_sides)   // (the add's plan was accepted: the pieces were too many)
        return gm_fail(ctx, st, "gm_wall_alignment align: the map image meets more than GM_WALL_ALIGN_MAX_PIECES elements");
    GMW_OK(joint_refusal(ctx, st));
    const gm_wall_alignment_add_info &pl = j.plan.add;
    for (uint32_t k = 0; k < pl.n_sides; ++k) j.side[k] = al->maps[pl.side_element[k]];
    for (uint32_t k = 0; k < j.plan.n_pieces; ++k) j.piece[k] = al->maps[j.plan.piece[k].element];
    if (j.plan.own) {
        j.own = j.side[0];
        return GM_OK;
    }
    memset(&j.bin, 0, sizeof(j.bin));
    memset(&j.val, 0, sizeof(j.val));
    memset(&j.score, 0, sizeof(j.score));
    WallAlignJointArgs &b = j.bin;
    b.n_sides = pl.n_sides;
    b.P = ap.half_patch_stations;
    GMW_OK(joint_sides(j.side, pose, pl, b.side, b.grid, b.planes));
    b.gate = (float)ap.gate;   // the align's own, rounded once
    for (uint32_t k = 0; k < pl.n_sides; ++k) b.row0[k] = j.plan.row0[k];
    WallAlignJointValuesArgs &v = j.val;
    v.P = ap.half_patch_stations;
    v.A = ap.max_station_shift;
    v.n_sectors = b.grid.n_sectors;
    v.min_count = ap.min_count;
    v.min_frame_count = ap.min_frame_count;
    v.n_pieces = j.plan.n_pieces;
    v.g0 = (j.plan.anchor_global - (int64_t)v.P) - (int64_t)v.A;
    for (uint32_t k = 0; k < v.n_pieces; ++k) {
        v.piece[k].table = j.piece[k]->table;
        v.piece[k].first_row = j.plan.piece[k].first_row;
        v.piece[k].n_stations = j.plan.piece[k].n_stations;
    }
    WallAlignArgs &s = j.score;
    s.w.n_sectors = b.grid.n_sectors;
    s.P = v.P;
    s.A = v.A;
    s.B = ap.max_sector_shift;
    s.C = (long long)rint(ap.clip * 1048576.0);
    const gm_wall_map *m0 = j.side[0];
    const uint32_t rows = m0->align_rows ? m0->align_rows : wall_align_default_rows(m0->prm.n_sectors);
    s.rows = std::min(rows, 2u * s.P);
    return GM_OK;
}

// the scratch of (alignment, slot), laid out by this align's counts and zeroed on `s`
gm_status joint_align_prepare(gm_wall_alignment *al, uint32_t slot, hipStream_t s, JointAlign &j)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::AlignSlot &l = al->aligns[slot];
    PendingResult &res = al->align_res[slot];
    GMW_OK(res.ensure(ctx));
    const uint32_t nsec = j.val.n_sectors;
    const uint64_t nsh = (uint64_t)(2u * j.score.A + 1u) * (2u * j.score.B + 1u);
    const uint64_t pc = 2ull * j.val.P * nsec, mc = (2ull * j.val.P + 2ull * j.val.A) * nsec;
    const uint64_t res_bytes = 8ull * kWallAlignJointCounters + nsh * sizeof(gm_wall_align_score), zero_bytes = res_bytes + pc * 12;
    if (l.zeroed.cap < zero_bytes || l.f.cap < pc || l.m.cap < mc || l.h_res.cap < res_bytes)
        GMW_OK(res.wait(ctx));                       // the slot's last align may still be using the old blocks
    if (l.h_res.cap < res_bytes) l.have = false;     // (its result goes with the block)
    GMW_HIP(ctx, l.zeroed.reserve(zero_bytes));
    GMW_HIP(ctx, l.f.reserve(pc));
    GMW_HIP(ctx, l.m.reserve(mc));
    GMW_HIP(ctx, l.h_res.reserve(res_bytes));
    Carve cv{l.zeroed.p};
    unsigned long long *ctr = cv.take<unsigned long long>(kWallAlignJointCounters);
    gm_wall_align_score *table = cv.take<gm_wall_align_score>(nsh);
    unsigned long long *p_sum = cv.take<unsigned long long>(pc);
    uint32_t *p_cnt = cv.take<uint32_t>(pc);
    j.bin.ctr = ctr; j.bin.p_sum = p_sum; j.bin.p_cnt = p_cnt;
    j.val.ctr = ctr; j.val.p_sum = p_sum; j.val.p_cnt = p_cnt; j.val.f = l.f.p; j.val.m = l.m.p;
    j.score.table = table; j.score.f = l.f.p; j.score.m = l.m.p;
    GMW_HIP(ctx, hipMemsetAsync(l.zeroed.p, 0, zero_bytes, s));
    return GM_OK;
}

// the three launches (the maps are read behind the wait on the adds of every piece's map), the copy of the result and the
// event behind them
gm_status joint_align_enqueue(gm_wall_alignment *al, uint32_t slot, const JointAlign &j, uint32_t n_cap, const gm_wall_align_params &ap,
                              const double pose[12], hipStream_t s)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::AlignSlot &l = al->aligns[slot];
    const uint32_t nsh = (2u * j.score.A + 1u) * (2u * j.score.B + 1u);
    launch_wall_align_bin_joint(j.bin, n_cap, s);
    GMW_HIP(ctx, hipGetLastError());
    for (uint32_t k = 0; k < j.plan.n_pieces; ++k) GMW_OK(wait_adds(j.piece[k], slot, s));
    launch_wall_align_values_joint(j.val, s);
    launch_wall_align_score(j.score, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_res.p, l.zeroed.p, 8 * kWallAlignJointCounters + (size_t)nsh * sizeof(gm_wall_align_score),
                                hipMemcpyDeviceToHost, s));
    GMW_OK(al->align_res[slot].record(ctx, s));
    l.prm = ap;
    memcpy(l.pose, pose, sizeof(l.pose));
    l.plan = j.plan;
    l.n_shifts = nsh;
    l.own = nullptr;
    l.have = true;
    return GM_OK;
}

// the slot's last align was the element map's own
void align_note_own(gm_wall_alignment *al, uint32_t slot, const JointAlign &j)
{
    gm_wall_alignment::AlignSlot &l = al->aligns[slot];
    l.plan = j.plan;
    l.own = j.own;
    l.have = true;
}

// an element map's own align as the alignment's info: the shared fields byte for byte, its classes as side 0's
void align_info_of_map(const gm_wall_alignment_align_plan_info &plan, const gm_wall_align_info &ai, gm_wall_alignment_align_info *info)
{
    static_assert(offsetof(gm_wall_alignment_align_info, element) == sizeof(gm_wall_align_info), "the shared head");
    static_assert(offsetof(gm_wall_alignment_align_info, pose) == offsetof(gm_wall_align_info, pose) &&
                      offsetof(gm_wall_alignment_align_info, anchor_station) == offsetof(gm_wall_align_info, anchor_station) &&
                      offsetof(gm_wall_alignment_align_info, distinction) == offsetof(gm_wall_align_info, distinction),
                  "the shared head");
    memset(info, 0, sizeof(*info));
    memcpy(info, &ai, sizeof(ai));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_align_info);
    info->element = plan.add.element;
    info->n_sides = 1u;
    info->chainage = plan.add.chainage;
    info->anchor_global = plan.anchor_global;
    info->side_class[0][0] = ai.plane; info->side_class[0][1] = ai.beyond_gate;
    info->side_class[0][2] = ai.outside_patch; info->side_class[0][3] = ai.binned;
    info->plan = plan.add;
}

// the result of (alignment, slot) of an align that is not an element map's own, waited for: the device's table and counts,
// the selection and the pose in fp64
gm_status joint_align_result(gm_wall_alignment *al, uint32_t slot, gm_wall_alignment_align_info *info, gm_wall_align_score *scores,
                             uint32_t capacity, uint32_t *n_out)
{
    gm_ctx *ctx = al->ctx;
    gm_wall_alignment::AlignSlot &l = al->aligns[slot];
    GMW_OK(al->align_res[slot].wait(ctx));
    const unsigned long long *h = reinterpret_cast<const unsigned long long *>(l.h_res.p);
    const gm_wall_align_score *table = reinterpret_cast<const gm_wall_align_score *>(l.h_res.p + 8 * kWallAlignJointCounters);
    if (n_out) *n_out = l.n_shifts;
    if (info) {
        (void)alignment_align_select(al->A, l.pose, l.prm, l.plan, table, info);   // (the pose was accepted at the enqueue)
        info->plane = (uint32_t)h[0];
        info->beyond_gate = (uint32_t)h[1];
        info->outside_patch = (uint32_t)h[2];
        info->binned = (uint32_t)h[3];
        info->n_points = (uint32_t)h[4];
        info->patch_cells_usable = (uint32_t)h[5];
        for (uint32_t k = 0; k < l.plan.add.n_sides; ++k)
            for (int q = 0; q < 4; ++q) info->side_class[k][q] = (uint32_t)h[kWallAlignCounters + k * 4 + q];
    }
    if (!scores && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment align: NULL scores with a capacity");
    if (!scores) return GM_OK;   // a count query
    if (l.n_shifts > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_alignment align: score buffer too small");
    memcpy(scores, table, (size_t)l.n_shifts * sizeof(gm_wall_align_score));
    return GM_OK;
}

}  // namespace

extern "C" {

gm_status gm_wall_alignment_align_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_align_params *prm, gm_wall_alignment_align_plan_info *plan)
{
    if (!alignment || !ctx) return GM_ERR_INVALID_ARG;
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(alignment->maps[0], ctx, slot, "gm_wall_alignment_align_frame",
                           [&] { return align_prm_ok(ap, alignment->maps[0]->prm.n_sectors); }, sl));
    JointAlign j;
    GMW_OK(joint_align_args(alignment, pose, ap, j));
    if (plan) *plan = j.plan;
    if (j.own) {
        GMW_OK(gm_wall_map_align_frame(j.own, ctx, slot, pose, &ap, nullptr));
        align_note_own(alignment, slot, j);
        return GM_OK;
    }
    GMW_OK(set_device(ctx));
    GMW_OK(joint_align_prepare(alignment, slot, sl->stream, j));
    WallArgs w;
    frame_points(ctx, *sl, w);
    joint_points(j.bin, w);
    return joint_align_enqueue(alignment, slot, j, sl->n_in ? sl->n_in : 1u, ap, pose, sl->stream);
}

gm_status gm_wall_alignment_get_align(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_align_info *info,
                                      gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!alignment->aligns[slot].have)
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_get_align: no align was enqueued on this alignment and slot");
    GMW_OK(set_device(ctx));
    const gm_wall_alignment::AlignSlot &l = alignment->aligns[slot];
    if (l.own) {
        gm_wall_align_info ai;
        memset(&ai, 0, sizeof(ai));
        const gm_status st = gm_wall_map_get_align(l.own, slot, &ai, scores, capacity, n_out);
        if (info && (st == GM_OK || st == GM_ERR_CAPACITY)) align_info_of_map(l.plan, ai, info);
        return st;
    }
    return joint_align_result(alignment, slot, info, scores, capacity, n_out);
}

gm_status gm_wall_alignment_align_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_align_params *prm,
                                         gm_wall_alignment_align_plan_info *plan, gm_wall_alignment_align_info *info,
                                         gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out, float *residual,
                                         int32_t *cell, int32_t *element)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    if (n_out) *n_out = 0;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_align_points: NULL xyz");
    if (!scores && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_align_points: NULL scores with a capacity");
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    if (!align_prm_ok(ap, alignment->maps[0]->prm.n_sectors))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_align_points: struct_size mismatch or a parameter outside its limits");
    JointAlign j;
    GMW_OK(joint_align_args(alignment, pose, ap, j));
    if (plan) *plan = j.plan;
    if (j.own) {
        gm_wall_align_info ai;
        memset(&ai, 0, sizeof(ai));
        const gm_status st = gm_wall_map_align_points(j.own, xyz, n, labels, pose, &ap, nullptr, &ai, scores, capacity, n_out, residual, cell);
        if (st != GM_OK && st != GM_ERR_CAPACITY) return st;
        align_note_own(alignment, 0, j);
        if (info) align_info_of_map(j.plan, ai, info);
        if (element)
            for (uint32_t i = 0; i < n; ++i) element[i] = (int32_t)j.plan.add.side_element[0];
        return st;
    }
    // (the staging slot is the context's; the per-point outputs are staged in the alignment's own buffers, not a map's)
    StageCall sc{j.side[0], n, alignment->pt, residual, cell, nullptr, nullptr, element};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    GMW_OK(joint_align_prepare(alignment, 0, s, j));
    GMW_OK(joint_upload(sc, xyz, labels, j.bin));
    GMW_OK(joint_align_enqueue(alignment, 0, j, n ? n : 1u, ap, pose, s));
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    return joint_align_result(alignment, 0, info, scores, capacity, n_out);
}

}  // extern "C"
