// gm_wall_slot.hip -- C ABI of the wall map's per-(map, slot) calls (gm_wall_map_check_*, _locate_*, _align_*,
// gm_wall_map_check_objects / gm_wall_check_objects; include/gm_hip.h states the rules).  Each enqueues on a slot's stream
// and leaves a PendingResult (gm_wall_map.hpp) the host reads later.  Kernels are in k_wall_check.hip, k_wall_locate.hip,
// k_wall_align.hip and k_wall_objects.hip.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

gm_status wait_adds(gm_wall_map *m, uint32_t slot, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    for (uint32_t i = 0; i < ctx->n_slots; ++i) {
        if (i == slot || !m->pending[i]) continue;
        if (!m->adds[i]) GMW_HIP(ctx, hipEventCreateWithFlags(&m->adds[i], hipEventDisableTiming));
        GMW_HIP(ctx, hipEventRecord(m->adds[i], ctx->slots[i].stream));
        GMW_HIP(ctx, hipStreamWaitEvent(s, m->adds[i], 0));
    }
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

namespace {

// ---- gm_wall_map_check_* ----

// The scratch of (map, slot) for a check of up to n_cap points, and everything a launch on `s` needs before it: zeroed
// counters, a fresh scan state, the buffers in `a`.
gm_status check_prepare(gm_wall_map *m, uint32_t slot, uint32_t n_cap, hipStream_t s, ScanState &st, WallCheckArgs &a)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    GMW_OK(c.res.ensure(ctx));
    GMW_HIP(ctx, c.ctr.reserve(kWallCheckCounters));
    GMW_HIP(ctx, c.h_ctr.reserve(kWallCheckCounters));
    if (c.stage.cap < n_cap || !c.scan.holds(n_cap)) {
        GMW_OK(c.res.wait(ctx));   // the slot's last check may still be writing the old blocks
        GMW_OK(m->add_checks[slot].res.wait(ctx));   // ... and a checked add behind it still reading the rows
        c.res.have = false;        // (its rows go with the block)
    }
    GMW_HIP(ctx, c.stage.reserve(n_cap));
    GMW_OK(c.scan.reserve(ctx, n_cap, s));
    st = c.scan.next(s);
    a.out = c.stage.p;
    a.ctr = c.ctr.p;
    GMW_HIP(ctx, hipMemsetAsync(c.ctr.p, 0, kWallCheckCounters * 8, s));
    return GM_OK;
}

// the launch, the copy of its counters and the event behind both
gm_status check_enqueue(gm_wall_map *m, uint32_t slot, const WallCheckArgs &a, const WallAxis &ax, uint32_t n_cap, const ScanState &st,
                        hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    launch_wall_check(a, ax, n_cap, st, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(c.h_ctr, c.ctr.p, kWallCheckCounters * 8, hipMemcpyDeviceToHost, s));
    GMW_OK(c.res.record(ctx, s));
    c.status = m->axis.d.status;
    c.T = a.T;
    c.anchor = a.w.anchor;
    c.cloud_seq = ctx->slots[slot].cloud_seq;
    return GM_OK;
}

// the result of (map, slot), waited for
gm_status check_result(gm_wall_map *m, uint32_t slot, gm_wall_check_info *info, gm_wall_check_point *points, uint32_t capacity,
                       uint32_t *n_out)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    GMW_OK(c.res.wait(ctx));
    const unsigned long long *h = c.h_ctr;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->struct_size = (uint32_t)sizeof(gm_wall_check_info);
        info->status = c.status;
        info->threshold_q = c.T;
        info->n_points = (uint32_t)h[10];
        info->plane = (uint32_t)h[GM_WALL_CHECK_CLS_PLANE];
        info->beyond_gate = (uint32_t)h[GM_WALL_CHECK_CLS_BEYOND_GATE];
        info->outside = (uint32_t)h[GM_WALL_CHECK_CLS_OUTSIDE];
        info->unsurveyed = (uint32_t)h[GM_WALL_CHECK_CLS_UNSURVEYED];
        info->unchanged = (uint32_t)h[GM_WALL_CHECK_CLS_UNCHANGED];
        info->changed_pos = (uint32_t)h[GM_WALL_CHECK_CLS_CHANGED_POS];
        info->changed_neg = (uint32_t)h[GM_WALL_CHECK_CLS_CHANGED_NEG];
        info->peak_pos = (int64_t)h[7];
        info->peak_neg = (int64_t)(0ull - h[8]);
    }
    const uint32_t got = (uint32_t)h[9];
    if (n_out) *n_out = got;
    if (!points && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map check: NULL points with a capacity");
    if (!points) return GM_OK;   // a count query
    if (got > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map check: point buffer too small");
    if (got) {   // on the map's own stream: the slot's may be busy with the next frame
        GMW_HIP(ctx, hipMemcpyAsync(points, c.stage.p, (size_t)got * sizeof(gm_wall_check_point), hipMemcpyDeviceToHost, m->stream));
        GMW_HIP(ctx, hipStreamSynchronize(m->stream));
    }
    return GM_OK;
}

// ---- gm_wall_map_locate_* ----

// the start of include/gm_hip.h: the add's frame before the rounding (f: with the o_f the result is composed from), and s0
gm_status locate_args(gm_wall_map *m, const double pose[12], const gm_wall_locate_params &lp, WallLocateArgs &a, WallFrame64 &f)
{
    memset(&a, 0, sizeof(a));
    GMW_OK(add_frame_args(m, pose, nullptr, a.w, &f));
    a.reference = lp.reference;
    a.min_count = lp.min_count;
    a.gate = lp.gate;
    for (int k = 0; k < 3; ++k) { a.c0[k] = f.c[k]; a.d0[k] = f.d[k]; a.u0[k] = f.u[k]; a.v0[k] = f.v[k]; }
    a.s0 = -dot(f.c, f.d);
    return GM_OK;
}

// the scratch of (map, slot); a new ticket is zeroed on `s`
gm_status locate_prepare(gm_wall_map *m, uint32_t slot, hipStream_t s, WallLocateArgs &a)
{
    gm_ctx *ctx = m->ctx;
    WallLocateSlot &l = m->locates[slot];
    GMW_OK(l.res.ensure(ctx));
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

// the three passes, the copy of the result and the event behind them; the slot keeps what the result is composed from
gm_status locate_enqueue(gm_wall_map *m, uint32_t slot, const WallLocateArgs &a, const WallFrame64 &f, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    WallLocateSlot &l = m->locates[slot];
    launch_wall_locate(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_work.p, l.work.p, sizeof(WallLocateWork), hipMemcpyDeviceToHost, s));
    GMW_OK(l.res.record(ctx, s));
    l.anchor = a.w.anchor;
    for (int k = 0; k < 3; ++k) l.of[k] = f.of[k];
    return GM_OK;
}

// the result of (map, slot), waited for: the device's record, and the pose composed in fp64
gm_status locate_result(gm_wall_map *m, uint32_t slot, gm_wall_locate_info *info)
{
    WallLocateSlot &l = m->locates[slot];
    GMW_OK(l.res.wait(m->ctx));
    const WallLocateWork &wk = *l.h_work.p;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_locate_info);
    info->status = wk.status;
    info->passes = wk.passes;
    info->n_points = wk.n_points;
    info->anchor_station = l.anchor;
    for (int k = 0; k < GM_LOCATE_PASSES; ++k) info->pass[k] = wk.pass[k];
    if (wk.status & GM_LOCATE_FAILED_MASK) {
        const double nan = __builtin_nan("");
        for (int k = 0; k < 12; ++k) info->pose[k] = nan;
        info->lateral[0] = info->lateral[1] = info->tilt[0] = info->tilt[1] = nan;
        return GM_OK;
    }
    if (wk.last_step > GM_FIT_STEP_BOUND) info->status |= GM_LOCATE_NOT_CONVERGED;
    for (int k = 0; k < 2; ++k) { info->lateral[k] = wk.lateral[k]; info->tilt[k] = wk.tilt[k]; }
    const DesignFrame &d = m->axis.d;
    for (int r = 0; r < 3; ++r) {   // Rm' = a d^T + u u'^T + v v'^T, tr' = o_f - Rm' c
        double rc = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double e = d.a[r] * wk.d[c] + d.u[r] * wk.u[c] + d.v[r] * wk.v[c];
            info->pose[4 * r + c] = e;
            rc += e * wk.c[c];
        }
        info->pose[4 * r + 3] = l.of[r] - rc;
    }
    return GM_OK;
}

// ---- gm_wall_map_align_* ----

// the kernels' arguments but for the buffers
gm_status align_args(gm_wall_map *m, const double pose[12], const gm_wall_align_params &ap, gm_wall_add_info *add_info, WallAlignArgs &a)
{
    memset(&a, 0, sizeof(a));
    GMW_OK(add_frame_args(m, pose, add_info, a.w));
    a.w.gate = (float)ap.gate;
    if (add_info) add_info->gate = a.w.gate;
    a.P = ap.half_patch_stations;
    a.A = ap.max_station_shift;
    a.B = ap.max_sector_shift;
    a.min_count = ap.min_count;
    a.min_frame_count = ap.min_frame_count;
    a.C = (long long)rint(ap.clip * 1048576.0);
    const uint32_t rows = m->align_rows ? m->align_rows : wall_align_default_rows(m->prm.n_sectors);
    a.rows = std::min(rows, 2u * a.P);
    return GM_OK;
}

// the scratch of (map, slot), laid out by this align's counts and zeroed on `s`
gm_status align_prepare(gm_wall_map *m, uint32_t slot, hipStream_t s, WallAlignArgs &a)
{
    gm_ctx *ctx = m->ctx;
    WallAlignSlot &l = m->aligns[slot];
    GMW_OK(l.res.ensure(ctx));
    const uint64_t nsh = (uint64_t)(2u * a.A + 1u) * (2u * a.B + 1u);
    const uint64_t pc = 2ull * a.P * m->prm.n_sectors, mc = (2ull * a.P + 2ull * a.A) * m->prm.n_sectors;
    const uint64_t res_bytes = 8ull * kWallAlignCounters + nsh * sizeof(gm_wall_align_score), zero_bytes = res_bytes + pc * 12;
    if (l.zeroed.cap < zero_bytes || l.f.cap < pc || l.m.cap < mc || l.h_res.cap < res_bytes)
        GMW_OK(l.res.wait(ctx));                         // the slot's last align may still be using the old blocks
    if (l.h_res.cap < res_bytes) l.res.have = false;     // (its result goes with the block)
    GMW_HIP(ctx, l.zeroed.reserve(zero_bytes));
    GMW_HIP(ctx, l.f.reserve(pc));
    GMW_HIP(ctx, l.m.reserve(mc));
    GMW_HIP(ctx, l.h_res.reserve(res_bytes));
    Carve cv{l.zeroed.p};
    a.ctr = cv.take<unsigned long long>(kWallAlignCounters);
    a.table = cv.take<gm_wall_align_score>(nsh);
    a.p_sum = cv.take<unsigned long long>(pc);
    a.p_cnt = cv.take<uint32_t>(pc);
    a.f = l.f.p;
    a.m = l.m.p;
    GMW_HIP(ctx, hipMemsetAsync(l.zeroed.p, 0, zero_bytes, s));
    return GM_OK;
}

// the three launches (the map is read behind the wait on the adds), the copy of the result and the event behind them
gm_status align_enqueue(gm_wall_map *m, uint32_t slot, const WallAlignArgs &a, uint32_t n_cap, const gm_wall_align_params &ap,
                        const double pose[12], hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    WallAlignSlot &l = m->aligns[slot];
    const uint32_t nsh = (2u * a.A + 1u) * (2u * a.B + 1u);
    launch_wall_align_bin(a, n_cap, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_OK(wait_adds(m, slot, s));
    launch_wall_align_values(a, s);
    launch_wall_align_score(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_res.p, l.zeroed.p, 8 * kWallAlignCounters + (size_t)nsh * sizeof(gm_wall_align_score),
                                hipMemcpyDeviceToHost, s));
    GMW_OK(l.res.record(ctx, s));
    l.prm = ap;
    memcpy(l.pose, pose, sizeof(l.pose));
    l.n_shifts = nsh;
    return GM_OK;
}

// the result of (map, slot), waited for: the device's table and counts, the selection and the pose in fp64
gm_status align_result(gm_wall_map *m, uint32_t slot, gm_wall_align_info *info, gm_wall_align_score *scores, uint32_t capacity,
                       uint32_t *n_out)
{
    gm_ctx *ctx = m->ctx;
    WallAlignSlot &l = m->aligns[slot];
    GMW_OK(l.res.wait(ctx));
    const unsigned long long *h = reinterpret_cast<const unsigned long long *>(l.h_res.p);
    const gm_wall_align_score *table = reinterpret_cast<const gm_wall_align_score *>(l.h_res.p + 8 * kWallAlignCounters);
    if (n_out) *n_out = l.n_shifts;
    if (info) {
        double Rm[3][3], tr[3];
        (void)pose_split(l.pose, Rm, tr);   // (accepted at the enqueue)
        align_select(m->axis.d, m->prm, l.prm, Rm, tr, table, info);
        info->plane = (uint32_t)h[0];
        info->beyond_gate = (uint32_t)h[1];
        info->outside_patch = (uint32_t)h[2];
        info->binned = (uint32_t)h[3];
        info->n_points = (uint32_t)h[4];
        info->patch_cells_usable = (uint32_t)h[5];
    }
    if (!scores && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map align: NULL scores with a capacity");
    if (!scores) return GM_OK;   // a count query
    if (l.n_shifts > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map align: score buffer too small");
    memcpy(scores, table, (size_t)l.n_shifts * sizeof(gm_wall_align_score));
    return GM_OK;
}

}  // namespace

namespace gm {
namespace wall {

// ---- gm_wall_map_check_objects / gm_wall_check_objects, gm_wall_alignment_check_objects / _rows ----

void ObjectScratch::read_tile_env()
{
    if (const char *e = getenv("GM_WALL_OBJECT_TILE")) {
        unsigned r = 0, c = 0;
        if (sscanf(e, "%ux%u", &r, &c) == 2 && r >= 1u && c >= 1u && (uint64_t)r * c <= kWallObjectTileBlocks) {
            tr = r;
            tc = c;
        }
    }
}

gm_status objects_run(gm_ctx *ctx, hipStream_t s, ObjectScratch &ob, const ObjectGrid &grid, const gm_wall_check_point *d_rows,
                      uint32_t n_rows, uint32_t rejected_if_empty, const uint32_t *side_rows_if_empty, const gm_wall_object_params &op,
                      const ObjectWindow &win, gm_wall_objects_info *info, uint32_t *side_rows, gm_wall_object *objects,
                      uint32_t capacity, uint32_t *n_out, int32_t *object_of_row, const char *who)
{
    memset(&info->n_rows, 0, sizeof(*info) - offsetof(gm_wall_objects_info, n_rows));
    info->n_rows = n_rows;
    info->station0 = win.station0;
    info->n_stations = win.n_stations;
    info->blocks_stations = win.nJ;
    info->blocks_sectors = win.NK;
    if (side_rows) std::fill(side_rows, side_rows + GM_WALL_JOINT_MAX_SIDES, 0u);
    if (!n_rows || !win.nJ) {   // nothing to launch
        info->rejected = rejected_if_empty;
        info->outside_window = n_rows - rejected_if_empty;
        if (side_rows && side_rows_if_empty) std::copy(side_rows_if_empty, side_rows_if_empty + GM_WALL_JOINT_MAX_SIDES, side_rows);
        if (object_of_row) std::fill(object_of_row, object_of_row + n_rows, -1);
        return GM_OK;
    }
    const uint64_t NB = (uint64_t)win.nJ * win.NK, pairs = 2u * NB;
    GMW_HIP(ctx, ob.blocks.reserve(3u * pairs));
    GMW_HIP(ctx, ob.ctr.reserve(kWallObjectCounters));
    if (object_of_row) GMW_HIP(ctx, ob.of_row.reserve(n_rows));
    WallObjectArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.nsec = grid.nsec;
    a.cells = grid.cells;   // <= GM_WALL_MAX_CELLS
    a.sides = grid.sides;
    a.bs = op.block_stations; a.bk = op.block_sectors; a.NK = win.NK;
    a.J0 = win.J0; a.nJ = win.nJ; a.NB = (uint32_t)NB;
    a.ts = ob.tr; a.tk = ob.tc;
    a.tiles_s = (a.nJ + a.ts - 1u) / a.ts;
    a.tiles_k = (a.NK + a.tk - 1u) / a.tk;
    a.conn8 = op.connectivity == 8u ? 1u : 0u;
    a.min_block_points = op.min_block_points;
    a.min_points = op.min_points;
    a.cnt = ob.blocks.p;   // cnt | parent | slot, [pairs] each
    a.parent = a.cnt + pairs;
    a.slot = a.parent + pairs;
    a.ctr = ob.ctr.p;
    a.object_of_row = ob.of_row.p;
    unsigned long long ctr[kWallObjectCounters];
    GMW_HIP(ctx, hipMemsetAsync(a.cnt, 0, pairs * 4, s));
    GMW_HIP(ctx, hipMemsetAsync(a.ctr, 0, kWallObjectCounters * 8, s));
    launch_wall_object_label(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    GMW_HIP(ctx, hipStreamSynchronize(s));   // the one count the host needs: it sizes the records
    const uint64_t ncomp = ctr[7];
    if (ncomp) {
        GMW_HIP(ctx, ob.recs.reserve(ncomp * (sizeof(WallObjectAcc) + sizeof(gm_wall_object) + 4 + 4)));
        Carve recs{ob.recs.p};
        a.acc = recs.take<WallObjectAcc>(ncomp);
        a.out = recs.take<gm_wall_object>(ncomp);
        a.out_slot = recs.take<uint32_t>(ncomp);
        a.pos = recs.take<int32_t>(ncomp);
        a.ncomp = (uint32_t)ncomp;
        GMW_HIP(ctx, hipMemsetAsync(a.acc, 0, ncomp * sizeof(WallObjectAcc), s));
        launch_wall_object_reduce(a, s);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
        GMW_HIP(ctx, hipStreamSynchronize(s));
    }
    const uint32_t nobj = (uint32_t)ctr[8];
    info->rejected = (uint32_t)ctr[0]; info->outside_window = (uint32_t)ctr[1]; info->sparse = (uint32_t)ctr[2];
    info->small = (uint32_t)ctr[3]; info->in_object = (uint32_t)ctr[4];
    info->flagged_neg = (uint32_t)ctr[5]; info->flagged_pos = (uint32_t)ctr[6];
    info->components = (uint32_t)ncomp;
    info->objects = nobj;
    if (side_rows)
        for (int k = 0; k < GM_WALL_JOINT_MAX_SIDES; ++k) side_rows[k] = (uint32_t)ctr[kWallObjectSideRows + k];
    if (n_out) *n_out = nobj;
    const bool fits = nobj <= capacity;
    if (nobj && ((objects && fits) || object_of_row)) {   // the list in (label, sign) order
        ob.host.resize(nobj);
        ob.host_slot.resize(nobj);
        ob.order.resize(nobj);
        GMW_HIP(ctx, hipMemcpyAsync(ob.host.data(), a.out, (size_t)nobj * sizeof(gm_wall_object), hipMemcpyDeviceToHost, s));
        GMW_HIP(ctx, hipMemcpyAsync(ob.host_slot.data(), a.out_slot, (size_t)nobj * 4, hipMemcpyDeviceToHost, s));
        GMW_HIP(ctx, hipStreamSynchronize(s));
        for (uint32_t i = 0; i < nobj; ++i) ob.order[i] = i;
        const std::vector<gm_wall_object> &h = ob.host;
        std::sort(ob.order.begin(), ob.order.end(), [&h](uint32_t x, uint32_t y) {
            return h[x].label != h[y].label ? h[x].label < h[y].label : h[x].sign < h[y].sign;
        });
        if (objects && fits)
            for (uint32_t i = 0; i < nobj; ++i) objects[i] = h[ob.order[i]];
    }
    if (object_of_row) {
        if (ncomp) {
            ob.pos.assign((size_t)ncomp, -1);
            for (uint32_t i = 0; i < nobj; ++i) ob.pos[ob.host_slot[ob.order[i]]] = (int32_t)i;
            GMW_HIP(ctx, hipMemcpyAsync(const_cast<int32_t *>(a.pos), ob.pos.data(), (size_t)ncomp * 4, hipMemcpyHostToDevice, s));
            launch_wall_object_rows(a, s);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(object_of_row, a.object_of_row, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
            GMW_HIP(ctx, hipStreamSynchronize(s));
        } else {
            std::fill(object_of_row, object_of_row + n_rows, -1);
        }
    }
    if (!fits && (objects || capacity)) return gm_fail(ctx, GM_ERR_CAPACITY, who);
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

extern "C" {

gm_status gm_wall_map_check_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_check_params *prm, gm_wall_add_info *add_info)
{
    const gm_wall_check_params cp = params_or(prm, gm_wall_check_default_params);
    WallCheckArgs a;
    memset(&a, 0, sizeof(a));
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(map, ctx, slot, "gm_wall_map_check_frame", [&] { return check_prm_ok(cp, a.T); }, sl));
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, a.w, nullptr, &ax));
    a.w.gate = (float)cp.gate;
    if (add_info) add_info->gate = a.w.gate;
    GMW_OK(set_device(ctx));
    const uint32_t n_cap = sl->n_in ? sl->n_in : 1u;
    ScanState scan;
    GMW_OK(check_prepare(map, slot, n_cap, sl->stream, scan, a));
    GMW_OK(wait_adds(map, slot, sl->stream));
    frame_points(ctx, *sl, a.w);
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    return check_enqueue(map, slot, a, ax, n_cap, scan, sl->stream);
}

gm_status gm_wall_map_get_check(gm_wall_map *map, uint32_t slot, gm_wall_check_info *info, gm_wall_check_point *points,
                                uint32_t capacity, uint32_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->checks[slot].res.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_check: no check was enqueued on this map and slot");
    GMW_OK(set_device(ctx));
    return check_result(map, slot, info, points, capacity, n_out);
}

gm_status gm_wall_map_check_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                   const gm_wall_check_params *prm, gm_wall_add_info *add_info, gm_wall_check_info *info,
                                   gm_wall_check_point *points, uint32_t capacity, uint32_t *n_out, float *residual,
                                   int32_t *cell, int32_t *delta, uint8_t *cls)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_points: NULL xyz");
    if (!points && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_points: NULL points with a capacity");
    const gm_wall_check_params cp = params_or(prm, gm_wall_check_default_params);
    WallCheckArgs a;
    memset(&a, 0, sizeof(a));
    if (!check_prm_ok(cp, a.T))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_points: struct_size mismatch or a parameter outside its limits");
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, a.w, nullptr, &ax));
    a.w.gate = (float)cp.gate;
    if (add_info) add_info->gate = a.w.gate;
    StageCall sc{map, n, map->pt, residual, cell, delta, cls, nullptr};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    const uint32_t n_cap = n ? n : 1u;
    ScanState scan;
    GMW_OK(check_prepare(map, 0, n_cap, s, scan, a));
    GMW_OK(wait_adds(map, 0, s));
    GMW_OK(sc.upload(xyz, labels, a.w));
    a.delta = map->pt.dev_delta();
    a.cls = map->pt.dev_cls();
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    a.row_is_index = 1u;
    GMW_OK(check_enqueue(map, 0, a, ax, n_cap, scan, s));
    GMW_OK(sc.close());
    return check_result(map, 0, info, points, capacity, n_out);
}

gm_status gm_wall_map_locate_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                   const gm_wall_locate_params *prm)
{
    const gm_wall_locate_params lp = params_or(prm, gm_wall_locate_default_params);
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(map, ctx, slot, "gm_wall_map_locate_frame", [&] { return locate_prm_ok(lp); }, sl));
    WallLocateArgs a;
    WallFrame64 f;
    GMW_OK(locate_args(map, pose, lp, a, f));
    GMW_OK(set_device(ctx));
    GMW_OK(locate_prepare(map, slot, sl->stream, a));
    GMW_OK(wait_adds(map, slot, sl->stream));
    frame_points(ctx, *sl, a.w);
    return locate_enqueue(map, slot, a, f, sl->stream);
}

gm_status gm_wall_map_get_locate(gm_wall_map *map, uint32_t slot, gm_wall_locate_info *info)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_get_locate: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->locates[slot].res.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_locate: no locate was enqueued on this map and slot");
    GMW_OK(set_device(ctx));
    return locate_result(map, slot, info);
}

gm_status gm_wall_map_locate_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                    const gm_wall_locate_params *prm, gm_wall_locate_info *info, float *residual, int32_t *cell)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_locate_points: NULL info");
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_locate_points: NULL xyz");
    const gm_wall_locate_params lp = params_or(prm, gm_wall_locate_default_params);
    if (!locate_prm_ok(lp))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_locate_points: struct_size mismatch or a parameter outside its limits");
    WallLocateArgs a;
    WallFrame64 f;
    GMW_OK(locate_args(map, pose, lp, a, f));
    StageCall sc{map, n, map->pt, residual, cell, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    GMW_OK(locate_prepare(map, 0, s, a));
    GMW_OK(wait_adds(map, 0, s));
    GMW_OK(sc.upload(xyz, labels, a.w));
    GMW_OK(locate_enqueue(map, 0, a, f, s));
    GMW_OK(sc.close());
    return locate_result(map, 0, info);
}

gm_status gm_wall_map_align_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_align_params *prm, gm_wall_add_info *add_info)
{
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(map, ctx, slot, "gm_wall_map_align_frame", [&] { return align_prm_ok(ap, map->prm.n_sectors); }, sl));
    WallAlignArgs a;
    GMW_OK(align_args(map, pose, ap, add_info, a));
    GMW_OK(set_device(ctx));
    GMW_OK(align_prepare(map, slot, sl->stream, a));
    frame_points(ctx, *sl, a.w);
    return align_enqueue(map, slot, a, sl->n_in ? sl->n_in : 1u, ap, pose, sl->stream);
}

gm_status gm_wall_map_get_align(gm_wall_map *map, uint32_t slot, gm_wall_align_info *info, gm_wall_align_score *scores,
                                uint32_t capacity, uint32_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->aligns[slot].res.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_align: no align was enqueued on this map and slot");
    GMW_OK(set_device(ctx));
    return align_result(map, slot, info, scores, capacity, n_out);
}

gm_status gm_wall_map_align_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                   const gm_wall_align_params *prm, gm_wall_add_info *add_info, gm_wall_align_info *info,
                                   gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out, float *residual,
                                   int32_t *cell)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_align_points: NULL xyz");
    if (!scores && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_align_points: NULL scores with a capacity");
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    if (!align_prm_ok(ap, map->prm.n_sectors))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_align_points: struct_size mismatch or a parameter outside its limits");
    WallAlignArgs a;
    GMW_OK(align_args(map, pose, ap, add_info, a));
    StageCall sc{map, n, map->pt, residual, cell, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    GMW_OK(align_prepare(map, 0, s, a));
    GMW_OK(sc.upload(xyz, labels, a.w));
    GMW_OK(align_enqueue(map, 0, a, n ? n : 1u, ap, pose, s));
    GMW_OK(sc.close());
    return align_result(map, 0, info, scores, capacity, n_out);
}

gm_status gm_wall_map_check_objects(gm_wall_map *map, uint32_t slot, const gm_wall_object_params *prm, gm_wall_objects_info *info,
                                    gm_wall_object *objects, uint32_t capacity, uint32_t *n_out, int32_t *object_of_row,
                                    uint32_t row_capacity)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    const gm_wall_object_params op = params_or(prm, gm_wall_object_default_params);
    if (!object_prm_ok(op))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: struct_size mismatch or a parameter outside its limits");
    if (!objects && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: NULL objects with a capacity");
    if (!object_of_row && row_capacity)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: NULL object_of_row with a row capacity");
    WallCheckSlot &c = map->checks[slot];
    if (!c.res.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_check_objects: no check was enqueued on this map and slot");
    ObjectWindow win;
    if (!object_window(map->prm.n_stations, map->prm.n_sectors, op, c.anchor, win))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: the window holds more than GM_WALL_OBJECT_MAX_BLOCKS blocks");
    GMW_OK(set_device(ctx));
    GMW_OK(c.res.wait(ctx));   // that check only: the slot's stream may be busy with the next frame
    const uint32_t n_rows = (uint32_t)c.h_ctr[9];
    const bool rows_fit = !object_of_row || row_capacity >= n_rows;
    // (a check's own rows are never rejected: with nothing to launch they are all outside the window)
    info->struct_size = (uint32_t)sizeof(gm_wall_objects_info);
    const ObjectGrid grid{map->prm.n_sectors, (uint32_t)map->ncell, {}};
    const gm_status st = objects_run(ctx, map->stream, map->ob, grid, c.stage.p, n_rows, 0u, nullptr, op, win, info, nullptr, objects, capacity,
                                     n_out, rows_fit ? object_of_row : nullptr, "gm_wall_map_check_objects: object buffer too small");
    if (st != GM_OK) return st;
    if (!rows_fit) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_check_objects: object_of_row buffer too small");
    return GM_OK;
}

gm_status gm_wall_check_objects(gm_wall_map *map, const gm_wall_check_point *rows, uint32_t n_rows, int64_t anchor_station,
                                const gm_wall_object_params *prm, gm_wall_objects_info *info, gm_wall_object *objects,
                                uint32_t capacity, uint32_t *n_out, int32_t *object_of_row)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: NULL info");
    if (n_rows && !rows) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: NULL rows");
    const gm_wall_object_params op = params_or(prm, gm_wall_object_default_params);
    if (!object_prm_ok(op))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: struct_size mismatch or a parameter outside its limits");
    if (!objects && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: NULL objects with a capacity");
    ObjectWindow win;
    if (!object_window(map->prm.n_stations, map->prm.n_sectors, op, anchor_station, win))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: the window holds more than GM_WALL_OBJECT_MAX_BLOCKS blocks");
    GMW_OK(set_device(ctx));
    uint32_t rejected = 0;
    if (n_rows && !win.nJ) {   // nothing will be launched: the one class that needs the rows, on the host
        for (uint32_t i = 0; i < n_rows; ++i) {
            uint32_t b[5];
            memcpy(b, &rows[i], sizeof(b));   // x y z delta e
            if (wall_object_rejected(b[0], b[1], b[2], b[4], rows[i].cell, wall_check_fix(rows[i].delta), (uint32_t)map->ncell)) ++rejected;
        }
    } else if (n_rows) {
        GMW_HIP(ctx, map->ob.rows.reserve(n_rows));
        GMW_HIP(ctx, hipMemcpyAsync(map->ob.rows.p, rows, (size_t)n_rows * sizeof(gm_wall_check_point), hipMemcpyHostToDevice, map->stream));
    }
    info->struct_size = (uint32_t)sizeof(gm_wall_objects_info);
    const ObjectGrid grid{map->prm.n_sectors, (uint32_t)map->ncell, {}};
    return objects_run(ctx, map->stream, map->ob, grid, map->ob.rows.p, n_rows, rejected, nullptr, op, win, info, nullptr, objects, capacity,
                       n_out, object_of_row, "gm_wall_check_objects: object buffer too small");
}

}  // extern "C"
