// gm_wall_add_checked.hip -- C ABI of the add less the check's changed rows (gm_wall_map_add_frame_checked,
// gm_wall_map_get_add_checked, gm_wall_map_add_points_checked; include/gm_hip.h states the rule).  Host logic only: the
// scratch of a call, the order on the slot's stream, the counts.  Kernels: k_wall_add_checked.hip (mark) and k_wall.hip
// (the masked instantiation of the add).
#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

uint64_t add_checked_block_words(uint32_t n_cap) { return kWallAddCheckedCounters + ((uint64_t)n_cap + 63u) / 64u; }

void add_checked_fill_info(gm_wall_add_checked_info *info, uint32_t status, long long S, const unsigned long long *h)
{
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_add_checked_info);
    info->status = status;
    info->min_delta_q = S;
    info->n_points = (uint32_t)h[10];
    info->n_rows = (uint32_t)h[9];
    info->rows_neg = (uint32_t)h[0]; info->rows_pos = (uint32_t)h[1];
    info->rows_kept = (uint32_t)h[2]; info->rows_rejected = (uint32_t)h[3];
    info->skipped = (uint32_t)h[4];
    info->mapped = (uint32_t)h[5]; info->outside = (uint32_t)h[6]; info->beyond_gate = (uint32_t)h[7]; info->plane = (uint32_t)h[8];
}

}  // namespace wall
}  // namespace gm

namespace {

uint64_t block_words(uint32_t n_cap) { return add_checked_block_words(n_cap); }

// What one call enqueues on `s`, in this order: its block -- counters | mask words of n_cap points -- zeroed by ONE fill, the
// mark over up to rows_cap rows, the masked add.  mk: rows, counts and parameters filled by the caller; blk: the call's.
gm_status add_checked_enqueue(gm_wall_map *m, WallMarkArgs &mk, const WallArgs &w, const WallAxis &ax, uint32_t n_cap,
                              DevArray<unsigned long long> &blk, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    GMW_HIP(ctx, blk.reserve(block_words(n_cap)));
    GMW_HIP(ctx, hipMemsetAsync(blk.p, 0, block_words(n_cap) * 8, s));
    mk.ctr = blk.p;
    mk.mask = reinterpret_cast<uint32_t *>(blk.p + kWallAddCheckedCounters);
    launch_wall_mark(mk, mk.rows_cap, s);
    launch_wall_add(w, ax, blk.p + kWallAddCheckedCounters, blk.p, n_cap, m->points_per_block, s);
    GMW_HIP(ctx, hipGetLastError());
    return GM_OK;
}

void fill_info(gm_wall_add_checked_info *info, uint32_t status, long long S, const unsigned long long *h)
{
    add_checked_fill_info(info, status, S, h);
}

}  // namespace

extern "C" {

gm_status gm_wall_map_add_frame_checked(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_add_checked_params *prm, gm_wall_add_info *add_info)
{
    const gm_wall_add_checked_params ap = params_or(prm, gm_wall_add_checked_default_params);
    WallMarkArgs mk;
    memset(&mk, 0, sizeof(mk));
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(map, ctx, slot, "gm_wall_map_add_frame_checked", [&] { return add_checked_prm_ok(ap, mk.S); }, sl));
    WallArgs w;
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, w, nullptr, &ax));
    WallCheckSlot &c = map->checks[slot];
    if (!c.res.have || c.cloud_seq != sl->cloud_seq)
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_add_frame_checked: no check was enqueued on this map and slot for the frame the slot holds");
    GMW_OK(set_device(ctx));
    WallAddCheckedSlot &ac = map->add_checks[slot];
    GMW_OK(ac.res.ensure(ctx));
    const uint32_t n_cap = sl->n_in;
    if (ac.blk.cap < block_words(n_cap) || !ac.h_ctr)
        GMW_OK(ac.res.wait(ctx));   // the slot's last checked add may still be using the old block
    GMW_HIP(ctx, ac.h_ctr.reserve(kWallAddCheckedCounters));
    frame_points(ctx, *sl, w);
    mk.rows = c.stage.p;
    mk.n_rows_ptr = c.ctr.p + 9;
    mk.rows_cap = (uint32_t)std::min<uint64_t>(c.stage.cap, n_cap);   // (a check emits at most one row per point)
    mk.n_ptr = w.n_ptr;
    mk.n_host = w.n_host;
    mk.skip = ap.skip;
    GMW_OK(add_wait_readers(map, slot, sl->stream));
    GMW_OK(add_checked_enqueue(map, mk, w, ax, n_cap, ac.blk, sl->stream));
    GMW_HIP(ctx, hipMemcpyAsync(ac.h_ctr.p, ac.blk.p, kWallAddCheckedCounters * 8, hipMemcpyDeviceToHost, sl->stream));
    GMW_OK(ac.res.record(ctx, sl->stream));
    ac.status = map->axis.d.status;
    ac.S = mk.S;
    map->pending[slot] = 1;
    ++map->frames;
    return GM_OK;
}

gm_status gm_wall_map_get_add_checked(gm_wall_map *map, uint32_t slot, gm_wall_add_checked_info *info)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_get_add_checked: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    WallAddCheckedSlot &ac = map->add_checks[slot];
    if (!ac.res.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_add_checked: no checked add was enqueued on this map and slot");
    GMW_OK(set_device(ctx));
    GMW_OK(ac.res.wait(ctx));
    fill_info(info, ac.status, ac.S, ac.h_ctr.p);
    return GM_OK;
}

gm_status gm_wall_map_add_points_checked(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_add_checked_params *prm,
                                         const gm_wall_check_point *rows, uint32_t n_rows, gm_wall_add_info *add_info,
                                         gm_wall_add_checked_info *info, float *residual, int32_t *cell)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_points_checked: NULL xyz");
    if (n_rows && !rows) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_points_checked: NULL rows");
    const gm_wall_add_checked_params ap = params_or(prm, gm_wall_add_checked_default_params);
    WallMarkArgs mk;
    memset(&mk, 0, sizeof(mk));
    if (!add_checked_prm_ok(ap, mk.S))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_points_checked: struct_size mismatch or a parameter outside its limits");
    WallArgs w;
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, w, nullptr, &ax));
    StageCall sc{map, n, map->pt, residual, cell, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    GMW_OK(sc.upload(xyz, labels, w));
    hipStream_t s = sc.sl->stream;
    GMW_HIP(ctx, map->ac_rows.reserve(n_rows ? n_rows : 1u));
    if (n_rows) GMW_HIP(ctx, hipMemcpyAsync(map->ac_rows.p, rows, (size_t)n_rows * sizeof(gm_wall_check_point), hipMemcpyHostToDevice, s));
    mk.rows = map->ac_rows.p;
    mk.n_rows_host = n_rows;
    mk.rows_cap = n_rows;
    mk.n_host = n;
    mk.skip = ap.skip;
    GMW_OK(add_wait_readers(map, 0, s));   // (as gm_wall_map_add_points; the staging slot is slot 0)
    GMW_OK(add_checked_enqueue(map, mk, w, ax, n, map->ac_blk, s));
    unsigned long long h[kWallAddCheckedCounters];
    GMW_HIP(ctx, hipMemcpyAsync(h, map->ac_blk.p, sizeof(h), hipMemcpyDeviceToHost, s));
    GMW_OK(sc.close());   // (blocks: h is filled)
    ++map->frames;
    if (info) fill_info(info, map->axis.d.status, mk.S, h);
    return GM_OK;
}

}  // extern "C"
