// gm_wall_alignment_objects.hip -- C ABI of a check's objects on the wall alignment (gm_wall_alignment_check_objects,
// gm_wall_alignment_check_objects_rows; include/gm_hip.h states the rule).  Host logic only: where the rows of the slot's
// last check are staged, the plan's sides as the kernels' side table, the window on the global station grid.  The call
// itself is objects_run (gm_wall_slot.hip), shared with gm_wall_map_check_objects, on the alignment's own scratch; the
// kernels that read a row are k_wall_objects_joint.hip's, the others k_wall_objects.hip's; the window and the device-free
// calls are in gm_wall_alignment_host.hip.
#include <stddef.h>

#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace {

// the refusals both calls share, in gm_wall_map_check_objects' order; op: the parameters
gm_status objects_head(gm_ctx *ctx, const char *who, const gm_wall_object_params *prm, const gm_wall_alignment_objects_info *info,
                       const gm_wall_object *objects, uint32_t capacity, gm_wall_object_params &op)
{
    auto refuse = [&](const char *why) { return gm_fail(ctx, GM_ERR_INVALID_ARG, (std::string(who) + why).c_str()); };
    if (!info) return refuse(": NULL info");
    op = params_or(prm, gm_wall_object_default_params);
    if (!object_prm_ok(op)) return refuse(": struct_size mismatch or a parameter outside its limits");
    if (!objects && capacity) return refuse(": NULL objects with a capacity");
    return GM_OK;
}

// the window of `plan`, the grid and the side table; the host half's refusals as the call's failure
gm_status objects_grid(gm_wall_alignment *al, const char *who, const gm_wall_alignment_add_info &plan, const gm_wall_object_params &op,
                       ObjectWindow &win, ObjectGrid &grid, gm_wall_alignment_objects_info *info)
{
    gm_ctx *ctx = al->ctx;
    const gm_status st = alignment_object_window(al->A, plan, op, win, info);
    if (st == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, st, (std::string(who) + ": the alignment's stations or its blocks do not fit 32 bits").c_str());
    if (st != GM_OK)
        return gm_fail(ctx, st, (std::string(who) + ": a plan whose sides are not consecutive elements of this alignment around its "
                                                    "element, or a window above GM_WALL_OBJECT_MAX_BLOCKS blocks").c_str());
    grid.nsec = al->A.el[0].p.n_sectors;
    grid.cells = 0u;   // (the map kernels' field; every side has its own below)
    grid.sides.n_sides = plan.n_sides;
    for (uint32_t k = 0; k < plan.n_sides; ++k) {
        grid.sides.first[k] = info->side_first[k];
        grid.sides.cells[k] = (uint32_t)al->maps[plan.side_element[k]]->ncell;   // <= GM_WALL_MAX_CELLS
    }
    return GM_OK;
}

// the shared head of the two infos, as objects_run fills it
gm_wall_objects_info *head_of(gm_wall_alignment_objects_info *info)
{
    static_assert(offsetof(gm_wall_alignment_objects_info, n_rows) == offsetof(gm_wall_objects_info, n_rows) &&
                      offsetof(gm_wall_alignment_objects_info, reserved) == offsetof(gm_wall_objects_info, reserved) &&
                      offsetof(gm_wall_alignment_objects_info, element) == sizeof(gm_wall_objects_info),
                  "the shared head");
    return reinterpret_cast<gm_wall_objects_info *>(info);
}

}  // namespace

extern "C" {

gm_status gm_wall_alignment_check_objects(gm_wall_alignment *alignment, uint32_t slot, const gm_wall_object_params *prm,
                                          gm_wall_alignment_objects_info *info, gm_wall_object *objects, uint32_t capacity,
                                          uint32_t *n_out, int32_t *object_of_row, uint32_t row_capacity)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    const char *who = "gm_wall_alignment_check_objects";
    if (n_out) *n_out = 0;
    gm_wall_object_params op;
    GMW_OK(objects_head(ctx, who, prm, info, objects, capacity, op));
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!object_of_row && row_capacity)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_objects: NULL object_of_row with a row capacity");
    gm_wall_alignment::CheckSlot &c = alignment->checks[slot];
    if (!c.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_check_objects: no check was enqueued on this alignment and slot");
    if (c.own && (!c.own->checks[slot].res.have || c.own->checks[slot].scan.epoch != c.own_epoch))
        return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_alignment_check_objects: a check on the element map itself has replaced the alignment's rows");
    ObjectWindow win;
    ObjectGrid grid;
    GMW_OK(objects_grid(alignment, who, c.plan, op, win, grid, info));
    GMW_OK(set_device(ctx));
    // the rows of the alignment's last check on this slot, wherever they are staged; that check only is waited for
    WallCheckSlot *oc = c.own ? &c.own->checks[slot] : nullptr;
    GMW_OK(oc ? oc->res.wait(ctx) : alignment->check_res[slot].wait(ctx));
    const unsigned long long *h = oc ? oc->h_ctr.p : c.h_ctr.p;
    const uint32_t n_rows = (uint32_t)h[9];
    // (a check's own rows are never rejected: with nothing to launch each side's rows are its changed points)
    uint32_t side_rows[GM_WALL_JOINT_MAX_SIDES] = {};
    if (oc) side_rows[0] = n_rows;
    else
        for (uint32_t k = 0; k < c.plan.n_sides; ++k)
            side_rows[k] = (uint32_t)(h[kWallCheckCounters + k * GM_WALL_CHECK_N_CLS + GM_WALL_CHECK_CLS_CHANGED_POS] +
                                      h[kWallCheckCounters + k * GM_WALL_CHECK_N_CLS + GM_WALL_CHECK_CLS_CHANGED_NEG]);
    const bool rows_fit = !object_of_row || row_capacity >= n_rows;
    // on a map's own stream: the slot's may be busy with the next frame
    const gm_status st = objects_run(ctx, alignment->maps[0]->stream, alignment->ob, grid, oc ? oc->stage.p : c.stage.p, n_rows, 0u, side_rows,
                                     op, win, head_of(info), info->side_rows, objects, capacity, n_out, rows_fit ? object_of_row : nullptr,
                                     "gm_wall_alignment_check_objects: object buffer too small");
    if (st != GM_OK) return st;
    if (!rows_fit) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_alignment_check_objects: object_of_row buffer too small");
    return GM_OK;
}

gm_status gm_wall_alignment_check_objects_rows(gm_wall_alignment *alignment, const gm_wall_check_point *rows, uint32_t n_rows,
                                               const gm_wall_alignment_add_info *plan, const gm_wall_object_params *prm,
                                               gm_wall_alignment_objects_info *info, gm_wall_object *objects, uint32_t capacity,
                                               uint32_t *n_out, int32_t *object_of_row)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    const char *who = "gm_wall_alignment_check_objects_rows";
    if (n_out) *n_out = 0;
    gm_wall_object_params op;
    GMW_OK(objects_head(ctx, who, prm, info, objects, capacity, op));
    if (n_rows && !rows) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_objects_rows: NULL rows");
    if (!plan) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_check_objects_rows: NULL plan");
    ObjectWindow win;
    ObjectGrid grid;
    GMW_OK(objects_grid(alignment, who, *plan, op, win, grid, info));
    GMW_OK(set_device(ctx));
    hipStream_t s = alignment->maps[0]->stream;
    uint32_t rejected = 0, side_rows[GM_WALL_JOINT_MAX_SIDES] = {};
    if (n_rows && !win.nJ) {   // nothing will be launched: the classes that need the rows, on the host
        for (uint32_t i = 0; i < n_rows; ++i) {
            uint32_t b[5];
            memcpy(b, &rows[i], sizeof(b));   // x y z delta e
            const uint32_t side = GM_WALL_ROW_SIDE(rows[i].cell);
            if (side >= grid.sides.n_sides ||
                wall_object_rejected(b[0], b[1], b[2], b[4], (int32_t)GM_WALL_ROW_CELL(rows[i].cell), wall_check_fix(rows[i].delta),
                                     grid.sides.cells[side]))
                ++rejected;
            else
                ++side_rows[side];
        }
    } else if (n_rows) {
        GMW_HIP(ctx, alignment->ob.rows.reserve(n_rows));
        GMW_HIP(ctx, hipMemcpyAsync(alignment->ob.rows.p, rows, (size_t)n_rows * sizeof(gm_wall_check_point), hipMemcpyHostToDevice, s));
    }
    return objects_run(ctx, s, alignment->ob, grid, alignment->ob.rows.p, n_rows, rejected, side_rows, op, win, head_of(info), info->side_rows,
                       objects, capacity, n_out, object_of_row, "gm_wall_alignment_check_objects_rows: object buffer too small");
}

}  // extern "C"
