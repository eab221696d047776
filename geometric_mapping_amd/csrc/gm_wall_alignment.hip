// gm_wall_alignment.hip -- C ABI of the wall alignment (gm_wall_alignment_*; include/gm_hip.h states the rule): the calls
// on a context.  Host logic only: the element maps, the sides of an add, their per-add frames (add_frame_args of each
// element map, unchanged), the deal of the LDS table.  The kernel is k_wall_joint.hip's, the device-free calls are in
// gm_wall_alignment_host.hip.
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

void free_alignment(gm_wall_alignment *al, bool maps_too)
{
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
