// gm_wall_alignment.hip -- C ABI of the wall alignment (gm_wall_alignment_*; include/gm_hip.h states the rule): the object
// (create, destroy, map, info, sync) and the add.  Host logic only: the element maps, the plan of a call and its refusals, the
// sides of a plan (their per-add frames: add_frame_args of each element map, unchanged), the deal of the add's LDS table.
// gm_wall_alignment.hpp declares what the other call families take from here: the locate is gm_wall_alignment_locate.hip,
// the align gm_wall_alignment_align.hip, the check and the checked add gm_wall_alignment_check.hip.  The add's kernel is k_wall_joint.hip's; the device-free calls
// are in gm_wall_alignment_host.hip.
#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

gm_status joint_refusal(gm_ctx *ctx, gm_status st)
{
    if (st == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, st, "gm_wall_alignment: the frame's reach meets more than GM_WALL_JOINT_MAX_SIDES elements");
    return st == GM_OK ? GM_OK : gm_fail(ctx, st, "gm_wall_alignment: bad pose, or a pose too far along the axis");
}

gm_status joint_plan(gm_wall_alignment *al, const double pose[12], gm_wall_alignment_add_info &plan,
                     gm_wall_map *(&side)[GM_WALL_JOINT_MAX_SIDES])
{
    gm_ctx *ctx = al->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment: NULL pose");
    GMW_OK(joint_refusal(ctx, alignment_add_plan(al->A, pose, ctx->cfg.boxFilterBound, &plan)));
    for (uint32_t k = 0; k < plan.n_sides; ++k) side[k] = al->maps[plan.side_element[k]];
    return GM_OK;
}

gm_status joint_sides(gm_wall_map *const (&map)[GM_WALL_JOINT_MAX_SIDES], const double pose[12], const gm_wall_alignment_add_info &plan,
                      WallJointSide (&side)[GM_WALL_JOINT_MAX_SIDES], WallJointGrid &grid, WallJointPlanes &planes)
{
    const uint32_t ns = plan.n_sides;
    for (uint32_t k = 0; k < ns; ++k) {
        gm_wall_map *m = map[k];
        WallArgs w;
        WallAxis ax;
        GMW_OK(add_frame_args(m, pose, nullptr, w, nullptr, &ax));
        WallJointSide &S = side[k];
        S.anchor = w.anchor;
        for (int c = 0; c < 3; ++c) { S.o[c] = w.o[c]; S.a[c] = w.a[c]; S.u[c] = w.u[c]; S.v[c] = w.v[c]; }
        S.ax = ax.ax;
        S.table = w.table;
        S.n_stations = w.n_stations;
        S.win_first = w.win_first;
        S.win_stations = w.win_stations;
        S.axis = ax.kind;
        S.element = (int32_t)plan.side_element[k];
        if (k == 0u) grid = WallJointGrid{w.R, w.station_length, w.sector_angle, w.two_pi, w.n_sectors};
    }
    for (uint32_t k = 0; k + 1u < ns; ++k)
        for (int c = 0; c < 3; ++c) { planes.jo[k][c] = plan.joint_o[k][c]; planes.ja[k][c] = plan.joint_a[k][c]; }
    return GM_OK;
}

// The deal of the add's LDS table: each side's window is the stations of its map's own window that lie in the element, cut to
// what the table has left, in the order of the sides.
static void joint_deal_windows(WallJointArgs &a)
{
    const uint32_t nsec = a.grid.n_sectors;
    uint32_t left = GM_SURF_MAX_CELLS;
    for (uint32_t k = 0; k < a.n_sides; ++k) {
        WallJointSide &S = a.side[k];
        const int64_t lo = std::max<int64_t>(S.anchor + S.win_first, 0);
        const int64_t hi = std::min<int64_t>(S.anchor + S.win_first + (int64_t)S.win_stations, (int64_t)S.n_stations);
        const uint32_t nst = (uint32_t)std::min<int64_t>(std::max<int64_t>(hi - lo, 0), (int64_t)(left / nsec));
        S.win_first = nst ? (int32_t)(lo - S.anchor) : 0;
        S.win_stations = nst;
        S.lds_first = GM_SURF_MAX_CELLS - left;
        left -= nst * nsec;
    }
    a.lds_cells = GM_SURF_MAX_CELLS - left;
}

gm_status joint_add_args(gm_wall_alignment *al, const double pose[12], JointAdd &j)
{
    GMW_OK(joint_plan(al, pose, j.plan, j.side));
    memset(&j.ja, 0, sizeof(j.ja));
    j.ja.n_sides = j.plan.n_sides;
    if (j.plan.n_sides < 2u) return GM_OK;   // (the map's own add computes its frame)
    GMW_OK(joint_sides(j.side, pose, j.plan, j.ja.side, j.ja.grid, j.ja.planes));
    j.ja.gate = (float)j.side[0]->prm.gate;   // (the map's own, as add_frame_args rounds it)
    joint_deal_windows(j.ja);
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

namespace {

void free_alignment(gm_wall_alignment *al, bool maps_too)
{
    for (std::vector<PendingResult> *v : {&al->locate_res, &al->check_res, &al->add_res, &al->align_res})
        for (PendingResult &r : *v) r.release();   // nothing may still be writing the alignment's blocks
    for (gm_wall_map *m : al->maps) { m->al_locates = nullptr; m->al_checks = nullptr; m->al_aligns = nullptr; }
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
        if (E.ax.is_clothoid()) ms = gm_wall_map_create_clothoid(ctx, &E.p, &E.cl, &m);
        else if (E.ax.is_arc()) ms = gm_wall_map_create_arc(ctx, &E.p, &E.arc, &m);
        else ms = gm_wall_map_create(ctx, &E.p, &m);
        if (ms != GM_OK) {
            free_alignment(al, true);
            return ms;
        }
        al->maps.push_back(m);
    }
    // the per-slot state of the locates, the checks and the aligns (no device memory: vectors of empty owners); the element
    // maps learn where the pending results are
    al->ob.read_tile_env();
    al->tpl = *params;
    al->elements.assign(elements, elements + n);
    al->locates.resize(ctx->n_slots);
    al->checks.resize(ctx->n_slots);
    al->aligns.resize(ctx->n_slots);
    for (std::vector<PendingResult> *v : {&al->locate_res, &al->check_res, &al->add_res, &al->align_res}) v->resize(ctx->n_slots);
    for (gm_wall_map *m : al->maps) { m->al_locates = &al->locate_res; m->al_checks = &al->check_res; m->al_aligns = &al->align_res; }
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
    joint_points(j.ja, w);
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
    StageCall sc{j.side[0], n, alignment->pt, residual, cell, nullptr, nullptr, element};
    GMW_OK(sc.open());
    GMW_OK(joint_upload(sc, xyz, labels, j.ja));
    hipStream_t s = sc.sl->stream;
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) GMW_OK(add_wait_readers(j.side[k], 0, s));   // (the staging slot is slot 0)
    launch_wall_add_joint(j.ja, n, j.side[0]->points_per_block, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_OK(sc.close());   // (blocks until the slot's stream has drained)
    for (uint32_t k = 0; k < j.plan.n_sides; ++k) ++j.side[k]->frames;
    return GM_OK;
}

gm_status gm_wall_alignment_sync(gm_wall_alignment *alignment)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    for (gm_wall_map *m : alignment->maps) GMW_OK(gm_wall_map_sync(m));
    for (std::vector<PendingResult> *v : {&alignment->locate_res, &alignment->check_res, &alignment->add_res, &alignment->align_res})
        for (PendingResult &r : *v) GMW_OK(r.wait(alignment->ctx));
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
