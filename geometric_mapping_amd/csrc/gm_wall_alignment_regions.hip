// gm_wall_alignment_regions.hip -- C ABI of the deviation regions of a window of the wall alignment
// (gm_wall_alignment_regions; include/gm_hip.h states the rule).  Host logic only: the refusals in gm_wall_map_regions'
// order, the baseline, the window's pieces as the joint kernels take them, the sync of the element maps the window meets.
// The call itself is regions_run (gm_wall.hip), shared with gm_wall_map_regions, on the alignment's own scratch; the two
// kernels that read a cell are k_wall_regions_joint.hip's, the others k_wall_regions.hip's; the window and the device-free
// calls are in gm_wall_alignment_host.hip.
#include <stddef.h>

#include "gm_wall_alignment.hpp"

using namespace gm;
using namespace gm::wall;

namespace {

// the refusals of a baseline (NULL: none): the alignment itself, another context, another template, another element list
gm_status check_baseline(gm_wall_alignment *al, gm_wall_alignment *baseline)
{
    if (!baseline) return GM_OK;
    gm_ctx *ctx = al->ctx;
    auto refuse = [&](const char *why) { return gm_fail(ctx, GM_ERR_INVALID_ARG, (std::string("gm_wall_alignment_regions") + why).c_str()); };
    if (baseline == al) return refuse(": the baseline is the alignment itself");
    if (baseline->ctx != ctx) return refuse(": the baseline belongs to another context");
    const gm_wall_params &p = al->tpl, &b = baseline->tpl;   // (n_stations is not read from a template; gate may differ)
    if (p.n_sectors != b.n_sectors || memcmp(&p.station_length, &b.station_length, 8) || memcmp(&p.t_min, &b.t_min, 8) ||
        memcmp(p.point, b.point, 24) || memcmp(p.direction, b.direction, 24) || memcmp(&p.radius, &b.radius, 8) || memcmp(p.up, b.up, 24) ||
        memcmp(p.forward, b.forward, 24))
        return refuse(": the baseline is an alignment on another template");
    if (al->elements.size() != baseline->elements.size()) return refuse(": the baseline has another element list");
    for (size_t i = 0; i < al->elements.size(); ++i) {
        const gm_wall_element &x = al->elements[i], &y = baseline->elements[i];
        if (x.kind != y.kind || x.n_stations != y.n_stations || memcmp(x.turn, y.turn, sizeof(x.turn)) || memcmp(&x.curvature, &y.curvature, 8) ||
            memcmp(&x.rate, &y.rate, 8))
            return refuse(": the baseline has another element list");
    }
    return GM_OK;
}

// the shared head of the two infos, as regions_run fills it
gm_wall_regions_info *head_of(gm_wall_alignment_regions_info *info)
{
    static_assert(offsetof(gm_wall_alignment_regions_info, station0) == offsetof(gm_wall_regions_info, station0) &&
                      offsetof(gm_wall_alignment_regions_info, flagged_pos) == offsetof(gm_wall_regions_info, flagged_pos) &&
                      offsetof(gm_wall_alignment_regions_info, cell_area) == offsetof(gm_wall_regions_info, cell_area) &&
                      offsetof(gm_wall_alignment_regions_info, total) == sizeof(gm_wall_regions_info),
                  "the shared head");
    return reinterpret_cast<gm_wall_regions_info *>(info);
}

}  // namespace

extern "C" {

gm_status gm_wall_alignment_regions(gm_wall_alignment *alignment, gm_wall_alignment *baseline, uint32_t station0, uint32_t n,
                                    const gm_wall_region_params *prm, gm_wall_alignment_regions_info *info, gm_wall_region *regions,
                                    uint32_t capacity, uint32_t *n_out, int32_t *cell_labels)
{
    if (!alignment) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = alignment->ctx;
    const char *who = "gm_wall_alignment_regions";
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_regions: NULL info");
    const gm_wall_region_params rp = params_or(prm, gm_wall_region_default_params);
    long long T = 0;
    if (const char *why = region_prm_refusal(rp, T)) return gm_fail(ctx, GM_ERR_INVALID_ARG, (std::string(who) + why).c_str());
    if (!regions && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_regions: NULL regions with a capacity");
    GMW_OK(check_baseline(alignment, baseline));
    const gm_status wst = alignment_region_window(alignment->A, station0, n, info);
    if (wst == GM_ERR_UNSUPPORTED)
        return gm_fail(ctx, wst, "gm_wall_alignment_regions: the alignment's cells do not fit 31 bits, or a window above "
                                 "GM_WALL_ALIGNMENT_REGION_MAX_CELLS cells");
    if (wst != GM_OK) return gm_fail(ctx, wst, "gm_wall_alignment_regions: the window leaves [0, total]");
    info->threshold_q = T;
    // every element map the window meets, and the baseline's: every add enqueued so far, through the alignment or not
    for (uint32_t k = 0; k < info->n_pieces; ++k) {
        GMW_OK(gm_wall_map_sync(alignment->maps[info->element_from + k]));
        if (baseline) GMW_OK(gm_wall_map_sync(baseline->maps[info->element_from + k]));
    }
    if (!n) return GM_OK;

    // the pieces, ascending and gapless over the window's rows; each is checked against its map before it leaves the host
    const uint32_t np = info->n_pieces, nsec = info->n_sectors;
    GMW_OK(set_device(ctx));
    GMW_HIP(ctx, alignment->rg.pieces.reserve(np));
    GMW_HIP(ctx, alignment->rg_pieces_host.reserve(np));
    WallRegionPiece *pc = alignment->rg_pieces_host.p;
    uint32_t row = 0;
    for (uint32_t k = 0; k < np; ++k) {
        const uint32_t e = info->element_from + k;
        gm_wall_map *m = alignment->maps[e];
        const uint32_t first = k == 0u ? info->station_from : 0u;
        const uint32_t last = k + 1u == np ? info->station_to : m->prm.n_stations - 1u;
        if (first > last || last >= m->prm.n_stations || m->prm.n_sectors != nsec || (baseline && baseline->maps[e]->ncell != m->ncell))
            return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_regions: a piece outside its element map");
        memset(&pc[k], 0, sizeof(pc[k]));
        pc[k].row0 = row;
        pc[k].station0 = first;
        pc[k].rows = last - first + 1u;
        pc[k].map = m->table;
        pc[k].base = baseline ? baseline->maps[e]->table : m->table;
        row += pc[k].rows;
    }
    if (row != n) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_alignment_regions: the pieces do not cover the window");
    // on a map's own stream, as the objects call: a slot's may be busy with the next frame
    gm_wall_map *m0 = alignment->maps[0];
    hipStream_t s = m0->stream;
    GMW_HIP(ctx, hipMemcpyAsync(alignment->rg.pieces.p, pc, (size_t)np * sizeof(WallRegionPiece), hipMemcpyHostToDevice, s));
    alignment->rg.ts = m0->rg.ts;
    alignment->rg.tk = m0->rg.tk;

    WallRegionArgs a;
    memset(&a, 0, sizeof(a));
    a.has_base = baseline ? 1u : 0u;
    a.n = n;
    a.nsec = nsec;
    a.first = (uint64_t)station0 * nsec;   // (global: < 2^31 by the size rule)
    a.conn8 = rp.connectivity == 8u ? 1u : 0u;
    a.min_count = rp.min_count;
    a.min_cells = rp.min_cells;
    a.T = T;
    a.n_pieces = np;
    a.pieces = alignment->rg.pieces.p;
    // (element map 0's staging holds min(kStageCells, its cells) raw records of 24 B: room for six labels each)
    return regions_run(ctx, s, alignment->rg, a, reinterpret_cast<int32_t *>(m0->stage.p), std::min(kStageCells, m0->ncell * 6u), head_of(info),
                       regions, capacity, n_out, cell_labels, "gm_wall_alignment_regions: region buffer too small");
}

}  // extern "C"
