// gm_wall.hip -- C ABI of the persistent wall map (gm_wall_*; include/gm_hip.h states the rule): the map itself and the
// window calls.  Host logic only: the arguments of an add from the axis' per-add frame (DesignAxis, gm_wall_host.hip), the
// station window of a frame, ownership.  Kernels are in k_wall*.hip behind one launch front per family, the device-free
// calls in gm_wall_host.hip, the per-(map, slot) calls in gm_wall_slot.hip.
#include <stdio.h>
#include <stdlib.h>

#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

// the LDS window of an add: whole stations around the anchor for |t| / ds <= reach, as many as the LDS table holds; a
// footprint beyond it is centred (the rest goes to the map directly)
static void add_window(const gm_wall_params &p, double reach_stations, WallArgs &w)
{
    const uint32_t wmax = GM_SURF_MAX_CELLS / p.n_sectors;   // >= 1: n_sectors <= 4096
    const double reach = std::min(reach_stations, 1.0e6);
    const int64_t first = (int64_t)floor(-reach) - 1, last = (int64_t)floor(reach) + 2;   // one station of fp32 slack each side
    const int64_t need = last - first + 1;
    if (need <= (int64_t)wmax) {
        w.win_first = (int32_t)first;
        w.win_stations = (uint32_t)need;
    } else {
        w.win_first = -(int32_t)(wmax / 2);
        w.win_stations = wmax;
    }
}

gm_status add_frame_args(gm_wall_map *m, const double pose[12], gm_wall_add_info *info, WallArgs &w, WallFrame64 *f64, WallAxis *ax)
{
    gm_ctx *ctx = m->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: NULL pose");
    double Rm[3][3], tr[3];
    const int bad = pose_split(pose, Rm, tr);
    if (bad == 1) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose is not finite");
    if (bad) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose rotation is not orthonormal to 1e-6 or is a reflection");
    const gm_wall_params &p = m->prm;
    const DesignFrame &d = m->axis.d;
    if (m->axis.kind != kAxisStraight && !ax)
        return gm_fail(ctx, GM_ERR_UNSUPPORTED, "gm_wall_map: this call is not available on a map with an arc or a clothoid design axis");
    // what every axis computes (include/gm_hip.h: per add): (o', a', u', v') rounded once, the axis block, the anchor
    AxisAddFrame f;
    if (!m->axis.add_frame(p, Rm, tr, f)) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose is too far along the axis");
    memset(&w, 0, sizeof(w));
    for (int k = 0; k < 3; ++k) {
        w.o[k] = f.o[k]; w.a[k] = f.a[k]; w.u[k] = (float)f.u64[k]; w.v[k] = (float)f.v64[k];
        if (f64) { f64->c[k] = f.o64[k]; f64->d[k] = f.a64[k]; f64->u[k] = f.u64[k]; f64->v[k] = f.v64[k]; f64->of[k] = f.P[k]; }
    }
    if (ax) {   // (a straight map: the kind alone, the block zero)
        memset(ax, 0, sizeof(*ax));
        ax->kind = m->axis.kind;
    }
    if (ax && ax->kind != kAxisStraight) {
        for (int k = 0; k < 3; ++k) { ax->ax.arc.n[k] = f.n[k]; ax->ax.arc.b[k] = f.b[k]; }
        ax->ax.arc.kappa = f.kappa;
        ax->ax.arc.un = f.un; ax->ax.arc.ub = f.ub; ax->ax.arc.vn = f.vn; ax->ax.arc.vb = f.vb;
        ax->ax.rate = f.rate;
    }
    w.anchor = f.anchor;
    w.R = (float)d.R;
    w.station_length = (float)p.station_length;
    w.gate = (float)p.gate;
    w.sector_angle = (float)(kTwoPi / (double)p.n_sectors);
    w.two_pi = (float)kTwoPi;
    w.n_stations = p.n_stations;
    w.n_sectors = p.n_sectors;
    w.table = m->table;
    add_window(p, m->axis.reach(p, ctx->cfg.boxFilterBound, f.a1), w);
    if (info) {
        memset(info, 0, sizeof(*info));
        info->struct_size = (uint32_t)sizeof(gm_wall_add_info);
        info->status = d.status;
        info->anchor_station = w.anchor;
        for (int k = 0; k < 3; ++k) { info->o[k] = w.o[k]; info->a[k] = w.a[k]; info->u[k] = w.u[k]; info->v[k] = w.v[k]; }
        info->R = w.R;
        info->station_length = w.station_length;
        info->sector_angle = w.sector_angle;
        info->gate = w.gate;
    }
    return GM_OK;
}

gm_status PointOutputs::reserve(gm_ctx *ctx, uint64_t n, uint32_t want, uint32_t hold)
{
    wanted = want;
    if (hold & kPtRes) GMW_HIP(ctx, res.reserve(n));
    if (hold & kPtCell) GMW_HIP(ctx, cell.reserve(n));
    if (hold & kPtDelta) GMW_HIP(ctx, delta.reserve(n));
    if (hold & kPtCls) GMW_HIP(ctx, cls.reserve(n));
    if (hold & kPtElement) GMW_HIP(ctx, element.reserve(n));
    return GM_OK;
}

gm_status PointOutputs::copy_back(gm_ctx *ctx, hipStream_t s, uint32_t n, float *h_res, int32_t *h_cell, int32_t *h_delta,
                                  uint8_t *h_cls, int32_t *h_element) const
{
    if (h_res && n) GMW_HIP(ctx, hipMemcpyAsync(h_res, res.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (h_cell && n) GMW_HIP(ctx, hipMemcpyAsync(h_cell, cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (h_delta && n) GMW_HIP(ctx, hipMemcpyAsync(h_delta, delta.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (h_cls && n) GMW_HIP(ctx, hipMemcpyAsync(h_cls, cls.p, (size_t)n, hipMemcpyDeviceToHost, s));
    if (h_element && n) GMW_HIP(ctx, hipMemcpyAsync(h_element, element.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return GM_OK;
}

gm_status StageCall::open()
{
    gm_ctx *ctx = map->ctx;
    GMW_OK(gm_begin_stage(ctx, sl));
    GMW_OK(gm_ensure_capacity(ctx, *sl, n ? n : 1u, (size_t)(n ? n : 1u) * 16, true));
    const uint32_t want = (residual ? kPtRes : 0u) | (cell ? kPtCell : 0u) | (delta ? kPtDelta : 0u) | (cls ? kPtCls : 0u) |
                          (element ? kPtElement : 0u);
    uint32_t hold = want;
    if (&out == &map->pt) {   // a map's own call holds residual with cell and delta with cls
        if (want & (kPtRes | kPtCell)) hold |= kPtRes | kPtCell;
        if (want & (kPtDelta | kPtCls)) hold |= kPtDelta | kPtCls;
    }
    return out.reserve(ctx, n, want, hold);
}

gm_status StageCall::upload(const float *xyz, const uint8_t *labels, WallArgs &w)
{
    gm_ctx *ctx = map->ctx;
    GMW_OK(gm_upload_xyz(ctx, *sl, xyz, n, sl->crop4));
    if (labels && n) GMW_HIP(ctx, hipMemcpyAsync(sl->labels, labels, n, hipMemcpyHostToDevice, sl->stream));
    w.pts = sl->crop4;
    w.labels = labels ? sl->labels : nullptr;
    w.n_ptr = nullptr;
    w.n_host = n;
    w.res = out.dev_res();
    w.cell = out.dev_cell();
    return GM_OK;
}

gm_status StageCall::close()
{
    gm_ctx *ctx = map->ctx;
    GMW_OK(out.copy_back(ctx, sl->stream, n, residual, cell, delta, cls, element));
    GMW_HIP(ctx, hipStreamSynchronize(sl->stream));
    return GM_OK;
}

gm_status add_wait_readers(gm_wall_map *m, uint32_t slot, hipStream_t s)
{
    for (uint32_t i = 0; i < m->ctx->n_slots; ++i)
        for (const PendingResult *r : {&m->checks[i].res, &m->locates[i].res, &m->aligns[i].res})
            if (i != slot && r->outstanding) GMW_HIP(m->ctx, hipStreamWaitEvent(s, r->done, 0));
    for (const std::vector<PendingResult> *al : {m->al_locates, m->al_checks, m->al_aligns})
        if (al)
            for (uint32_t i = 0; i < m->ctx->n_slots; ++i)
                if (i != slot && (*al)[i].outstanding) GMW_HIP(m->ctx, hipStreamWaitEvent(s, (*al)[i].done, 0));
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

namespace {

// every pending result of the map: the checks', the locates', the aligns', the checked adds'
template <class F>
gm_status each_result(gm_wall_map *m, F f)
{
    for (WallCheckSlot &c : m->checks) GMW_OK(f(c.res));
    for (WallLocateSlot &l : m->locates) GMW_OK(f(l.res));
    for (WallAlignSlot &l : m->aligns) GMW_OK(f(l.res));
    for (WallAddCheckedSlot &l : m->add_checks) GMW_OK(f(l.res));
    return GM_OK;
}

gm_status sync_map(gm_wall_map *m)
{
    gm_ctx *ctx = m->ctx;
    GMW_OK(set_device(ctx));
    for (uint32_t i = 0; i < ctx->n_slots; ++i)
        if (m->pending[i]) {
            GMW_HIP(ctx, hipStreamSynchronize(ctx->slots[i].stream));
            m->pending[i] = 0;
        }
    GMW_OK(each_result(m, [&](PendingResult &r) { return r.wait(ctx); }));
    GMW_HIP(ctx, hipStreamSynchronize(m->stream));
    return GM_OK;
}

gm_status check_window(gm_wall_map *m, uint32_t station0, uint32_t n, uint64_t capacity, uint64_t *n_out, const char *who)
{
    if ((uint64_t)station0 + n > m->prm.n_stations)
        return gm_fail(m->ctx, GM_ERR_INVALID_ARG, "gm_wall_map: the window leaves [0, n_stations]");
    const uint64_t nc = (uint64_t)n * m->prm.n_sectors;
    if (n_out) *n_out = nc;
    if (nc > capacity) return gm_fail(m->ctx, GM_ERR_CAPACITY, who);
    return GM_OK;
}

// the refusals of a baseline (NULL: none) in the call `who`: the map itself, another context, another grid
gm_status check_baseline(gm_wall_map *map, gm_wall_map *baseline, const char *who)
{
    if (!baseline) return GM_OK;
    gm_ctx *ctx = map->ctx;
    auto refuse = [&](const char *why) { return gm_fail(ctx, GM_ERR_INVALID_ARG, (std::string(who) + why).c_str()); };
    if (baseline == map) return refuse(": the baseline is the map itself");
    if (baseline->ctx != ctx) return refuse(": the baseline belongs to another context");
    const gm_wall_params &p = map->prm, &b = baseline->prm;
    if (p.n_stations != b.n_stations || p.n_sectors != b.n_sectors || memcmp(&p.station_length, &b.station_length, 8) ||
        memcmp(&p.t_min, &b.t_min, 8) || memcmp(p.point, b.point, 24) || memcmp(p.direction, b.direction, 24) ||
        memcmp(&p.radius, &b.radius, 8) || memcmp(p.up, b.up, 24) || memcmp(p.forward, b.forward, 24))
        return refuse(": the baseline is a map on another grid");
    if (memcmp(&map->arc, &baseline->arc, sizeof(gm_wall_arc))) return refuse(": the baseline is a map on another arc");
    if (memcmp(&map->clothoid, &baseline->clothoid, sizeof(gm_wall_clothoid))) return refuse(": the baseline is a map on another clothoid");
    return GM_OK;
}

}  // namespace

namespace gm {
namespace wall {

const char *region_prm_refusal(const gm_wall_region_params &p, long long &T)
{
    T = 0;
    if (p.struct_size != sizeof(gm_wall_region_params) || p.min_count < 1u || p.min_cells < 1u || (p.connectivity != 4u && p.connectivity != 8u) ||
        !(p.threshold > 0.0) || !(p.threshold <= 8.0))
        return ": struct_size mismatch or a parameter outside its limits";
    T = (long long)rint(p.threshold * 1048576.0);
    return T < 1 ? ": the threshold rounds to 0" : nullptr;
}

gm_status regions_run(gm_ctx *ctx, hipStream_t s, RegionScratch &rg, WallRegionArgs &a, int32_t *stage, uint64_t stage_labels,
                      gm_wall_regions_info *info, gm_wall_region *regions, uint32_t capacity, uint32_t *n_out, int32_t *cell_labels,
                      const char *who)
{
    const uint64_t total = (uint64_t)a.n * a.nsec;
    a.ts = rg.ts;
    a.tk = rg.tk;
    a.tiles_s = (a.n + a.ts - 1u) / a.ts;
    a.tiles_k = (a.nsec + a.tk - 1u) / a.tk;
    GMW_HIP(ctx, rg.cells.reserve(total * (8 + 4 + 4)));
    GMW_HIP(ctx, rg.ctr.reserve(kWallRegionCounters));
    Carve cells{rg.cells.p};
    a.d = cells.take<long long>(total);
    a.parent = cells.take<uint32_t>(total);
    a.slot = cells.take<uint32_t>(total);
    a.ctr = rg.ctr.p;
    unsigned long long ctr[kWallRegionCounters];
    GMW_HIP(ctx, hipMemsetAsync(a.ctr, 0, kWallRegionCounters * 8, s));
    launch_wall_region_label(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    GMW_HIP(ctx, hipStreamSynchronize(s));   // the one count the host needs: it sizes the records
    const uint64_t ncomp = ctr[4];
    info->flagged_pos = ctr[0]; info->flagged_neg = ctr[1]; info->unusable = ctr[2]; info->empty = ctr[3];
    info->components = ncomp;
    uint64_t nreg = 0;
    if (ncomp) {
        GMW_HIP(ctx, rg.recs.reserve(ncomp * (sizeof(WallRegionAcc) + sizeof(gm_wall_region))));
        Carve recs{rg.recs.p};
        a.acc = recs.take<WallRegionAcc>(ncomp);
        a.out = recs.take<gm_wall_region>(ncomp);
        a.ncomp = (uint32_t)ncomp;
        GMW_HIP(ctx, hipMemsetAsync(a.acc, 0, ncomp * sizeof(WallRegionAcc), s));
        launch_wall_region_reduce(a, s);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(&nreg, a.ctr + 5, 8, hipMemcpyDeviceToHost, s));
        GMW_HIP(ctx, hipStreamSynchronize(s));
    }
    info->regions = nreg;
    if (n_out) *n_out = (uint32_t)nreg;
    const bool fits = nreg <= capacity;
    if (regions && fits && nreg) {
        GMW_HIP(ctx, hipMemcpyAsync(regions, a.out, nreg * sizeof(gm_wall_region), hipMemcpyDeviceToHost, s));
        GMW_HIP(ctx, hipStreamSynchronize(s));
        std::sort(regions, regions + nreg, [](const gm_wall_region &x, const gm_wall_region &y) { return x.label < y.label; });
    }
    if (cell_labels) {
        for (uint64_t done = 0; done < total; done += stage_labels) {
            const uint64_t c = std::min(stage_labels, total - done);
            launch_wall_region_labels(a, done, c, stage, s);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(cell_labels + done, stage, c * 4, hipMemcpyDeviceToHost, s));
            GMW_HIP(ctx, hipStreamSynchronize(s));
        }
    }
    if (!fits && (regions || capacity)) return gm_fail(ctx, GM_ERR_CAPACITY, who);
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

namespace {

void free_map(gm_wall_map *m)
{
    gm_ctx *ctx = m->ctx;
    hipSetDevice(ctx->device);
    for (uint32_t i = 0; i < ctx->n_slots; ++i)
        if (m->pending[i] && ctx->slots[i].stream) hipStreamSynchronize(ctx->slots[i].stream);
    (void)each_result(m, [](PendingResult &r) { r.release(); return GM_OK; });
    for (hipEvent_t e : m->adds)
        if (e) hipEventDestroy(e);
    if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
    delete m;   // (every DevArray and HostArray goes with it)
}

// gm_wall_map_read (raw false: gm_surface_cell) and gm_wall_map_read_raw (gm_wall_raw_cell): the window in chunks of the
// staging buffer
gm_status read_window(gm_wall_map *m, uint32_t station0, uint32_t n, void *cells, uint64_t capacity, uint64_t *n_out, bool raw)
{
    if (!m) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = m->ctx;
    GMW_OK(check_window(m, station0, n, capacity, n_out,
                        raw ? "gm_wall_map_read_raw: cell buffer too small" : "gm_wall_map_read: cell buffer too small"));
    if (!n) return sync_map(m);
    if (!cells) return gm_fail(ctx, GM_ERR_INVALID_ARG, raw ? "gm_wall_map_read_raw: NULL cells" : "gm_wall_map_read: NULL cells");
    GMW_OK(sync_map(m));
    const uint64_t first = (uint64_t)station0 * m->prm.n_sectors, total = (uint64_t)n * m->prm.n_sectors;
    const size_t rec = raw ? sizeof(gm_wall_raw_cell) : sizeof(gm_surface_cell);
    for (uint64_t done = 0; done < total; done += kStageCells) {
        const uint64_t c = std::min(kStageCells, total - done);
        if (raw) launch_wall_read_raw(m->table, first + done, c, reinterpret_cast<gm_wall_raw_cell *>(m->stage.p), m->stream);
        else launch_wall_read(m->table, first + done, c, reinterpret_cast<gm_surface_cell *>(m->stage.p), m->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync((uint8_t *)cells + done * rec, m->stage.p, c * rec, hipMemcpyDeviceToHost, m->stream));
        GMW_HIP(ctx, hipStreamSynchronize(m->stream));
    }
    return GM_OK;
}

bool cloud_params_ok(const gm_wall_cloud_params &c)
{
    if (c.struct_size != sizeof(gm_wall_cloud_params) || c.block_stations < 1u || c.block_sectors < 1u || c.min_count < 1u) return false;
    if (!isfinite(c.exaggeration) || !(c.exaggeration >= 0.0)) return false;
    return isfinite(c.anchor[0]) && isfinite(c.anchor[1]) && isfinite(c.anchor[2]);
}

// the head of a cloud's info: the window and its block grid (bs, bk clamped to the window and the ring)
void cloud_info_head(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_cloud_params &cp, gm_wall_cloud_info *info)
{
    const uint32_t nsec = map->prm.n_sectors;
    const uint32_t bk = std::min(cp.block_sectors, nsec), bs = std::min(cp.block_stations, std::max(n, 1u));
    const uint32_t NK = (nsec + bk - 1u) / bk, NJ = (n + bs - 1u) / bs;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_cloud_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->blocks_stations = NJ;
    info->blocks_sectors = NK;
    info->blocks = (uint64_t)NJ * NK;
}

// gm_wall_map_mesh's vertex pass: the tables its emit step fills beside the records (k_wall_mesh.hip)
struct MeshTables { uint32_t *rank; float *mean; };

// The chunks of gm_wall_map_cloud over the window of `info` (cloud_info_head's, n_stations >= 1; the map synchronised):
// the records to points (may be NULL) while they fit capacity, the three class counts to info.  mesh (gm_wall_map_mesh):
// the same passes with the emit step that also fills the tables.
gm_status cloud_chunks(gm_wall_map *map, const gm_wall_cloud_params &cp, gm_wall_cloud_info *info, gm_wall_cloud_point *points,
                       uint64_t capacity, const MeshTables *mesh)
{
    gm_ctx *ctx = map->ctx;
    const uint32_t station0 = info->station0, n = info->n_stations, nsec = info->n_sectors;
    const uint32_t bk = std::min(cp.block_sectors, nsec), bs = std::min(cp.block_stations, n);
    const uint32_t NK = info->blocks_sectors, NJ = info->blocks_stations;

    // chunks of whole block rows
    const uint64_t chunk = map->cloud_chunk ? map->cloud_chunk : kStageCells;
    const uint32_t rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(chunk / NK, 1u), NJ);
    const uint64_t cb = (uint64_t)rows * NK;   // blocks of a full chunk
    const bool merged = bs > 1u || bk > 1u;
    const uint64_t acc_bytes = cb * kWallCloudAccBytes;
    if (merged) GMW_HIP(ctx, map->cl_acc.reserve(acc_bytes));
    GMW_HIP(ctx, map->cl_stage.reserve(cb));
    GMW_OK(map->cl_scan.reserve(ctx, (uint32_t)cb, map->stream));   // (nothing of the map's is in flight: the call synchronised above)
    GMW_HIP(ctx, map->cl_ctr.reserve(kWallCloudCounters));
    GMW_HIP(ctx, map->cl_dirs.reserve((uint64_t)GM_WALL_MAX_SECTORS * 2));
    map->cl_dirs_host.resize((size_t)2 * NK);
    cloud_directions(nsec, bk, map->cl_dirs_host.data());
    GMW_HIP(ctx, hipMemcpyAsync(map->cl_dirs.p, map->cl_dirs_host.data(), (size_t)NK * 16, hipMemcpyHostToDevice, map->stream));
    GMW_HIP(ctx, hipMemsetAsync(map->cl_ctr.p, 0, kWallCloudCounters * 8, map->stream));

    WallCloudArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.first = (uint64_t)station0 * nsec;
    a.station0 = station0; a.n = n; a.nsec = nsec;
    a.bs = bs; a.bk = bk; a.NK = NK;
    a.merged = merged ? 1u : 0u;
    a.min_count = cp.min_count;
    if (merged) {
        Carve acc{map->cl_acc.p};   // kWallCloudAccBytes per block
        a.acc_sum = acc.take<unsigned long long>(cb);
        a.acc_cnt = acc.take<unsigned long long>(cb);
        a.acc_lo = acc.take<uint32_t>(cb);
        a.acc_hi = acc.take<uint32_t>(cb);
        a.acc_cells = acc.take<uint32_t>(cb);
    }
    a.dirs = map->cl_dirs.p;
    const DesignFrame &d = map->axis.d;
    for (int k = 0; k < 3; ++k) {
        a.oa[k] = d.o[k] - cp.anchor[k];
        a.a[k] = d.a[k]; a.u[k] = d.u[k]; a.v[k] = d.v[k];
    }
    a.R = d.R;
    a.g = cp.exaggeration;
    a.t_min = map->prm.t_min;
    a.ds = map->prm.station_length;
    a.out = map->cl_stage.p;
    a.ctr = map->cl_ctr.p;
    // the position rule of a curved axis: its constants, and a table of the chunk's block rows (DesignAxis::row)
    const DesignAxis &axis = map->axis;
    const uint32_t rw = axis.row_width();
    WallCloudAxis ca;
    memset(&ca, 0, sizeof(ca));
    ca.kind = axis.kind;
    if (rw) {
        GMW_HIP(ctx, map->cl_rows.reserve((uint64_t)rows * rw));
        map->cl_rows_host.resize((size_t)rows * rw);
        ca.arc.rows = map->cl_rows.p;
        for (int k = 0; k < 3; ++k) { ca.arc.ca[k] = axis.arc.C[k] - cp.anchor[k]; ca.arc.n[k] = axis.n[k]; ca.arc.b[k] = axis.b[k]; }
        ca.arc.inv_kappa = axis.arc.inv_kappa;
        ca.arc.un = axis.un; ca.arc.ub = axis.ub; ca.arc.vn = axis.vn; ca.arc.vb = axis.vb;
    }

    uint64_t total = 0;
    unsigned long long ctr[kWallCloudCounters] = {0ull, 0ull, 0ull, 0ull};
    bool copying = points != nullptr;
    for (uint32_t J0 = 0; J0 < NJ; J0 += rows) {   // (the trip count depends on the window alone)
        a.J0 = J0;
        a.nJ = std::min(rows, NJ - J0);
        if (merged) {
            GMW_HIP(ctx, hipMemsetAsync(map->cl_acc.p, 0, acc_bytes, map->stream));
            launch_wall_cloud_merge(a, map->stream);
            GMW_HIP(ctx, hipGetLastError());
        }
        if (rw) {   // the rows at their centre chainages: tc by the emit step's rule
            for (uint32_t jl = 0; jl < a.nJ; ++jl) {
                const uint32_t jw = (J0 + jl) * bs, ns = std::min(n - jw, bs);
                const double h = (double)(2u * (station0 + jw) + ns) * 0.5;
                axis.row(a.t_min + h * a.ds, cp.anchor, &map->cl_rows_host[(size_t)rw * jl]);
            }   // (the last chunk's copy has been waited for: every trip ends with a synchronisation)
            GMW_HIP(ctx, hipMemcpyAsync(map->cl_rows.p, map->cl_rows_host.data(), (size_t)a.nJ * rw * 8, hipMemcpyHostToDevice,
                                        map->stream));
        }
        const ScanState st = map->cl_scan.next(map->stream);
        if (mesh) launch_wall_mesh_vertices(a, ca, mesh->rank, mesh->mean, (uint32_t)total, st, map->stream);
        else launch_wall_cloud_compact(a, ca, st, map->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        const uint64_t got = (uint32_t)ctr[2];
        if (copying && total + got > capacity) copying = false;   // copying stops, counting goes on
        if (copying && got) {
            GMW_HIP(ctx, hipMemcpyAsync(points + total, a.out, got * sizeof(gm_wall_cloud_point), hipMemcpyDeviceToHost,
                                        map->stream));
            GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        }
        total += got;
    }
    info->points = total;
    info->empty = ctr[0];
    info->below_min_count = ctr[1];
    return GM_OK;
}

}  // namespace

namespace gm {
void gm_wall_free_all(gm_ctx *ctx)
{
    gm_wall_alignment_free_all(ctx);
    for (gm_wall_map *m : ctx->walls) free_map(m);
    ctx->walls.clear();
}
}  // namespace gm

extern "C" {

// gm_wall_map_create (arc and cl NULL), gm_wall_map_create_arc and gm_wall_map_create_clothoid
static gm_status create_map(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_arc *arc, const gm_wall_clothoid *cl,
                            gm_wall_map **map)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!map) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create: NULL map");
    *map = nullptr;
    if (check_params(params) != GM_OK)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create: NULL, struct_size mismatch or a parameter outside its limits");
    DesignAxis axis;
    const gm_status ast = axis_check(params, arc, cl, axis);
    if (ast == GM_ERR_OOM) return gm_fail(ctx, GM_ERR_OOM, "gm_wall_map_create_clothoid: no memory for the table of station starts");
    if (ast != GM_OK)
        return gm_fail(ctx, GM_ERR_INVALID_ARG,
                       arc ? "gm_wall_map_create_arc: struct_size mismatch, or a curvature outside its limits for this map"
                           : "gm_wall_map_create_clothoid: struct_size mismatch, or a normal, curvature or rate outside its limits for this map");
    GMW_OK(set_device(ctx));
    gm_wall_map *m = new gm_wall_map;
    m->axis = std::move(axis);
    m->ctx = ctx;
    m->prm = *params;
    m->ncell = (uint64_t)params->n_stations * params->n_sectors;
    m->pending.assign(ctx->n_slots, 0);
    m->adds.assign(ctx->n_slots, nullptr);
    m->checks.resize(ctx->n_slots);
    m->locates.resize(ctx->n_slots);
    m->aligns.resize(ctx->n_slots);
    m->add_checks.resize(ctx->n_slots);
    if (const char *e = getenv("GM_WALL_ALIGN_ROWS")) m->align_rows = (uint32_t)strtoul(e, nullptr, 10);   // 0: the default
    if (const char *e = getenv("GM_WALL_POINTS_PER_BLOCK")) m->points_per_block = (uint32_t)strtoul(e, nullptr, 10);
    if (const char *e = getenv("GM_WALL_REGION_TILE")) {   // <stations>x<sectors>; anything else: the default
        unsigned ts = 0, tk = 0;
        if (sscanf(e, "%ux%u", &ts, &tk) == 2 && ts >= 1u && tk >= 1u && (uint64_t)ts * tk <= kWallRegionTileCells) {
            m->rg.ts = ts;
            m->rg.tk = tk;
        }
    }
    m->ob.read_tile_env();
    if (const char *e = getenv("GM_WALL_CLOUD_CHUNK")) {   // blocks; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->cloud_chunk = v < kStageCells ? (uint32_t)v : 0u;
    }
    if (const char *e = getenv("GM_WALL_SECTION_CHUNK")) {   // sections; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->section_chunk = v < kSectionChunk ? (uint32_t)v : 0u;
    }
    if (const char *e = getenv("GM_WALL_CLEAR_CHUNK")) {   // cells; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->clear_chunk = v < kStageCells ? (uint32_t)v : 0u;
    }
    if (const char *e = getenv("GM_WALL_QUANTITY_CHUNK")) {   // sections; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->quantity_chunk = v < kStageBytes ? (uint32_t)v : 0u;
    }
    memset(&m->arc, 0, sizeof(m->arc));
    m->arc.struct_size = (uint32_t)sizeof(gm_wall_arc);
    if (arc) { m->arc = *arc; m->arc.reserved = 0u; }
    memset(&m->clothoid, 0, sizeof(m->clothoid));
    if (cl) m->clothoid = *cl;
    auto body = [&]() -> gm_status {
        GMW_HIP(ctx, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
        GMW_HIP(ctx, m->base.reserve(wall_table_bytes(m->ncell)));
        GMW_HIP(ctx, m->stage.reserve(std::min(kStageCells, m->ncell) * sizeof(gm_wall_raw_cell)));
        GMW_HIP(ctx, hipMemsetAsync(m->base.p, 0, wall_table_bytes(m->ncell), m->stream));
        GMW_HIP(ctx, hipStreamSynchronize(m->stream));
        return GM_OK;
    };
    const gm_status st = body();
    if (st != GM_OK) {
        (void)hipGetLastError();
        free_map(m);
        return st;
    }
    m->table = wall_table(m->base.p, m->ncell);
    ctx->walls.push_back(m);
    *map = m;
    return GM_OK;
}

gm_status gm_wall_map_create(gm_ctx *ctx, const gm_wall_params *params, gm_wall_map **map)
{
    return create_map(ctx, params, nullptr, nullptr, map);
}

gm_status gm_wall_map_create_arc(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_arc *arc, gm_wall_map **map)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (map) *map = nullptr;
    if (!arc) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create_arc: NULL arc");
    return create_map(ctx, params, arc, nullptr, map);
}

gm_status gm_wall_map_create_clothoid(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_clothoid *clothoid, gm_wall_map **map)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (map) *map = nullptr;
    if (!clothoid) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create_clothoid: NULL clothoid");
    return create_map(ctx, params, nullptr, clothoid, map);
}

gm_status gm_wall_map_get_clothoid(gm_wall_map *map, gm_wall_clothoid *clothoid)
{
    if (!map || !clothoid) return GM_ERR_INVALID_ARG;
    *clothoid = map->clothoid;
    return GM_OK;
}

gm_status gm_wall_map_get_arc(gm_wall_map *map, gm_wall_arc *arc)
{
    if (!map || !arc) return GM_ERR_INVALID_ARG;
    *arc = map->arc;
    return GM_OK;
}

void gm_wall_map_destroy(gm_wall_map *map)
{
    if (!map) return;
    std::vector<gm_wall_map *> &w = map->ctx->walls;
    w.erase(std::remove(w.begin(), w.end(), map), w.end());
    free_map(map);
}

gm_status gm_wall_map_add_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12], gm_wall_add_info *add_info)
{
    Slot *sl = nullptr;
    GMW_OK(frame_call_head(map, ctx, slot, "gm_wall_map_add_frame", [] { return true; }, sl));
    WallArgs w;
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, w, nullptr, &ax));
    GMW_OK(set_device(ctx));
    frame_points(ctx, *sl, w);
    GMW_OK(add_wait_readers(map, slot, sl->stream));
    launch_wall_add(w, ax, nullptr, nullptr, sl->n_in, map->points_per_block, sl->stream);
    GMW_HIP(ctx, hipGetLastError());
    map->pending[slot] = 1;
    ++map->frames;
    return GM_OK;
}

gm_status gm_wall_map_add_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                 gm_wall_add_info *add_info, float *residual, int32_t *cell)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n && !xyz) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_points: NULL xyz");
    WallArgs w;
    WallAxis ax;
    GMW_OK(add_frame_args(map, pose, add_info, w, nullptr, &ax));
    StageCall sc{map, n, map->pt, residual, cell, nullptr, nullptr, nullptr};
    GMW_OK(sc.open());
    GMW_OK(sc.upload(xyz, labels, w));
    hipStream_t s = sc.sl->stream;
    GMW_OK(add_wait_readers(map, 0, s));   // (as gm_wall_map_add_frame; the staging slot is slot 0)
    launch_wall_add(w, ax, nullptr, nullptr, n, map->points_per_block, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_OK(sc.close());
    ++map->frames;
    return GM_OK;
}

gm_status gm_wall_map_sync(gm_wall_map *map)
{
    if (!map) return GM_ERR_INVALID_ARG;
    return sync_map(map);
}

gm_status gm_wall_map_info(gm_wall_map *map, gm_wall_info *info)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_info: NULL info");
    GMW_OK(sync_map(map));
    unsigned long long tot[kWallTotals];
    GMW_HIP(ctx, hipMemsetAsync(map->table.totals + 4, 0, 8, map->stream));
    launch_wall_count(map->table, map->ncell, map->stream);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(tot, map->table.totals, sizeof(tot), hipMemcpyDeviceToHost, map->stream));
    GMW_HIP(ctx, hipStreamSynchronize(map->stream));
    const DesignFrame &d = map->axis.d;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_info);
    info->status = d.status;
    info->n_stations = map->prm.n_stations;
    info->n_sectors = map->prm.n_sectors;
    info->frames = map->frames;
    info->mapped = tot[0]; info->outside = tot[1]; info->beyond_gate = tot[2]; info->plane = tot[3];
    info->cells_hit = tot[4];
    for (int k = 0; k < 3; ++k) { info->o[k] = d.o[k]; info->a[k] = d.a[k]; info->u[k] = d.u[k]; info->v[k] = d.v[k]; }
    info->R = d.R;
    return GM_OK;
}

gm_status gm_wall_map_read(gm_wall_map *map, uint32_t station0, uint32_t n, gm_surface_cell *cells, uint64_t capacity,
                           uint64_t *n_out)
{
    return read_window(map, station0, n, cells, capacity, n_out, false);
}

gm_status gm_wall_map_read_raw(gm_wall_map *map, uint32_t station0, uint32_t n, gm_wall_raw_cell *cells, uint64_t capacity,
                               uint64_t *n_out)
{
    return read_window(map, station0, n, cells, capacity, n_out, true);
}

gm_status gm_wall_map_add_raw(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_raw_cell *cells)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    if (n && !cells) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_raw: NULL cells");
    GMW_OK(sync_map(map));
    const uint64_t first = (uint64_t)station0 * map->prm.n_sectors, total = (uint64_t)n * map->prm.n_sectors;
    for (uint64_t done = 0; done < total; done += kStageCells) {
        const uint64_t c = std::min(kStageCells, total - done);
        GMW_HIP(ctx, hipMemcpyAsync(map->stage.p, cells + done, c * sizeof(gm_wall_raw_cell), hipMemcpyHostToDevice, map->stream));
        launch_wall_merge_raw(map->table, first + done, c, reinterpret_cast<const gm_wall_raw_cell *>(map->stage.p), map->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
    }
    return GM_OK;
}

gm_status gm_wall_map_clear(gm_wall_map *map, uint32_t station0, uint32_t n)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    const bool all = station0 == 0 && n == map->prm.n_stations;
    launch_wall_clear(map->table, (uint64_t)station0 * map->prm.n_sectors, (uint64_t)n * map->prm.n_sectors, all, map->stream);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipStreamSynchronize(map->stream));
    if (all) map->frames = 0;
    return GM_OK;
}

gm_status gm_wall_map_regions(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n,
                              const gm_wall_region_params *prm, gm_wall_regions_info *info, gm_wall_region *regions,
                              uint32_t capacity, uint32_t *n_out, int32_t *cell_labels)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: NULL info");
    const gm_wall_region_params rp = params_or(prm, gm_wall_region_default_params);
    long long T = 0;
    if (const char *why = region_prm_refusal(rp, T)) return gm_fail(ctx, GM_ERR_INVALID_ARG, (std::string("gm_wall_map_regions") + why).c_str());
    if (!regions && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: NULL regions with a capacity");
    GMW_OK(check_baseline(map, baseline, "gm_wall_map_regions"));
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    if (baseline) GMW_OK(sync_map(baseline));
    const uint32_t nsec = map->prm.n_sectors;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_regions_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->threshold_q = T;
    info->cell_area = map->prm.station_length * map->prm.radius * kTwoPi / (double)nsec;
    if (!n) return GM_OK;

    WallRegionArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.has_base = baseline ? 1u : 0u;
    a.base = baseline ? baseline->table : map->table;
    a.n = n;
    a.nsec = nsec;
    a.first = (uint64_t)station0 * nsec;
    a.conn8 = rp.connectivity == 8u ? 1u : 0u;
    a.min_count = rp.min_count;
    a.min_cells = rp.min_cells;
    a.T = T;
    // (kStageCells raw records of staging: room for as many labels)
    return regions_run(ctx, map->stream, map->rg, a, reinterpret_cast<int32_t *>(map->stage.p), std::min(kStageCells, map->ncell), info,
                       regions, capacity, n_out, cell_labels, "gm_wall_map_regions: region buffer too small");
}

gm_status gm_wall_map_cloud(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_cloud_params *prm,
                            gm_wall_cloud_info *info, gm_wall_cloud_point *points, uint64_t capacity, uint64_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_cloud: NULL info");
    const gm_wall_cloud_params cp = params_or(prm, gm_wall_cloud_default_params);
    if (!cloud_params_ok(cp))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_cloud: struct_size mismatch or a parameter outside its limits");
    if (!points && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_cloud: NULL points with a capacity");
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    cloud_info_head(map, station0, n, cp, info);
    if (!n) return GM_OK;
    GMW_OK(cloud_chunks(map, cp, info, points, capacity, nullptr));
    if (n_out) *n_out = info->points;
    if (points && info->points > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_cloud: point buffer too small");
    return GM_OK;
}

gm_status gm_wall_map_mesh(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_mesh_params *prm,
                           gm_wall_mesh_info *info, gm_wall_cloud_point *vertices, uint64_t vertex_capacity,
                           gm_wall_mesh_triangle *triangles, uint64_t triangle_capacity, uint64_t *n_vertices,
                           uint64_t *n_triangles)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_vertices) *n_vertices = 0;
    if (n_triangles) *n_triangles = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_mesh: NULL info");
    const gm_wall_mesh_params mp = params_or(prm, gm_wall_mesh_default_params);
    if (mp.struct_size != sizeof(gm_wall_mesh_params) || mp.reserved || !mesh_rule_ok(mp.flags, mp.max_step) || !cloud_params_ok(mp.cloud))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_mesh: struct_size mismatch, an unknown flag or a parameter outside its limits");
    if ((!vertices && vertex_capacity) || (!triangles && triangle_capacity))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_mesh: NULL vertices or triangles with a capacity");
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_mesh_info);
    cloud_info_head(map, station0, n, mp.cloud, &info->cloud);
    const uint32_t NJ = info->cloud.blocks_stations, NK = info->cloud.blocks_sectors;
    const MeshGrid g = mesh_grid(NJ, NK, mp.flags);
    info->wrapped = g.wrapped;
    info->quads = g.quads;
    if (!n) return GM_OK;

    // 1. the vertices: the cloud's chunks, with the index (and, for a step cut, the mean) of every survivor on the side
    const uint64_t nb = info->cloud.blocks;   // <= 2^24
    const bool cutting = mp.max_step > 0.0;
    GMW_HIP(ctx, map->ms_rank.reserve(nb));
    if (cutting) GMW_HIP(ctx, map->ms_mean.reserve(nb));
    GMW_HIP(ctx, hipMemsetAsync(map->ms_rank.p, 0xFF, nb * sizeof(uint32_t), map->stream));   // kWallMeshDead everywhere
    const MeshTables tables{map->ms_rank.p, cutting ? map->ms_mean.p : nullptr};
    GMW_OK(cloud_chunks(map, mp.cloud, &info->cloud, vertices, vertex_capacity, &tables));
    const uint64_t nv = info->cloud.points;
    if (n_vertices) *n_vertices = nv;

    // 2. the triangles: chunks of as many whole quad rows as a vertex chunk has block rows
    uint64_t total = 0;
    unsigned long long ctr[kWallMeshCounters] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (g.quads) {
        const uint64_t chunk = map->cloud_chunk ? map->cloud_chunk : kStageCells;
        const uint32_t rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(chunk / NK, 1u), NJ - 1u);
        const uint64_t slots = 2ull * rows * g.NKq;   // of a full chunk, <= 2^21
        GMW_HIP(ctx, map->ms_stage.reserve(slots));
        GMW_OK(map->ms_scan.reserve(ctx, (uint32_t)slots, map->stream));   // (nothing of the map's is in flight: the call synchronised above)
        GMW_HIP(ctx, map->ms_ctr.reserve(kWallMeshCounters));
        GMW_HIP(ctx, hipMemsetAsync(map->ms_ctr.p, 0, kWallMeshCounters * 8, map->stream));
        WallMeshArgs a;
        memset(&a, 0, sizeof(a));
        a.rank = tables.rank;
        a.mean = tables.mean;
        a.NK = NK; a.NKq = g.NKq;
        a.outward = (mp.flags & GM_WALL_MESH_OUTWARD) ? 1u : 0u;
        a.max_step = (float)mp.max_step;
        a.out = map->ms_stage.p;
        a.ctr = map->ms_ctr.p;
        bool copying = triangles != nullptr;
        for (uint32_t J0 = 0; J0 < NJ - 1u; J0 += rows) {   // (the trip count depends on the window alone)
            a.Q0 = J0 * g.NKq;
            a.nq = std::min(rows, NJ - 1u - J0) * g.NKq;
            launch_wall_mesh_triangles(a, map->ms_scan.next(map->stream), map->stream);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, map->stream));
            GMW_HIP(ctx, hipStreamSynchronize(map->stream));
            const uint64_t got = (uint32_t)ctr[4];
            if (copying && total + got > triangle_capacity) copying = false;   // copying stops, counting goes on
            if (copying && got) {
                GMW_HIP(ctx, hipMemcpyAsync(triangles + total, a.out, got * sizeof(gm_wall_mesh_triangle), hipMemcpyDeviceToHost,
                                            map->stream));
                GMW_HIP(ctx, hipStreamSynchronize(map->stream));
            }
            total += got;
        }
    }
    info->quads_two = ctr[0];
    info->quads_one = ctr[1];
    info->quads_none = ctr[2];
    info->cut_by_step = ctr[3];
    info->triangles = total;
    if (n_triangles) *n_triangles = total;
    if ((vertices && nv > vertex_capacity) || (triangles && total > triangle_capacity))
        return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_mesh: vertex or triangle buffer too small");
    return GM_OK;
}

gm_status gm_wall_map_clearance(gm_wall_map *map, uint32_t station0, uint32_t n, const int32_t *gauge_q, uint32_t n_gauges,
                                const uint8_t *station_gauge, const gm_wall_clearance_params *prm, gm_wall_clearance_info *info,
                                gm_wall_clearance_station *stations, uint32_t station_capacity, gm_wall_clearance_cell *cells,
                                uint64_t cell_capacity, uint64_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_clearance: NULL info");
    const gm_wall_clearance_params cp = params_or(prm, gm_wall_clearance_default_params);
    if ((uint64_t)station0 + n > map->prm.n_stations)   // (before the tables: station_gauge has n entries)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: the window leaves [0, n_stations]");
    long long T, Rq;
    if (!clearance_ok(&map->prm, cp, gauge_q, n_gauges, station_gauge, n, T, Rq))
        return gm_fail(ctx, GM_ERR_INVALID_ARG,
                       "gm_wall_map_clearance: struct_size mismatch, a parameter outside its limits, a bad gauge table or a radius above 4096 m");
    if ((!stations && station_capacity) || (!cells && cell_capacity))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_clearance: NULL stations or cells with a capacity");
    GMW_OK(sync_map(map));
    const uint32_t nsec = map->prm.n_sectors;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_clearance_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->margin_q = T;
    info->radius_q = Rq;
    info->min_clearance = INT64_MAX;
    info->min_cell = UINT32_MAX;
    if (!n) return GM_OK;

    // chunks of whole stations
    const uint64_t chunk = map->clear_chunk ? map->clear_chunk : kStageCells;
    const uint32_t rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(chunk / nsec, 1u), n);
    const uint64_t cc = (uint64_t)rows * nsec;   // cells of a full chunk, <= 2^20
    const size_t entries = (size_t)n_gauges * nsec;
    GMW_HIP(ctx, map->cr_gauge.reserve(entries));
    if (station_gauge) GMW_HIP(ctx, map->cr_station_gauge.reserve(n));
    GMW_HIP(ctx, map->cr_stations.reserve(n));
    GMW_HIP(ctx, map->cr_ctr.reserve(kWallClearCounters));
    GMW_HIP(ctx, hipMemcpyAsync(map->cr_gauge.p, gauge_q, entries * sizeof(int32_t), hipMemcpyHostToDevice, map->stream));
    if (station_gauge) GMW_HIP(ctx, hipMemcpyAsync(map->cr_station_gauge.p, station_gauge, n, hipMemcpyHostToDevice, map->stream));
    GMW_HIP(ctx, hipMemsetAsync(map->cr_ctr.p, 0, kWallClearCounters * 8, map->stream));

    WallClearArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.first = (uint64_t)station0 * nsec;
    a.n = n; a.nsec = nsec;
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    a.T = T; a.Rq = Rq;
    a.gauge = map->cr_gauge.p;
    a.station_gauge = station_gauge ? map->cr_station_gauge.p : nullptr;
    a.stations = map->cr_stations.p;
    a.ctr = map->cr_ctr.p;

    unsigned long long ctr[kWallClearCounters];
    launch_wall_clear_stations(a, map->stream);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, map->stream));
    GMW_HIP(ctx, hipStreamSynchronize(map->stream));   // (the tables have left the caller's buffers, too)
    info->ungauged = ctr[kWallClearUngauged];
    info->empty = ctr[kWallClearEmpty];
    info->unusable = ctr[kWallClearUnusable];
    info->infringed = ctr[kWallClearInfringed];
    info->tight = ctr[kWallClearTight];
    info->clear = ctr[kWallClearClear];
    info->stations_tight = (uint32_t)ctr[6];
    info->stations_infringed = (uint32_t)ctr[7];
    if (ctr[8]) {
        const unsigned long long key = ~ctr[8];
        info->min_clearance = (long long)(key >> 24) - kWallClearBias;
        info->min_cell = (uint32_t)(key & 0xFFFFFFull);
    }
    const uint64_t total = info->tight + info->infringed;
    if (n_out) *n_out = total;
    if ((stations && station_capacity < n) || (cells && total > cell_capacity))
        return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_clearance: station or cell buffer too small");
    if (stations) {
        GMW_HIP(ctx, hipMemcpyAsync(stations, a.stations, (size_t)n * sizeof(gm_wall_clearance_station), hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
    }
    if (!cells || !total) return GM_OK;

    GMW_HIP(ctx, map->cr_stage.reserve(cc));
    GMW_OK(map->cr_scan.reserve(ctx, (uint32_t)cc, map->stream));   // (nothing of the map's is in flight: the call synchronised above)
    a.out = map->cr_stage.p;
    uint64_t done = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += rows) {   // (the trip count depends on the window alone)
        a.j0 = j0;
        a.nj = std::min(rows, n - j0);
        launch_wall_clear_list(a, map->cr_scan.next(map->stream), map->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(&ctr[9], a.ctr + 9, 8, hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        const uint64_t got = (uint32_t)ctr[9];
        if (done + got > total) return gm_fail(ctx, GM_ERR_DEVICE, "gm_wall_map_clearance: the list disagrees with the totals");
        if (got) {
            GMW_HIP(ctx, hipMemcpyAsync(cells + done, a.out, got * sizeof(gm_wall_clearance_cell), hipMemcpyDeviceToHost, map->stream));
            GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        }
        done += got;
    }
    if (done != total) return gm_fail(ctx, GM_ERR_DEVICE, "gm_wall_map_clearance: the list disagrees with the totals");
    return GM_OK;
}

gm_status gm_wall_map_sections(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n,
                               const gm_wall_section_params *prm, gm_wall_sections_info *info, gm_wall_section *sections,
                               uint32_t capacity, uint32_t *n_out, gm_wall_section_sums *sums)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_sections: NULL info");
    const gm_wall_section_params sp = params_or(prm, gm_wall_section_default_params);
    long long Tr;
    if (!section_prm_ok(sp, Tr))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_sections: struct_size mismatch or a parameter outside its limits");
    if (!sections && (capacity || sums))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_sections: NULL sections with a capacity or with sums");
    GMW_OK(check_baseline(map, baseline, "gm_wall_map_sections"));
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    if (baseline) GMW_OK(sync_map(baseline));
    const uint32_t nsec = map->prm.n_sectors, S = sp.section_stations, H = sp.harmonics, P = 1u + 2u * H, Pf = sp.passes;
    const uint32_t NS = n ? (n - 1u) / S + 1u : 0u;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_sections_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->section_stations = S;
    info->sections = NS;
    info->harmonics = H;
    info->passes = Pf;
    info->reject_q = Tr;
    info->max_gap_sectors = (uint32_t)floor(sp.max_gap_deg * (double)nsec / 360.0);
    if (n_out) *n_out = NS;
    if (!n) return GM_OK;
    if (sections && capacity < NS) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_sections: section buffer too small");

    const uint32_t cs = std::min(map->section_chunk ? map->section_chunk : kSectionChunk, NS);   // sections of a full chunk
    GMW_HIP(ctx, map->sc_basis.reserve((uint64_t)nsec * P));
    GMW_HIP(ctx, map->sc_chunk.reserve((uint64_t)cs * (sizeof(WallSectionModel) + sizeof(WallSectionOut))));
    map->sc_basis_host.resize((size_t)nsec * P);
    section_basis(nsec, H, map->sc_basis_host.data());
    GMW_HIP(ctx, hipMemcpyAsync(map->sc_basis.p, map->sc_basis_host.data(), (size_t)nsec * P * sizeof(int32_t), hipMemcpyHostToDevice,
                                map->stream));
    Carve chunk{map->sc_chunk.p};
    WallSectionArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.has_base = baseline ? 1u : 0u;
    a.base = baseline ? baseline->table : map->table;
    a.n = n; a.nsec = nsec;
    a.first = (uint64_t)station0 * nsec;
    a.S = S; a.P = P;
    a.min_count = sp.min_count;
    a.basis = map->sc_basis.p;
    WallSectionModel *d_model = chunk.take<WallSectionModel>(cs);
    WallSectionOut *d_out = chunk.take<WallSectionOut>(cs);
    a.model = d_model;
    a.out = d_out;

    std::vector<WallSectionModel> &model = map->sc_model_host;
    std::vector<WallSectionOut> &out = map->sc_out_host;
    std::vector<gm_wall_section> rec;
    for (uint32_t sec0 = 0; sec0 < NS; sec0 += cs) {   // (the trip count depends on the window alone)
        const uint32_t ns = std::min(cs, NS - sec0);
        a.sec0 = sec0;
        a.nsect = ns;
        WallSectionModel fresh;
        memset(&fresh, 0, sizeof(fresh));
        fresh.alive = 1;
        model.assign(ns, fresh);
        out.resize(ns);
        gm_wall_section zero;
        memset(&zero, 0, sizeof(zero));
        rec.assign(ns, zero);
        uint32_t alive = ns;
        for (uint32_t pass = 1; pass <= Pf + 1u && alive; ++pass) {   // Pf fitting passes, then the evaluation
            const bool eval = pass == Pf + 1u;
            a.fit = eval ? 0u : 1u;
            a.thr = pass == 1u ? INT64_MAX : (eval ? Tr : Tr << (Pf - pass));
            GMW_HIP(ctx, hipMemcpyAsync(d_model, model.data(), (size_t)ns * sizeof(WallSectionModel), hipMemcpyHostToDevice, map->stream));
            launch_wall_sections(a, map->stream);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(out.data(), d_out, (size_t)ns * sizeof(WallSectionOut), hipMemcpyDeviceToHost, map->stream));
            GMW_HIP(ctx, hipStreamSynchronize(map->stream));
            for (uint32_t i = 0; i < ns; ++i) {
                if (!model[i].alive) continue;
                const WallSectionOut &o = out[i];
                gm_wall_section &r = rec[i];
                if (pass == 1u) {
                    r.usable = o.usable;
                    info->empty += o.empty;
                    info->unusable += o.unusable;
                    info->usable += o.usable;
                }
                if (eval) {
                    r.accepted = o.sums.fitted;
                    r.rejected = r.usable - r.accepted;
                    r.points = o.sums.points;
                    r.rss = o.rss;
                    r.peak_out = o.peak_out;
                    r.peak_in = o.peak_in;
                    r.peak_out_sector = o.peak_out_sector;
                    r.peak_in_sector = o.peak_in_sector;
                    continue;
                }
                r.fitted = o.sums.fitted;
                r.largest_gap = o.sums.largest_gap;
                if (sums) sums[sec0 + i] = o.sums;
                r.status = section_solve(o.sums, H, sp.min_columns, r.coef_q);   // (a failed solve leaves the coefficients 0)
                if (r.status) {
                    model[i].alive = 0;
                    --alive;
                }
                memcpy(model[i].c, r.coef_q, sizeof(r.coef_q));
            }
        }
        for (uint32_t i = 0; i < ns; ++i) {
            gm_wall_section &r = rec[i];
            const uint32_t j0 = (sec0 + i) * S;   // < n
            r.station_from = station0 + j0;
            r.stations = n - j0 < S ? n - j0 : S;
            if (r.status) {
                r.peak_out_sector = r.peak_in_sector = UINT32_MAX;
                ++info->sections_failed;
            } else {
                ++info->sections_ok;
                info->accepted += r.accepted;
                info->rejected += r.rejected;
            }
            if (r.largest_gap > info->max_gap_sectors) {
                r.status |= GM_SECTION_OPEN_ARC;
                ++info->sections_open_arc;
            }
        }
        if (sections) memcpy(sections + sec0, rec.data(), (size_t)ns * sizeof(gm_wall_section));
    }
    return GM_OK;
}

gm_status gm_wall_map_quantities(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n, const int32_t *lo_q,
                                 const int32_t *hi_q, uint32_t n_profiles, const uint8_t *section_profile,
                                 const uint8_t *zone, uint32_t n_zones, const gm_wall_quantity_params *prm,
                                 gm_wall_quantities_info *info, gm_wall_quantity *records, uint32_t capacity, uint32_t *n_out,
                                 int32_t *profile_rows)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_quantities: NULL info");
    const gm_wall_quantity_params qp = params_or(prm, gm_wall_quantity_default_params);
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));   // (before the tables: section_profile has ceil(n / S) entries)
    long long Rq;
    if (!quantity_ok(&map->prm, qp, lo_q, hi_q, n_profiles, section_profile, n, zone, n_zones, Rq))
        return gm_fail(ctx, GM_ERR_INVALID_ARG,
                       "gm_wall_map_quantities: struct_size mismatch, a parameter outside its limits, a bad line, profile or zone table or a radius above 4096 m");
    if (!records && (capacity || profile_rows))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_quantities: NULL records with a capacity or with profile rows");
    GMW_OK(check_baseline(map, baseline, "gm_wall_map_quantities"));
    GMW_OK(sync_map(map));
    if (baseline) GMW_OK(sync_map(baseline));
    const uint32_t nsec = map->prm.n_sectors, S = qp.section_stations;
    const uint32_t NS = n ? (n - 1u) / S + 1u : 0u;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_quantities_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->section_stations = S;
    info->sections = NS;
    info->n_zones = n_zones;
    info->n_profiles = n_profiles;
    info->radius_q = Rq;
    const uint32_t total = NS * n_zones;   // <= 2^24 8
    if (n_out) *n_out = total;
    if (!n) return GM_OK;

    // chunks of whole sections: the staging of a full one stays within kStageBytes
    const uint64_t per_section = (uint64_t)n_zones * sizeof(gm_wall_quantity) + (profile_rows ? (uint64_t)nsec * sizeof(int32_t) : 0u);
    const uint32_t fit = (uint32_t)std::max<uint64_t>(kStageBytes / per_section, 1u);
    const uint32_t cs = std::min(map->quantity_chunk ? std::min(map->quantity_chunk, fit) : fit, NS);   // sections of a full chunk
    const size_t entries = (size_t)n_profiles * nsec;
    GMW_HIP(ctx, map->qt_lines.reserve(2u * entries));
    GMW_HIP(ctx, map->qt_index.reserve((uint64_t)NS + nsec));
    GMW_HIP(ctx, map->qt_stage.reserve((uint64_t)cs * per_section));
    GMW_HIP(ctx, map->qt_ctr.reserve(kWallQuantityCounters));
    int32_t *d_lo = map->qt_lines.p, *d_hi = map->qt_lines.p + entries;
    uint8_t *d_profile = map->qt_index.p, *d_zone = map->qt_index.p + NS;
    GMW_HIP(ctx, hipMemcpyAsync(d_lo, lo_q, entries * sizeof(int32_t), hipMemcpyHostToDevice, map->stream));
    GMW_HIP(ctx, hipMemcpyAsync(d_hi, hi_q, entries * sizeof(int32_t), hipMemcpyHostToDevice, map->stream));
    if (section_profile) GMW_HIP(ctx, hipMemcpyAsync(d_profile, section_profile, NS, hipMemcpyHostToDevice, map->stream));
    if (zone) GMW_HIP(ctx, hipMemcpyAsync(d_zone, zone, nsec, hipMemcpyHostToDevice, map->stream));
    GMW_HIP(ctx, hipMemsetAsync(map->qt_ctr.p, 0, kWallQuantityCounters * 8, map->stream));

    Carve stage{map->qt_stage.p};
    WallQuantityArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.has_base = baseline ? 1u : 0u;
    a.base = baseline ? baseline->table : map->table;
    a.n = n; a.nsec = nsec;
    a.first = (uint64_t)station0 * nsec;
    a.station0 = station0; a.S = S;
    a.min_count = qp.min_count; a.n_zones = n_zones;
    a.Rq = Rq;
    a.lo = d_lo; a.hi = d_hi;
    a.section_profile = section_profile ? d_profile : nullptr;
    a.zone = zone ? d_zone : nullptr;
    a.records = stage.take<gm_wall_quantity>((uint64_t)cs * n_zones);
    a.rows = profile_rows ? stage.take<int32_t>((uint64_t)cs * nsec) : nullptr;
    a.ctr = map->qt_ctr.p;

    // A count query and a call without room run the same launches: the totals of info are the device's.  Only the copies
    // of the two arrays depend on the buffers.
    const bool copying = records && capacity >= total;
    unsigned long long ctr[kWallQuantityCounters];
    for (uint32_t sec0 = 0; sec0 < NS; sec0 += cs) {   // (the trip count depends on the window alone)
        const uint32_t ns = std::min(cs, NS - sec0);
        a.sec0 = sec0;
        a.nsect = ns;
        launch_wall_quantities(a, map->stream);
        GMW_HIP(ctx, hipGetLastError());
        if (copying) {
            GMW_HIP(ctx, hipMemcpyAsync(records + (size_t)sec0 * n_zones, a.records, (size_t)ns * n_zones * sizeof(gm_wall_quantity),
                                        hipMemcpyDeviceToHost, map->stream));
            if (profile_rows)
                GMW_HIP(ctx, hipMemcpyAsync(profile_rows + (size_t)sec0 * nsec, a.rows, (size_t)ns * nsec * sizeof(int32_t),
                                            hipMemcpyDeviceToHost, map->stream));
        }
        if (NS - sec0 <= cs)   // the last chunk: the totals ride on its wait
            GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));   // (the next chunk rewrites the staging; the tables have left the caller's buffers)
    }
    info->unmeasured = ctr[GM_WALL_QUANTITY_CLASS_UNMEASURED];
    info->empty = ctr[GM_WALL_QUANTITY_CLASS_EMPTY];
    info->unusable = ctr[GM_WALL_QUANTITY_CLASS_UNUSABLE];
    info->under = ctr[GM_WALL_QUANTITY_CLASS_UNDER];
    info->over = ctr[GM_WALL_QUANTITY_CLASS_OVER];
    info->within = ctr[GM_WALL_QUANTITY_CLASS_WITHIN];
    info->sections_under = (uint32_t)ctr[6];
    info->sections_over = (uint32_t)ctr[7];
    if (records && capacity < total) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_quantities: record buffer too small");
    return GM_OK;
}

}  // extern "C"
