// gm_wall.hip -- C ABI of the persistent wall map (gm_wall_*; include/gm_hip.h states the rule).  Host logic only: the
// design frame and the per-add frame in fp64, the station window of a frame, ownership.  Kernels are in k_wall.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gm_compact.hpp"
#include "gm_internal.hpp"

using namespace gm;

#define GMW_HIP(ctx, call)                                                           \
    do {                                                                             \
        hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) {                                                     \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);         \
            return (e__ == hipErrorOutOfMemory) ? GM_ERR_OOM : GM_ERR_DEVICE;        \
        }                                                                            \
    } while (0)
#define GMW_OK(call)                       \
    do {                                   \
        const gm_status s__ = (call);      \
        if (s__ != GM_OK) return s__;      \
    } while (0)

// The records of a chained scan (gm_compact.hpp) that is not a frame's -- a slot's own belong to the frame that may be in
// flight on it: the record array with the ticket word behind it, and the epoch of the launches on it so far.  The rule is
// next_scan's (gm_internal.hpp): epochs run 1 .. 2^29-2 and never 0, and the records are cleared when the counter wraps,
// behind every launch that wrote them.
struct ScanRecords {
    DevArray<unsigned long long> rec;   // [n] tile records | the ticket word
    uint32_t n = 0;
    uint32_t epoch = 0;
    bool holds(uint32_t points) const { return n >= compact_records(points); }
    // for launches over up to `points` inputs; a new block is zeroed on s.  Nothing may be in flight on the old one.
    gm_status reserve(gm_ctx *ctx, uint32_t points, hipStream_t s)
    {
        if (holds(points)) return GM_OK;
        n = 0;
        const uint32_t want = compact_records(points);
        GMW_HIP(ctx, rec.reserve((uint64_t)want + 1));
        GMW_HIP(ctx, hipMemsetAsync(rec.p, 0, sizeof(unsigned long long) * ((size_t)want + 1), s));
        n = want;
        return GM_OK;
    }
    // the state of the next k_compact launch on s
    ScanState next(hipStream_t s)
    {
        if (epoch >= 0x1FFFFFFEu) {
            (void)hipMemsetAsync(rec.p, 0, sizeof(unsigned long long) * ((size_t)n + 1), s);
            epoch = 0;
        }
        epoch += 1u;
        ScanState st;
        st.status = rec.p;
        st.ticket = reinterpret_cast<uint32_t *>(rec.p + n);
        st.epoch = epoch;
        st.frame_ptr = nullptr;
        return st;
    }
};

// gm_wall_map_check_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallCheckSlot {
    DevArray<gm_wall_check_point> stage;    // the changed rows of the last check, in order
    ScanRecords scan;                       // the check's own chained scan
    DevArray<unsigned long long> ctr;       // device [kWallCheckCounters]
    HostArray<unsigned long long> h_ctr;    // pinned copy, valid once `done` has passed
    hipEvent_t done = nullptr;              // recorded behind the check and the copy of its counters
    hipEvent_t adds = nullptr;              // recorded on this slot's stream by a check on another slot: the adds so far
    bool have = false;                      // a check was enqueued: a result is (or will be) readable
    bool outstanding = false;               // the host has not waited for `done` yet
    uint32_t status = 0;
    long long T = 0;
    int64_t anchor = 0;                     // the check's j_f (gm_wall_map_check_objects anchors its window on it)
};

// gm_wall_map_locate_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallLocateSlot {
    DevArray<WallLocateWork> work;          // the state between the passes, the result behind them
    DevArray<double> partial;               // [kFitBlocks][kFitRowLen] partial rows of a pass
    DevArray<uint32_t> ticket;              // last-block ticket of the passes (0 between launches)
    HostArray<WallLocateWork> h_work;       // pinned copy, valid once `done` has passed
    hipEvent_t done = nullptr;              // recorded behind the passes and the copy of the result
    bool have = false;                      // a locate was enqueued: a result is (or will be) readable
    bool outstanding = false;               // the host has not waited for `done` yet
    int64_t anchor = 0;                     // the locate's j_f
    double of[3] = {0.0, 0.0, 0.0};         // its o_f, map coordinates
};

// gm_wall_map_align_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallAlignSlot {
    DevArray<uint8_t> zeroed;               // counters | score table | patch sums | patch counts: one zero-fill per align
    DevArray<int32_t> f, m;                 // the two value images
    HostArray<uint8_t> h_res;               // pinned copy of counters | score table, valid once `done` has passed
    hipEvent_t done = nullptr;              // recorded behind the align and the copy of its result
    bool have = false;                      // an align was enqueued: a result is (or will be) readable
    bool outstanding = false;               // the host has not waited for `done` yet
    gm_wall_align_params prm;               // of that align
    double pose[12];                        // the caller's pose of that align
    uint32_t n_shifts = 0;                  // (2A + 1)(2B + 1)
};

struct gm_wall_map {
    gm_ctx *ctx = nullptr;
    gm_wall_params prm;
    uint64_t ncell = 0;
    DevArray<uint8_t> base;        // the device table (zeroed at creation)
    WallTable table;
    double o[3], a[3], u[3], v[3], R;   // the design frame, fp64, not rounded
    uint32_t status = GM_SURF_OK;
    uint64_t frames = 0;
    hipStream_t stream = nullptr;  // the small kernels (read / merge / clear / count) and their copies
    std::vector<uint8_t> pending;  // per slot of ctx: an add was enqueued on its stream since the last sync
    DevArray<uint8_t> stage;       // device staging of the window calls, kStageCells records
    // the stage calls' per-point outputs: gm_wall_map_add_points' and, beside them, gm_wall_map_check_points'
    DevArray<float> pt_res;
    DevArray<int32_t> pt_cell, ck_delta;
    DevArray<uint8_t> ck_cls;
    uint32_t points_per_block = 0; // 0: the kernel's default (GM_WALL_POINTS_PER_BLOCK: measurements)
    // gm_wall_map_regions: the tile (GM_WALL_REGION_TILE: tests, measurements) and the scratch
    uint32_t region_ts = GM_WALL_REGION_TILE_STATIONS, region_tk = GM_WALL_REGION_TILE_SECTORS;
    DevArray<uint8_t> rg_cells;    // per window cell: d i64 | parent u32 | slot u32
    DevArray<unsigned long long> rg_ctr;   // [kWallRegionCounters]
    DevArray<uint8_t> rg_recs;     // per component: WallRegionAcc | gm_wall_region
    // gm_wall_map_cloud: the chunk (GM_WALL_CLOUD_CHUNK: tests, measurements; 0: kStageCells blocks) and the scratch
    uint32_t cloud_chunk = 0;
    DevArray<uint8_t> cl_acc;      // merged accumulators of a chunk, kWallCloudAccBytes per block (a merging call only)
    DevArray<gm_wall_cloud_point> cl_stage;   // a chunk's records
    ScanRecords cl_scan;           // the map's own chained scan
    DevArray<unsigned long long> cl_ctr;      // [kWallCloudCounters]
    DevArray<double> cl_dirs;      // [GM_WALL_MAX_SECTORS][2]
    std::vector<double> cl_dirs_host;          // the table of the call in progress
    // gm_wall_map_clearance: the chunk (GM_WALL_CLEAR_CHUNK: tests, measurements; 0: kStageCells cells) and the scratch
    uint32_t clear_chunk = 0;
    DevArray<int32_t> cr_gauge;    // the uploaded tables [n_gauges][n_sectors]
    DevArray<uint8_t> cr_station_gauge;        // [n]
    DevArray<gm_wall_clearance_station> cr_stations;   // [n]
    DevArray<gm_wall_clearance_cell> cr_stage; // a chunk's list rows
    ScanRecords cr_scan;           // the list's own chained scan
    DevArray<unsigned long long> cr_ctr;       // [kWallClearCounters]
    // gm_wall_map_check_*
    std::vector<WallCheckSlot> checks;         // per slot of ctx
    // gm_wall_map_locate_*
    std::vector<WallLocateSlot> locates;       // per slot of ctx
    // gm_wall_map_align_*: the patch rows per score block (GM_WALL_ALIGN_ROWS: tests, measurements; 0: the default rule)
    std::vector<WallAlignSlot> aligns;         // per slot of ctx
    uint32_t align_rows = 0;
    // gm_wall_map_check_objects / gm_wall_check_objects: the tile in blocks (GM_WALL_OBJECT_TILE: tests, measurements) and
    // the scratch
    uint32_t object_tr = GM_WALL_OBJECT_TILE_ROWS, object_tc = GM_WALL_OBJECT_TILE_COLS;
    DevArray<uint32_t> ob_blocks;            // per window block and plane: cnt | parent | slot
    DevArray<unsigned long long> ob_ctr;     // [kWallObjectCounters]
    DevArray<uint8_t> ob_recs;               // per component: WallObjectAcc | gm_wall_object | out_slot u32 | pos i32
    DevArray<gm_wall_check_point> ob_rows;   // the stage call's rows
    DevArray<int32_t> ob_of_row;             // object_of_row
    std::vector<gm_wall_object> ob_host;     // the unsorted list, its slots, the sorting permutation, slot -> position
    std::vector<uint32_t> ob_host_slot, ob_order;
    std::vector<int32_t> ob_pos;
};

namespace {

constexpr uint64_t kStageCells = 1u << 20;   // cells per chunk of a window call (24 MiB of raw records)

double dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

gm_status check_params(const gm_wall_params *p)
{
    if (!p || p->struct_size != sizeof(gm_wall_params)) return GM_ERR_INVALID_ARG;
    if (p->n_stations < 1u || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS ||
        (uint64_t)p->n_stations * p->n_sectors > GM_WALL_MAX_CELLS)
        return GM_ERR_INVALID_ARG;
    if (!(p->station_length > 0.0) || !isfinite(p->station_length) || !((float)p->station_length > 0.0f) ||
        !isfinite((float)p->station_length) || !isfinite(p->t_min) || !(p->gate > 0.0) || !(p->gate <= 8.0) ||
        !(p->radius > 0.0) || !isfinite((float)p->radius))
        return GM_ERR_INVALID_ARG;
    double up2 = 0.0, fw2 = 0.0, d2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(p->up[k]) || !isfinite(p->forward[k]) || !isfinite(p->direction[k]) || !isfinite(p->point[k]))
            return GM_ERR_INVALID_ARG;
        up2 += p->up[k] * p->up[k];
        fw2 += p->forward[k] * p->forward[k];
        d2 += p->direction[k] * p->direction[k];
    }
    if (!(up2 > 0.0) || !(fw2 > 0.0) || !(d2 > 0.0) || !isfinite(up2) || !isfinite(fw2) || !isfinite(d2)) return GM_ERR_INVALID_ARG;
    return GM_OK;
}

// the design frame of include/gm_hip.h: k_surface.hip's surf_frame on fp64 inputs, kept in fp64
struct DesignFrame { double o[3], a[3], u[3], v[3], R; uint32_t status; };
void design_frame_of(const gm_wall_params &p, DesignFrame &d)
{
    const double dn = sqrt(dot(p.direction, p.direction));
    const double s = dot(p.direction, p.forward);
    for (int k = 0; k < 3; ++k) d.a[k] = (s >= 0.0 ? p.direction[k] : -p.direction[k]) / dn;
    const double ca = dot(p.point, d.a), ua = dot(p.up, d.a);
    double u[3];
    for (int k = 0; k < 3; ++k) u[k] = p.up[k] - ua * d.a[k];
    const double ul = sqrt(dot(u, u)), upl = sqrt(dot(p.up, p.up));
    d.status = GM_SURF_OK;
    if (ul < 0.1 * upl) {
        double e2[3];
        fit_basis(d.a, u, e2);
        d.status |= GM_SURF_UP_FALLBACK;
    } else {
        for (int k = 0; k < 3; ++k) u[k] /= ul;
    }
    const double *a = d.a;
    const double v[3] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]};
    for (int k = 0; k < 3; ++k) {
        d.o[k] = p.point[k] - ca * a[k];
        d.u[k] = u[k];
        d.v[k] = v[k];
    }
    d.R = p.radius;
}
void design_frame(gm_wall_map *m)
{
    DesignFrame d;
    design_frame_of(m->prm, d);
    for (int k = 0; k < 3; ++k) { m->o[k] = d.o[k]; m->a[k] = d.a[k]; m->u[k] = d.u[k]; m->v[k] = d.v[k]; }
    m->R = d.R;
    m->status = d.status;
}

// the library's pose check: 0 the pose is accepted (Rm, tr filled), 1 an entry is not finite, 2 Rm is not a rotation
int pose_split(const double pose[12], double Rm[3][3], double tr[3])
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c)
            if (!isfinite(pose[4 * r + c])) return 1;
        for (int c = 0; c < 3; ++c) Rm[r][c] = pose[4 * r + c];
        tr[r] = pose[4 * r + 3];
    }
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = Rm[0][i] * Rm[0][j] + Rm[1][i] * Rm[1][j] + Rm[2][i] * Rm[2][j] - (i == j ? 1.0 : 0.0);
            dev = std::max(dev, fabs(g));
        }
    const double det = Rm[0][0] * (Rm[1][1] * Rm[2][2] - Rm[1][2] * Rm[2][1]) - Rm[0][1] * (Rm[1][0] * Rm[2][2] - Rm[1][2] * Rm[2][0]) +
                       Rm[0][2] * (Rm[1][0] * Rm[2][1] - Rm[1][1] * Rm[2][0]);
    return (!(dev <= 1e-6) || !(det > 0.0)) ? 2 : 0;
}

// The per-add frame: pose check, anchor, (o', a', u', v') in sensor coordinates, and the kernel's arguments but for the
// buffers.  The context's crop bound (a cube around the sensor) sizes the LDS window.
// f64 (a locate's start): the same vectors before the rounding, and o_f in map coordinates.
struct WallFrame64 { double c[3], d[3], u[3], v[3], of[3]; };
gm_status add_frame_args(gm_wall_map *m, const double pose[12], gm_wall_add_info *info, WallArgs &w, WallFrame64 *f64 = nullptr)
{
    gm_ctx *ctx = m->ctx;
    if (!pose) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: NULL pose");
    double Rm[3][3], tr[3];
    const int bad = pose_split(pose, Rm, tr);
    if (bad == 1) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose is not finite");
    if (bad) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose rotation is not orthonormal to 1e-6 or is a reflection");
    const gm_wall_params &p = m->prm;
    const double ds = p.station_length;
    const double rel[3] = {tr[0] - m->o[0], tr[1] - m->o[1], tr[2] - m->o[2]};
    const double s = dot(rel, m->a);
    const double jd = floor((s - p.t_min) / ds);
    if (!(fabs(jd) < 4.0e18)) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map: pose is too far along the axis");
    const int64_t jf = (int64_t)jd;
    const double off = p.t_min + jd * ds;
    double of[3];   // o_f - tr
    for (int k = 0; k < 3; ++k) of[k] = m->o[k] + off * m->a[k] - tr[k];
    memset(&w, 0, sizeof(w));
    double a1 = 0.0;   // |a'|_1: the reach of the crop cube along the axis
    for (int c = 0; c < 3; ++c) {   // Rm^T x
        const double oo = Rm[0][c] * of[0] + Rm[1][c] * of[1] + Rm[2][c] * of[2];
        const double aa = Rm[0][c] * m->a[0] + Rm[1][c] * m->a[1] + Rm[2][c] * m->a[2];
        const double uu = Rm[0][c] * m->u[0] + Rm[1][c] * m->u[1] + Rm[2][c] * m->u[2];
        const double vv = Rm[0][c] * m->v[0] + Rm[1][c] * m->v[1] + Rm[2][c] * m->v[2];
        w.o[c] = (float)oo; w.a[c] = (float)aa; w.u[c] = (float)uu; w.v[c] = (float)vv;
        if (f64) { f64->c[c] = oo; f64->d[c] = aa; f64->u[c] = uu; f64->v[c] = vv; f64->of[c] = m->o[c] + off * m->a[c]; }
        a1 += fabs(aa);
    }
    const double two_pi = 6.283185307179586476925286766559;
    w.R = (float)m->R;
    w.station_length = (float)ds;
    w.gate = (float)p.gate;
    w.sector_angle = (float)(two_pi / (double)p.n_sectors);
    w.two_pi = (float)two_pi;
    w.n_stations = p.n_stations;
    w.n_sectors = p.n_sectors;
    w.anchor = jf;
    w.table = m->table;
    // The LDS window: t = p.a' + (s - chainage of the anchor station's start) lies in [-B |a'|_1, B |a'|_1 + ds) for the
    // points of the crop cube |p|_inf <= B, so their stations relative to the anchor in [floor(-reach), floor(reach) + 1].
    // Whole stations, as many as the LDS table holds; a footprint beyond it is centred (the rest goes to the map directly).
    const uint32_t wmax = GM_SURF_MAX_CELLS / p.n_sectors;   // >= 1: n_sectors <= 4096
    const double reach = std::min(ctx->cfg.boxFilterBound * a1 / ds, 1.0e6);
    const int64_t first = (int64_t)floor(-reach) - 1, last = (int64_t)floor(reach) + 2;   // one station of fp32 slack each side
    const int64_t need = last - first + 1;
    if (need <= (int64_t)wmax) {
        w.win_first = (int32_t)first;
        w.win_stations = (uint32_t)need;
    } else {
        w.win_first = -(int32_t)(wmax / 2);
        w.win_stations = wmax;
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->struct_size = (uint32_t)sizeof(gm_wall_add_info);
        info->status = m->status;
        info->anchor_station = jf;
        for (int k = 0; k < 3; ++k) { info->o[k] = w.o[k]; info->a[k] = w.a[k]; info->u[k] = w.u[k]; info->v[k] = w.v[k]; }
        info->R = w.R;
        info->station_length = w.station_length;
        info->sector_angle = w.sector_angle;
        info->gate = w.gate;
    }
    return GM_OK;
}

gm_status sync_map(gm_wall_map *m)
{
    gm_ctx *ctx = m->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    for (uint32_t i = 0; i < ctx->n_slots; ++i)
        if (m->pending[i]) {
            GMW_HIP(ctx, hipStreamSynchronize(ctx->slots[i].stream));
            m->pending[i] = 0;
        }
    for (WallCheckSlot &c : m->checks)
        if (c.outstanding) {
            GMW_HIP(ctx, hipEventSynchronize(c.done));
            c.outstanding = false;
        }
    for (WallLocateSlot &l : m->locates)
        if (l.outstanding) {
            GMW_HIP(ctx, hipEventSynchronize(l.done));
            l.outstanding = false;
        }
    for (WallAlignSlot &l : m->aligns)
        if (l.outstanding) {
            GMW_HIP(ctx, hipEventSynchronize(l.done));
            l.outstanding = false;
        }
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

void free_map(gm_wall_map *m)
{
    hipSetDevice(m->ctx->device);
    for (uint32_t i = 0; i < m->ctx->n_slots; ++i)
        if (m->pending[i] && m->ctx->slots[i].stream) hipStreamSynchronize(m->ctx->slots[i].stream);
    for (WallCheckSlot &c : m->checks) {
        if (c.outstanding) hipEventSynchronize(c.done);
        if (c.done) hipEventDestroy(c.done);
        if (c.adds) hipEventDestroy(c.adds);
    }
    for (WallLocateSlot &l : m->locates) {
        if (l.outstanding) hipEventSynchronize(l.done);
        if (l.done) hipEventDestroy(l.done);
    }
    for (WallAlignSlot &l : m->aligns) {
        if (l.outstanding) hipEventSynchronize(l.done);
        if (l.done) hipEventDestroy(l.done);
    }
    if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
    delete m;   // (every DevArray and HostArray goes with it)
}

// A stage call's points (gm_wall_map_add_points, gm_wall_map_check_points) on the staging slot: open, whatever the call
// enqueues ahead of its points, upload, the call's launch, close.
struct StageCall {
    gm_wall_map *map;
    uint32_t n;
    float *residual;   // the caller's per-point outputs (NULL: not wanted)
    int32_t *cell, *delta;
    uint8_t *cls;
    Slot *sl = nullptr;
    // the slot, its capacity and the device side of the per-point outputs; nothing is enqueued
    gm_status open()
    {
        gm_ctx *ctx = map->ctx;
        GMW_OK(gm_begin_stage(ctx, sl));
        GMW_OK(gm_ensure_capacity(ctx, *sl, n ? n : 1u, (size_t)(n ? n : 1u) * 16, true));
        if (residual || cell) {
            GMW_HIP(ctx, map->pt_res.reserve(n));
            GMW_HIP(ctx, map->pt_cell.reserve(n));
        }
        if (delta || cls) {
            GMW_HIP(ctx, map->ck_delta.reserve(n));
            GMW_HIP(ctx, map->ck_cls.reserve(n));
        }
        return GM_OK;
    }
    // points and labels onto the slot's stream; w: the point fields of the launch
    gm_status upload(const float *xyz, const uint8_t *labels, WallArgs &w)
    {
        gm_ctx *ctx = map->ctx;
        GMW_OK(gm_upload_xyz(ctx, *sl, xyz, n, sl->crop4));
        if (labels && n) GMW_HIP(ctx, hipMemcpyAsync(sl->labels, labels, n, hipMemcpyHostToDevice, sl->stream));
        w.pts = sl->crop4;
        w.labels = labels ? sl->labels : nullptr;
        w.n_ptr = nullptr;
        w.n_host = n;
        w.res = residual ? map->pt_res.p : nullptr;
        w.cell = cell ? map->pt_cell.p : nullptr;
        return GM_OK;
    }
    // the per-point outputs back, behind the launch; blocks until the slot's stream has drained
    gm_status close()
    {
        gm_ctx *ctx = map->ctx;
        if (residual && n) GMW_HIP(ctx, hipMemcpyAsync(residual, map->pt_res.p, (size_t)n * 4, hipMemcpyDeviceToHost, sl->stream));
        if (cell && n) GMW_HIP(ctx, hipMemcpyAsync(cell, map->pt_cell.p, (size_t)n * 4, hipMemcpyDeviceToHost, sl->stream));
        if (delta && n) GMW_HIP(ctx, hipMemcpyAsync(delta, map->ck_delta.p, (size_t)n * 4, hipMemcpyDeviceToHost, sl->stream));
        if (cls && n) GMW_HIP(ctx, hipMemcpyAsync(cls, map->ck_cls.p, (size_t)n, hipMemcpyDeviceToHost, sl->stream));
        GMW_HIP(ctx, hipStreamSynchronize(sl->stream));
        return GM_OK;
    }
};

// the caller's parameters, or the defaults for NULL
template <class P>
P params_or(const P *prm, void (*defaults)(P *))
{
    P p;
    defaults(&p);
    if (prm) p = *prm;
    return p;
}

// The extent outputs the two metrics calls share: chainage_from / _to and angle_from_deg / _to_deg of a record's station
// and sector extents, the turned pair when it is the shorter (the record lies across the seam).  false, and nothing
// written: the extents are not those of a record on this grid.  One operation per statement: the same roundings as the
// twin's, whatever the compiler may contract.
template <class R, class M>
bool extent_metrics(const gm_wall_params &p, const R &r, M *out)
{
    const uint32_t ns = p.n_sectors, half = ns / 2u;
    if (r.sector_min > r.sector_max || r.sector_max >= ns || r.sector_min_turned > r.sector_max_turned ||
        r.sector_max_turned >= ns || r.station_min > r.station_max)
        return false;
    const double from = (double)r.station_min * p.station_length;
    const double to = (double)(r.station_max + 1.0) * p.station_length;
    out->chainage_from = p.t_min + from;
    out->chainage_to = p.t_min + to;
    const uint32_t plain = r.sector_max - r.sector_min + 1u, turned = r.sector_max_turned - r.sector_min_turned + 1u;
    uint32_t k_from = r.sector_min, k_end = r.sector_max + 1u;
    if (turned < plain) {   // turned back: k = (t - n_sectors / 2) mod n_sectors
        k_from = (r.sector_min_turned + ns - half) % ns;
        k_end = (r.sector_max_turned + ns - half) % ns + 1u;
    }
    const double a0 = 360.0 * (double)k_from;
    const double a1 = 360.0 * (double)k_end;
    out->angle_from_deg = a0 / (double)ns;
    out->angle_to_deg = a1 / (double)ns;
    return true;
}

// one window call in chunks of the staging buffer: raw true -> gm_wall_raw_cell, else gm_surface_cell
gm_status read_window(gm_wall_map *m, uint32_t station0, uint32_t n, void *cells, bool raw)
{
    gm_ctx *ctx = m->ctx;
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

// the direction table of include/gm_hip.h: NK pairs (one operation per statement, as stated there)
void cloud_directions(uint32_t nsec, uint32_t bk, double *cos_sin)
{
    const double two_pi = 6.283185307179586476925286766559;
    const uint32_t NK = (nsec + bk - 1u) / bk;
    for (uint32_t K = 0; K < NK; ++K) {
        const uint32_t nk = nsec - K * bk < bk ? nsec - K * bk : bk;
        const double f = (double)(2u * K * bk + nk) / (double)(2u * nsec);
        const double phi = two_pi * f;
        cos_sin[2 * K] = cos(phi);
        cos_sin[2 * K + 1] = sin(phi);
    }
}

// ---- gm_wall_map_clearance ----

// gm_wall_clearance_check_params' rule; T and R_q of an accepted call
bool clearance_ok(const gm_wall_params *p, const gm_wall_clearance_params &c, const int32_t *gauge_q, uint32_t n_gauges,
                  const uint8_t *station_gauge, uint32_t n, long long &T, long long &Rq)
{
    T = 0; Rq = 0;
    if (!p || !gauge_q || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return false;
    if (c.struct_size != sizeof(gm_wall_clearance_params) || c.reference > (uint32_t)GM_WALL_CLEAR_MEAN || c.min_count < 1u) return false;
    if (!(c.margin >= 0.0) || !(c.margin <= 8.0)) return false;
    if (!(p->radius > 0.0) || !isfinite(p->radius)) return false;
    const double rq = rint(p->radius * 1048576.0);
    if (!(rq <= 4294967296.0)) return false;
    if (n_gauges < 1u || n_gauges > GM_WALL_CLEAR_MAX_GAUGES) return false;
    const size_t entries = (size_t)n_gauges * p->n_sectors;
    for (size_t i = 0; i < entries; ++i)
        if (gauge_q[i] < 0) return false;
    if (station_gauge)
        for (uint32_t j = 0; j < n; ++j)
            if (station_gauge[j] >= n_gauges) return false;
    T = (long long)rint(c.margin * 1048576.0);
    Rq = (long long)rq;
    return true;
}

double cross2(const double a[2], const double b[2]) { return a[0] * b[1] - a[1] * b[0]; }

// 1 when the closed segments ab and cd share a point
bool segments_meet(const double a[2], const double b[2], const double c[2], const double d[2])
{
    const double ab[2] = {b[0] - a[0], b[1] - a[1]}, cd[2] = {d[0] - c[0], d[1] - c[1]};
    const double ac[2] = {c[0] - a[0], c[1] - a[1]}, ad[2] = {d[0] - a[0], d[1] - a[1]};
    const double ca[2] = {a[0] - c[0], a[1] - c[1]}, cb[2] = {b[0] - c[0], b[1] - c[1]};
    const double o1 = cross2(ab, ac), o2 = cross2(ab, ad), o3 = cross2(cd, ca), o4 = cross2(cd, cb);
    if (((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0))) return true;
    auto on = [](const double p[2], const double q[2], const double r[2]) {   // r collinear with pq: inside its box?
        return std::min(p[0], q[0]) <= r[0] && r[0] <= std::max(p[0], q[0]) && std::min(p[1], q[1]) <= r[1] && r[1] <= std::max(p[1], q[1]);
    };
    return (o1 == 0.0 && on(a, b, c)) || (o2 == 0.0 && on(a, b, d)) || (o3 == 0.0 && on(c, d, a)) || (o4 == 0.0 && on(c, d, b));
}

// the polygon of gm_wall_gauge_from_polygon is accepted: finite, no edge of length 0, simple, the axis strictly inside
bool gauge_polygon_ok(const std::vector<double> &P, uint32_t nv)
{
    for (uint32_t i = 0; i < 2u * nv; ++i)
        if (!isfinite(P[i])) return false;
    const double zero[2] = {0.0, 0.0};
    int wn = 0;
    for (uint32_t i = 0; i < nv; ++i) {
        const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
        if (a[0] == b[0] && a[1] == b[1]) return false;
        const double left = cross2(a, b);   // > 0: the axis lies to the left of a -> b
        if (left == 0.0 && segments_meet(a, b, zero, zero)) return false;   // the axis on the boundary
        if (a[1] <= 0.0) {
            if (b[1] > 0.0 && left > 0.0) ++wn;
        } else if (b[1] <= 0.0 && left < 0.0) {
            --wn;
        }
    }
    if (wn == 0) return false;
    for (uint32_t i = 0; i < nv; ++i) {
        const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
        for (uint32_t j = i + 1u; j < nv; ++j) {
            const double *c = &P[2 * j], *d = &P[2 * ((j + 1u) % nv)];
            const bool next = j == i + 1u, prev = i == 0u && j == nv - 1u;
            if (next || prev) {   // neighbours share one vertex; they may not fold back onto each other
                const double *s = next ? b : a, *x = next ? a : b, *y = next ? d : c;   // s shared; x, y the far ends
                const double e[2] = {x[0] - s[0], x[1] - s[1]}, f[2] = {y[0] - s[0], y[1] - s[1]};
                if (cross2(e, f) == 0.0 && e[0] * f[0] + e[1] * f[1] > 0.0) return false;
            } else if (segments_meet(a, b, c, d)) {
                return false;
            }
        }
    }
    return true;
}

// ---- gm_wall_map_check_* ----

bool check_prm_ok(const gm_wall_check_params &c, long long &T)
{
    T = 0;
    if (c.struct_size != sizeof(gm_wall_check_params) || c.reference > (uint32_t)GM_WALL_CHECK_ENVELOPE || c.min_count < 1u) return false;
    if (!(c.threshold > 0.0) || !(c.threshold <= 8.0) || !(c.gate > 0.0) || !(c.gate <= 8.0)) return false;
    T = (long long)rint(c.threshold * 1048576.0);
    return T >= 1;
}

// The scratch of (map, slot) for a check of up to n_cap points, and everything a launch on `s` needs before it: zeroed
// counters, a fresh scan state.
gm_status check_prepare(gm_wall_map *m, uint32_t slot, uint32_t n_cap, hipStream_t s, ScanState &st)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    if (!c.done) GMW_HIP(ctx, hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
    GMW_HIP(ctx, c.ctr.reserve(kWallCheckCounters));
    GMW_HIP(ctx, c.h_ctr.reserve(kWallCheckCounters));
    if (c.stage.cap < n_cap || !c.scan.holds(n_cap)) {
        if (c.outstanding) {   // the slot's last check may still be writing the old blocks
            GMW_HIP(ctx, hipEventSynchronize(c.done));
            c.outstanding = false;
        }
        c.have = false;        // (its rows go with the block)
    }
    GMW_HIP(ctx, c.stage.reserve(n_cap));
    GMW_OK(c.scan.reserve(ctx, n_cap, s));
    st = c.scan.next(s);
    GMW_HIP(ctx, hipMemsetAsync(c.ctr.p, 0, kWallCheckCounters * 8, s));
    return GM_OK;
}

// `s` (the stream of `slot`) waits for the adds enqueued so far on every other slot's stream: an event, no host block
gm_status check_wait_adds(gm_wall_map *m, uint32_t slot, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    for (uint32_t i = 0; i < ctx->n_slots; ++i) {
        if (i == slot || !m->pending[i]) continue;
        WallCheckSlot &o = m->checks[i];
        if (!o.adds) GMW_HIP(ctx, hipEventCreateWithFlags(&o.adds, hipEventDisableTiming));
        GMW_HIP(ctx, hipEventRecord(o.adds, ctx->slots[i].stream));
        GMW_HIP(ctx, hipStreamWaitEvent(s, o.adds, 0));
    }
    return GM_OK;
}

// the launch, the copy of its counters and the event behind both
gm_status check_enqueue(gm_wall_map *m, uint32_t slot, const WallCheckArgs &a, uint32_t n_cap, const ScanState &st, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    launch_wall_check(a, n_cap, st, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(c.h_ctr, c.ctr.p, kWallCheckCounters * 8, hipMemcpyDeviceToHost, s));
    GMW_HIP(ctx, hipEventRecord(c.done, s));
    c.have = true;
    c.outstanding = true;
    c.status = m->status;
    c.T = a.T;
    c.anchor = a.w.anchor;
    return GM_OK;
}

// the result of (map, slot) once `done` has passed
gm_status check_result(gm_wall_map *m, uint32_t slot, gm_wall_check_info *info, gm_wall_check_point *points, uint32_t capacity,
                       uint32_t *n_out)
{
    gm_ctx *ctx = m->ctx;
    WallCheckSlot &c = m->checks[slot];
    if (c.outstanding) {
        GMW_HIP(ctx, hipEventSynchronize(c.done));
        c.outstanding = false;
    }
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

bool locate_prm_ok(const gm_wall_locate_params &p)
{
    return p.struct_size == sizeof(gm_wall_locate_params) && p.reference <= (uint32_t)GM_WALL_LOCATE_MAP && p.min_count >= 1u &&
           p.gate > 0.0 && p.gate <= 8.0;
}

// the start of include/gm_hip.h: the add's frame before the rounding, and s0
gm_status locate_args(gm_wall_map *m, uint32_t slot, const double pose[12], const gm_wall_locate_params &lp, WallLocateArgs &a)
{
    WallFrame64 f;
    memset(&a, 0, sizeof(a));
    GMW_OK(add_frame_args(m, pose, nullptr, a.w, &f));
    a.reference = lp.reference;
    a.min_count = lp.min_count;
    a.gate = lp.gate;
    for (int k = 0; k < 3; ++k) { a.c0[k] = f.c[k]; a.d0[k] = f.d[k]; a.u0[k] = f.u[k]; a.v0[k] = f.v[k]; }
    a.s0 = -dot(f.c, f.d);
    WallLocateSlot &l = m->locates[slot];
    l.anchor = a.w.anchor;
    for (int k = 0; k < 3; ++k) l.of[k] = f.of[k];
    return GM_OK;
}

// the scratch of (map, slot); a new ticket is zeroed on `s`
gm_status locate_prepare(gm_wall_map *m, uint32_t slot, hipStream_t s, WallLocateArgs &a)
{
    gm_ctx *ctx = m->ctx;
    WallLocateSlot &l = m->locates[slot];
    if (!l.done) GMW_HIP(ctx, hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
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
gm_status locate_enqueue(gm_wall_map *m, uint32_t slot, const WallLocateArgs &a, hipStream_t s)
{
    gm_ctx *ctx = m->ctx;
    WallLocateSlot &l = m->locates[slot];
    launch_wall_locate(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_work.p, l.work.p, sizeof(WallLocateWork), hipMemcpyDeviceToHost, s));
    GMW_HIP(ctx, hipEventRecord(l.done, s));
    l.have = true;
    l.outstanding = true;
    return GM_OK;
}

// the result of (map, slot) once `done` has passed: the device's record, and the pose composed in fp64
gm_status locate_result(gm_wall_map *m, uint32_t slot, gm_wall_locate_info *info)
{
    gm_ctx *ctx = m->ctx;
    WallLocateSlot &l = m->locates[slot];
    if (l.outstanding) {
        GMW_HIP(ctx, hipEventSynchronize(l.done));
        l.outstanding = false;
    }
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
    for (int r = 0; r < 3; ++r) {   // Rm' = a d^T + u u'^T + v v'^T, tr' = o_f - Rm' c
        double rc = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double e = m->a[r] * wk.d[c] + m->u[r] * wk.u[c] + m->v[r] * wk.v[c];
            info->pose[4 * r + c] = e;
            rc += e * wk.c[c];
        }
        info->pose[4 * r + 3] = l.of[r] - rc;
    }
    return GM_OK;
}

// an add on `s` must not be seen by the locates enqueued before it on other slots
gm_status add_wait_locates(gm_wall_map *m, uint32_t slot, hipStream_t s)
{
    for (uint32_t i = 0; i < m->ctx->n_slots; ++i)
        if (i != slot && m->locates[i].outstanding) GMW_HIP(m->ctx, hipStreamWaitEvent(s, m->locates[i].done, 0));
    return GM_OK;
}

// ---- gm_wall_map_align_* ----

bool align_prm_ok(const gm_wall_align_params &p, uint32_t nsec)
{
    if (p.struct_size != sizeof(gm_wall_align_params) || nsec < 1u || nsec > GM_WALL_MAX_SECTORS) return false;
    if (p.half_patch_stations < 1u || 2ull * p.half_patch_stations * nsec > GM_WALL_ALIGN_MAX_PATCH_CELLS) return false;
    if (p.max_station_shift > GM_WALL_ALIGN_MAX_SHIFT || p.max_sector_shift > GM_WALL_ALIGN_MAX_SHIFT) return false;
    if (2u * p.max_sector_shift + 1u > nsec) return false;
    if ((2u * p.max_station_shift + 1u) * (2u * p.max_sector_shift + 1u) > GM_WALL_ALIGN_MAX_SHIFTS) return false;
    if (p.min_count < 1u || p.min_frame_count < 1u || p.min_overlap < 1u) return false;
    if (!(p.gate > 0.0) || !(p.gate <= 8.0) || !(p.clip > 0.0) || !(p.clip <= 8.0) || !(rint(p.clip * 1048576.0) >= 1.0)) return false;
    return p.min_distinction >= 1.0 && isfinite(p.min_distinction);
}

// The selection and the pose of include/gm_hip.h from a table of (2A + 1)(2B + 1) records.  Host only; fills everything
// but the device's counts.
void align_select(const DesignFrame &d, const gm_wall_params &wp, const gm_wall_align_params &ap, const double Rm[3][3],
                  const double tr[3], const gm_wall_align_score *t, gm_wall_align_info *info)
{
    const int A = (int)ap.max_station_shift, B = (int)ap.max_sector_shift, nb = 2 * B + 1, ns = (2 * A + 1) * nb;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const double ds = wp.station_length;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_align_info);
    const double rel[3] = {tr[0] - d.o[0], tr[1] - d.o[1], tr[2] - d.o[2]};
    const double jd = floor((dot(rel, d.a) - wp.t_min) / ds);
    info->anchor_station = fabs(jd) < 4.0e18 ? (int64_t)jd : 0;
    info->half_patch_stations = ap.half_patch_stations;
    info->max_station_shift = ap.max_station_shift;
    info->max_sector_shift = ap.max_sector_shift;
    auto cheb = [&](int i, int a0, int b0) { return std::max(abs(i / nb - A - a0), abs(i % nb - B - b0)); };
    auto valid = [&](int i) { return t[i].n >= ap.min_overlap; };
    auto cost = [&](int i) { return (double)t[i].ssd / (double)t[i].n; };
    int best = -1;
    for (int i = 0; i < ns; ++i) {
        if (!valid(i)) continue;
        if (best >= 0) {   // ssd_i / n_i against ssd_best / n_best, exactly
            const unsigned __int128 l = (unsigned __int128)t[i].ssd * t[best].n, r = (unsigned __int128)t[best].ssd * t[i].n;
            if (l > r || (l == r && cheb(i, 0, 0) >= cheb(best, 0, 0))) continue;
        }
        best = i;
    }
    if (best < 0) {
        info->status = GM_ALIGN_NO_OVERLAP;
        info->frac_station = info->frac_sector = info->shift_m = info->roll = info->bias_m = nan;
        info->rms_best = info->rms_runner = info->distinction = nan;
        for (int k = 0; k < 12; ++k) info->pose[k] = nan;
        return;
    }
    const int ia = best / nb, ib = best % nb, sa = ia - A, sb = ib - B;
    const double c0 = cost(best);
    auto fraction = [&](int lo, int hi, bool have) {
        if (!have || !valid(lo) || !valid(hi)) return 0.0;
        const double cm = cost(lo), cp = cost(hi), den = cm - 2.0 * c0 + cp;
        if (!(den > 0.0)) return 0.0;
        const double f = 0.5 * (cm - cp) / den;
        return f < -0.5 ? -0.5 : (f > 0.5 ? 0.5 : f);
    };
    const double fa = fraction(best - nb, best + nb, ia > 0 && ia < 2 * A);
    const double fb = fraction(best - 1, best + 1, ib > 0 && ib < 2 * B);
    double cr = inf;
    bool runner = false;
    for (int i = 0; i < ns; ++i)
        if (valid(i) && cheb(i, sa, sb) > 1) {
            const double c = cost(i);
            if (!runner || c < cr) cr = c;
            runner = true;
        }
    const double two_pi = 6.283185307179586476925286766559;
    info->overlap = t[best].n;
    info->best_station = sa;
    info->best_sector = sb;
    info->frac_station = fa;
    info->frac_sector = fb;
    info->shift_m = ((double)sa + fa) * ds;
    info->roll = ((double)sb + fb) * (two_pi / (double)wp.n_sectors);
    info->bias_m = ((double)t[best].sum_d * 0x1p-20) / (double)t[best].n;
    info->rms_best = sqrt(c0) * 0x1p-20;
    info->rms_runner = runner ? sqrt(cr) * 0x1p-20 : nan;
    info->distinction = (c0 == 0.0 || !runner) ? inf : cr / c0;
    info->status = GM_ALIGN_OK;
    if (info->distinction < ap.min_distinction) info->status |= GM_ALIGN_AMBIGUOUS;
    if ((A > 0 && abs(sa) == A) || (B > 0 && abs(sb) == B)) info->status |= GM_ALIGN_AT_BORDER;
    // Rm' = Q Rm, tr' = o + Q (tr - o) + shift_m a;  Q = cos I + sin [a]x + (1 - cos) a a^T
    const double cs = cos(info->roll), sn = sin(info->roll);
    const double *a = d.a;
    const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
    double Q[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Q[r][c] = (r == c ? cs : 0.0) + sn * K[r][c] + (1.0 - cs) * a[r] * a[c];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) info->pose[4 * r + c] = Q[r][0] * Rm[0][c] + Q[r][1] * Rm[1][c] + Q[r][2] * Rm[2][c];
        info->pose[4 * r + 3] = d.o[r] + (Q[r][0] * rel[0] + Q[r][1] * rel[1] + Q[r][2] * rel[2]) + info->shift_m * a[r];
    }
}

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
    if (!l.done) GMW_HIP(ctx, hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
    const uint64_t nsh = (uint64_t)(2u * a.A + 1u) * (2u * a.B + 1u);
    const uint64_t pc = 2ull * a.P * m->prm.n_sectors, mc = (2ull * a.P + 2ull * a.A) * m->prm.n_sectors;
    const uint64_t res_bytes = 8ull * kWallAlignCounters + nsh * sizeof(gm_wall_align_score), zero_bytes = res_bytes + pc * 12;
    if (l.outstanding && (l.zeroed.cap < zero_bytes || l.f.cap < pc || l.m.cap < mc || l.h_res.cap < res_bytes)) {
        GMW_HIP(ctx, hipEventSynchronize(l.done));   // the slot's last align may still be using the old blocks
        l.outstanding = false;
    }
    if (l.h_res.cap < res_bytes) l.have = false;     // (its result goes with the block)
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
    GMW_OK(check_wait_adds(m, slot, s));
    launch_wall_align_values(a, s);
    launch_wall_align_score(a, s);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(l.h_res.p, l.zeroed.p, 8 * kWallAlignCounters + (size_t)nsh * sizeof(gm_wall_align_score),
                                hipMemcpyDeviceToHost, s));
    GMW_HIP(ctx, hipEventRecord(l.done, s));
    l.have = true;
    l.outstanding = true;
    l.prm = ap;
    memcpy(l.pose, pose, sizeof(l.pose));
    l.n_shifts = nsh;
    return GM_OK;
}

// the result of (map, slot) once `done` has passed: the device's table and counts, the selection and the pose in fp64
gm_status align_result(gm_wall_map *m, uint32_t slot, gm_wall_align_info *info, gm_wall_align_score *scores, uint32_t capacity,
                       uint32_t *n_out)
{
    gm_ctx *ctx = m->ctx;
    WallAlignSlot &l = m->aligns[slot];
    if (l.outstanding) {
        GMW_HIP(ctx, hipEventSynchronize(l.done));
        l.outstanding = false;
    }
    const unsigned long long *h = reinterpret_cast<const unsigned long long *>(l.h_res.p);
    const gm_wall_align_score *table = reinterpret_cast<const gm_wall_align_score *>(l.h_res.p + 8 * kWallAlignCounters);
    if (n_out) *n_out = l.n_shifts;
    if (info) {
        double Rm[3][3], tr[3];
        (void)pose_split(l.pose, Rm, tr);   // (accepted at the enqueue)
        DesignFrame d;
        for (int k = 0; k < 3; ++k) { d.o[k] = m->o[k]; d.a[k] = m->a[k]; d.u[k] = m->u[k]; d.v[k] = m->v[k]; }
        d.R = m->R;
        d.status = m->status;
        align_select(d, m->prm, l.prm, Rm, tr, table, info);
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

// an add on `s` must not be seen by the aligns enqueued before it on other slots
gm_status add_wait_aligns(gm_wall_map *m, uint32_t slot, hipStream_t s)
{
    for (uint32_t i = 0; i < m->ctx->n_slots; ++i)
        if (i != slot && m->aligns[i].outstanding) GMW_HIP(m->ctx, hipStreamWaitEvent(s, m->aligns[i].done, 0));
    return GM_OK;
}

// ---- gm_wall_map_check_objects / gm_wall_check_objects ----

bool object_prm_ok(const gm_wall_object_params &p)
{
    return p.struct_size == sizeof(gm_wall_object_params) && p.block_stations >= 1u && p.block_sectors >= 1u &&
           p.min_block_points >= 1u && p.min_points >= 1u && (p.connectivity == 4u || p.connectivity == 8u) &&
           p.half_window_stations >= 1u && p.half_window_stations <= (1u << 20);
}

struct ObjectWindow {
    uint32_t J0 = 0, nJ = 0, NK = 0;         // block rows [J0, J0 + nJ) (nJ 0: empty), blocks per block row
    uint32_t station0 = 0, n_stations = 0;   // the block rows' stations, clipped to the map
};
// the window of include/gm_hip.h around the anchor j_f; false: more than GM_WALL_OBJECT_MAX_BLOCKS blocks
bool object_window(const gm_wall_params &p, const gm_wall_object_params &op, int64_t jf, ObjectWindow &w)
{
    const int64_t H = op.half_window_stations, ns = p.n_stations;   // (compared before added: j_f is any int64)
    const int64_t lo = jf > H ? jf - H : 0, hi = jf >= ns - H ? ns : jf + H;
    w = ObjectWindow();
    w.NK = (p.n_sectors + op.block_sectors - 1u) / op.block_sectors;
    if (lo >= hi) return true;
    const uint64_t bs = op.block_stations, J0 = (uint64_t)lo / bs, J1 = (uint64_t)(hi - 1) / bs;
    w.J0 = (uint32_t)J0;
    w.nJ = (uint32_t)(J1 - J0 + 1u);
    w.station0 = (uint32_t)(J0 * bs);
    w.n_stations = (uint32_t)(std::min<uint64_t>((J1 + 1u) * bs, (uint64_t)ns) - J0 * bs);
    return (uint64_t)w.nJ * w.NK <= GM_WALL_OBJECT_MAX_BLOCKS;
}

// The call on n_rows device rows (32-byte aligned), on the map's stream, blocking.  rejected_if_empty: the rejected rows,
// used when nothing is launched (zero rows or an empty window).  objects / object_of_row may be NULL; the capacities were
// checked by the caller but for the record count.
gm_status objects_run(gm_wall_map *m, const gm_wall_check_point *d_rows, uint32_t n_rows, uint32_t rejected_if_empty,
                      const gm_wall_object_params &op, const ObjectWindow &win, gm_wall_objects_info *info, gm_wall_object *objects,
                      uint32_t capacity, uint32_t *n_out, int32_t *object_of_row, const char *who)
{
    gm_ctx *ctx = m->ctx;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_objects_info);
    info->n_rows = n_rows;
    info->station0 = win.station0;
    info->n_stations = win.n_stations;
    info->blocks_stations = win.nJ;
    info->blocks_sectors = win.NK;
    if (!n_rows || !win.nJ) {   // nothing to launch
        info->rejected = rejected_if_empty;
        info->outside_window = n_rows - rejected_if_empty;
        if (object_of_row) std::fill(object_of_row, object_of_row + n_rows, -1);
        return GM_OK;
    }
    const uint64_t NB = (uint64_t)win.nJ * win.NK, pairs = 2u * NB;
    GMW_HIP(ctx, m->ob_blocks.reserve(3u * pairs));
    GMW_HIP(ctx, m->ob_ctr.reserve(kWallObjectCounters));
    if (object_of_row) GMW_HIP(ctx, m->ob_of_row.reserve(n_rows));
    WallObjectArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.nsec = m->prm.n_sectors;
    a.cells = (uint32_t)m->ncell;   // <= GM_WALL_MAX_CELLS
    a.bs = op.block_stations; a.bk = op.block_sectors; a.NK = win.NK;
    a.J0 = win.J0; a.nJ = win.nJ; a.NB = (uint32_t)NB;
    a.ts = m->object_tr; a.tk = m->object_tc;
    a.tiles_s = (a.nJ + a.ts - 1u) / a.ts;
    a.tiles_k = (a.NK + a.tk - 1u) / a.tk;
    a.conn8 = op.connectivity == 8u ? 1u : 0u;
    a.min_block_points = op.min_block_points;
    a.min_points = op.min_points;
    a.cnt = m->ob_blocks.p;   // cnt | parent | slot, [pairs] each
    a.parent = a.cnt + pairs;
    a.slot = a.parent + pairs;
    a.ctr = m->ob_ctr.p;
    a.object_of_row = m->ob_of_row.p;
    unsigned long long ctr[kWallObjectCounters];
    GMW_HIP(ctx, hipMemsetAsync(a.cnt, 0, pairs * 4, m->stream));
    GMW_HIP(ctx, hipMemsetAsync(a.ctr, 0, kWallObjectCounters * 8, m->stream));
    launch_wall_object_label(a, m->stream);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
    GMW_HIP(ctx, hipStreamSynchronize(m->stream));   // the one count the host needs: it sizes the records
    const uint64_t ncomp = ctr[7];
    if (ncomp) {
        GMW_HIP(ctx, m->ob_recs.reserve(ncomp * (sizeof(WallObjectAcc) + sizeof(gm_wall_object) + 4 + 4)));
        Carve recs{m->ob_recs.p};
        a.acc = recs.take<WallObjectAcc>(ncomp);
        a.out = recs.take<gm_wall_object>(ncomp);
        a.out_slot = recs.take<uint32_t>(ncomp);
        a.pos = recs.take<int32_t>(ncomp);
        a.ncomp = (uint32_t)ncomp;
        GMW_HIP(ctx, hipMemsetAsync(a.acc, 0, ncomp * sizeof(WallObjectAcc), m->stream));
        launch_wall_object_reduce(a, m->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
        GMW_HIP(ctx, hipStreamSynchronize(m->stream));
    }
    const uint32_t nobj = (uint32_t)ctr[8];
    info->rejected = (uint32_t)ctr[0]; info->outside_window = (uint32_t)ctr[1]; info->sparse = (uint32_t)ctr[2];
    info->small = (uint32_t)ctr[3]; info->in_object = (uint32_t)ctr[4];
    info->flagged_neg = (uint32_t)ctr[5]; info->flagged_pos = (uint32_t)ctr[6];
    info->components = (uint32_t)ncomp;
    info->objects = nobj;
    if (n_out) *n_out = nobj;
    const bool fits = nobj <= capacity;
    if (nobj && ((objects && fits) || object_of_row)) {   // the list in (label, sign) order
        m->ob_host.resize(nobj);
        m->ob_host_slot.resize(nobj);
        m->ob_order.resize(nobj);
        GMW_HIP(ctx, hipMemcpyAsync(m->ob_host.data(), a.out, (size_t)nobj * sizeof(gm_wall_object), hipMemcpyDeviceToHost, m->stream));
        GMW_HIP(ctx, hipMemcpyAsync(m->ob_host_slot.data(), a.out_slot, (size_t)nobj * 4, hipMemcpyDeviceToHost, m->stream));
        GMW_HIP(ctx, hipStreamSynchronize(m->stream));
        for (uint32_t i = 0; i < nobj; ++i) m->ob_order[i] = i;
        const std::vector<gm_wall_object> &h = m->ob_host;
        std::sort(m->ob_order.begin(), m->ob_order.end(), [&h](uint32_t x, uint32_t y) {
            return h[x].label != h[y].label ? h[x].label < h[y].label : h[x].sign < h[y].sign;
        });
        if (objects && fits)
            for (uint32_t i = 0; i < nobj; ++i) objects[i] = h[m->ob_order[i]];
    }
    if (object_of_row) {
        if (ncomp) {
            m->ob_pos.assign((size_t)ncomp, -1);
            for (uint32_t i = 0; i < nobj; ++i) m->ob_pos[m->ob_host_slot[m->ob_order[i]]] = (int32_t)i;
            GMW_HIP(ctx, hipMemcpyAsync(const_cast<int32_t *>(a.pos), m->ob_pos.data(), (size_t)ncomp * 4, hipMemcpyHostToDevice, m->stream));
            launch_wall_object_rows(a, m->stream);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(object_of_row, a.object_of_row, (size_t)n_rows * 4, hipMemcpyDeviceToHost, m->stream));
            GMW_HIP(ctx, hipStreamSynchronize(m->stream));
        } else {
            std::fill(object_of_row, object_of_row + n_rows, -1);
        }
    }
    if (!fits && (objects || capacity)) return gm_fail(ctx, GM_ERR_CAPACITY, who);
    return GM_OK;
}

}  // namespace

namespace gm {
void gm_wall_free_all(gm_ctx *ctx)
{
    for (gm_wall_map *m : ctx->walls) free_map(m);
    ctx->walls.clear();
}
}  // namespace gm

extern "C" {

void gm_wall_default_params(gm_wall_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_params);
    p->n_stations = 4000;
    p->n_sectors = 90;
    p->station_length = 0.25;
    p->t_min = 0.0;
    p->gate = 0.25;
    p->direction[0] = 1.0;
    p->radius = 2.0;
    p->up[2] = 1.0;
    p->forward[0] = 1.0;
}

gm_status gm_wall_map_create(gm_ctx *ctx, const gm_wall_params *params, gm_wall_map **map)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!map) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create: NULL map");
    *map = nullptr;
    if (check_params(params) != GM_OK)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_create: NULL, struct_size mismatch or a parameter outside its limits");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    gm_wall_map *m = new gm_wall_map;
    m->ctx = ctx;
    m->prm = *params;
    m->ncell = (uint64_t)params->n_stations * params->n_sectors;
    m->pending.assign(ctx->n_slots, 0);
    m->checks.resize(ctx->n_slots);
    m->locates.resize(ctx->n_slots);
    m->aligns.resize(ctx->n_slots);
    if (const char *e = getenv("GM_WALL_ALIGN_ROWS")) m->align_rows = (uint32_t)strtoul(e, nullptr, 10);   // 0: the default
    if (const char *e = getenv("GM_WALL_POINTS_PER_BLOCK")) m->points_per_block = (uint32_t)strtoul(e, nullptr, 10);
    if (const char *e = getenv("GM_WALL_REGION_TILE")) {   // <stations>x<sectors>; anything else: the default
        unsigned ts = 0, tk = 0;
        if (sscanf(e, "%ux%u", &ts, &tk) == 2 && ts >= 1u && tk >= 1u && (uint64_t)ts * tk <= kWallRegionTileCells) {
            m->region_ts = ts;
            m->region_tk = tk;
        }
    }
    if (const char *e = getenv("GM_WALL_OBJECT_TILE")) {   // <block rows>x<block columns>; anything else: the default
        unsigned tr = 0, tc = 0;
        if (sscanf(e, "%ux%u", &tr, &tc) == 2 && tr >= 1u && tc >= 1u && (uint64_t)tr * tc <= kWallObjectTileBlocks) {
            m->object_tr = tr;
            m->object_tc = tc;
        }
    }
    if (const char *e = getenv("GM_WALL_CLOUD_CHUNK")) {   // blocks; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->cloud_chunk = v < kStageCells ? (uint32_t)v : 0u;
    }
    if (const char *e = getenv("GM_WALL_CLEAR_CHUNK")) {   // cells; 0 or more than the default: the default (scratch is sized by it)
        const unsigned long long v = strtoull(e, nullptr, 10);
        m->clear_chunk = v < kStageCells ? (uint32_t)v : 0u;
    }
    design_frame(m);
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

void gm_wall_map_destroy(gm_wall_map *map)
{
    if (!map) return;
    std::vector<gm_wall_map *> &w = map->ctx->walls;
    w.erase(std::remove(w.begin(), w.end(), map), w.end());
    free_map(map);
}

gm_status gm_wall_map_add_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12], gm_wall_add_info *add_info)
{
    if (!map || !ctx) return GM_ERR_INVALID_ARG;
    if (ctx != map->ctx) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_add_frame: the map belongs to another context");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    Slot &sl = ctx->slots[slot];
    if (!sl.submitted) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_add_frame: the slot holds no frame");
    WallArgs w;
    GMW_OK(add_frame_args(map, pose, add_info, w));
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    w.pts = sl.crop4;
    w.labels = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) ? sl.labels : nullptr;   // (label 1 exists with the plane RANSAC only)
    w.n_ptr = &sl.ctr->n_valid;
    w.n_host = sl.n_in;
    // a check enqueued on another slot before this add must not see it (nothing to wait for on a map without checks)
    for (uint32_t i = 0; i < ctx->n_slots; ++i)
        if (i != slot && map->checks[i].outstanding) GMW_HIP(ctx, hipStreamWaitEvent(sl.stream, map->checks[i].done, 0));
    GMW_OK(add_wait_locates(map, slot, sl.stream));   // (nor a locate)
    GMW_OK(add_wait_aligns(map, slot, sl.stream));    // (nor an align)
    launch_wall_add(w, sl.n_in, map->points_per_block, sl.stream);
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
    GMW_OK(add_frame_args(map, pose, add_info, w));
    StageCall sc{map, n, residual, cell, nullptr, nullptr};
    GMW_OK(sc.open());
    GMW_OK(sc.upload(xyz, labels, w));
    hipStream_t s = sc.sl->stream;
    for (uint32_t i = 1; i < ctx->n_slots; ++i)   // (as gm_wall_map_add_frame: behind the checks outstanding on other slots)
        if (map->checks[i].outstanding) GMW_HIP(ctx, hipStreamWaitEvent(s, map->checks[i].done, 0));
    GMW_OK(add_wait_locates(map, 0, s));
    GMW_OK(add_wait_aligns(map, 0, s));
    launch_wall_add(w, n, map->points_per_block, s);
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
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_info);
    info->status = map->status;
    info->n_stations = map->prm.n_stations;
    info->n_sectors = map->prm.n_sectors;
    info->frames = map->frames;
    info->mapped = tot[0]; info->outside = tot[1]; info->beyond_gate = tot[2]; info->plane = tot[3];
    info->cells_hit = tot[4];
    for (int k = 0; k < 3; ++k) { info->o[k] = map->o[k]; info->a[k] = map->a[k]; info->u[k] = map->u[k]; info->v[k] = map->v[k]; }
    info->R = map->R;
    return GM_OK;
}

gm_status gm_wall_map_read(gm_wall_map *map, uint32_t station0, uint32_t n, gm_surface_cell *cells, uint64_t capacity,
                           uint64_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    GMW_OK(check_window(map, station0, n, capacity, n_out, "gm_wall_map_read: cell buffer too small"));
    if (!n) return sync_map(map);
    if (!cells) return gm_fail(map->ctx, GM_ERR_INVALID_ARG, "gm_wall_map_read: NULL cells");
    GMW_OK(sync_map(map));
    return read_window(map, station0, n, cells, false);
}

gm_status gm_wall_map_read_raw(gm_wall_map *map, uint32_t station0, uint32_t n, gm_wall_raw_cell *cells, uint64_t capacity,
                               uint64_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    GMW_OK(check_window(map, station0, n, capacity, n_out, "gm_wall_map_read_raw: cell buffer too small"));
    if (!n) return sync_map(map);
    if (!cells) return gm_fail(map->ctx, GM_ERR_INVALID_ARG, "gm_wall_map_read_raw: NULL cells");
    GMW_OK(sync_map(map));
    return read_window(map, station0, n, cells, true);
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

void gm_wall_region_default_params(gm_wall_region_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_region_params);
    p->min_count = 8;
    p->min_cells = 4;
    p->connectivity = 8;
    p->threshold = 0.05;
}

gm_status gm_wall_region_metrics(const gm_wall_params *p, const gm_wall_region *r, struct gm_wall_region_metrics *out)
{
    if (!p || !r || !out || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || r->cells < 1u) return GM_ERR_INVALID_ARG;
    if (!extent_metrics(*p, *r, out)) return GM_ERR_INVALID_ARG;
    const uint32_t ns = p->n_sectors;
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double two_pi = 6.283185307179586476925286766559;
    const double sr = p->station_length * p->radius;
    const double ring = sr * two_pi;
    const double cell_area = ring / (double)ns;
    const double sum_m = (double)r->sum_d * 0x1p-20;
    out->area_m2 = (double)r->cells * cell_area;
    out->volume_m3 = sum_m * cell_area;
    out->peak_m = (double)r->peak * 0x1p-20;
    out->mean_m = sum_m / (double)r->cells;
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
    if (rp.struct_size != sizeof(gm_wall_region_params) || rp.min_count < 1u || rp.min_cells < 1u ||
        (rp.connectivity != 4u && rp.connectivity != 8u) || !(rp.threshold > 0.0) || !(rp.threshold <= 8.0))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: struct_size mismatch or a parameter outside its limits");
    const long long T = (long long)rint(rp.threshold * 1048576.0);
    if (T < 1) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: the threshold rounds to 0");
    if (!regions && capacity) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: NULL regions with a capacity");
    if (baseline) {
        if (baseline == map) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: the baseline is the map itself");
        if (baseline->ctx != ctx) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: the baseline belongs to another context");
        const gm_wall_params &p = map->prm, &b = baseline->prm;
        if (p.n_stations != b.n_stations || p.n_sectors != b.n_sectors || memcmp(&p.station_length, &b.station_length, 8) ||
            memcmp(&p.t_min, &b.t_min, 8) || memcmp(p.point, b.point, 24) || memcmp(p.direction, b.direction, 24) ||
            memcmp(&p.radius, &b.radius, 8) || memcmp(p.up, b.up, 24) || memcmp(p.forward, b.forward, 24))
            return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_regions: the baseline is a map on another grid");
    }
    GMW_OK(check_window(map, station0, n, ~0ull, nullptr, ""));
    GMW_OK(sync_map(map));
    if (baseline) {
        GMW_OK(sync_map(baseline));
    }
    const uint32_t nsec = map->prm.n_sectors;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_regions_info);
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    info->threshold_q = T;
    info->cell_area = map->prm.station_length * map->prm.radius * 6.283185307179586476925286766559 / (double)nsec;
    if (!n) return GM_OK;

    const uint64_t total = (uint64_t)n * nsec;
    WallRegionArgs a;
    memset(&a, 0, sizeof(a));
    a.map = map->table;
    a.has_base = baseline ? 1u : 0u;
    a.base = baseline ? baseline->table : map->table;
    a.n = n;
    a.nsec = nsec;
    a.first = (uint64_t)station0 * nsec;
    a.ts = map->region_ts;
    a.tk = map->region_tk;
    a.tiles_s = (n + a.ts - 1u) / a.ts;
    a.tiles_k = (nsec + a.tk - 1u) / a.tk;
    a.conn8 = rp.connectivity == 8u ? 1u : 0u;
    a.min_count = rp.min_count;
    a.min_cells = rp.min_cells;
    a.T = T;
    GMW_HIP(ctx, map->rg_cells.reserve(total * (8 + 4 + 4)));
    GMW_HIP(ctx, map->rg_ctr.reserve(kWallRegionCounters));
    Carve cells{map->rg_cells.p};
    a.d = cells.take<long long>(total);
    a.parent = cells.take<uint32_t>(total);
    a.slot = cells.take<uint32_t>(total);
    a.ctr = map->rg_ctr.p;
    unsigned long long ctr[kWallRegionCounters];
    GMW_HIP(ctx, hipMemsetAsync(a.ctr, 0, kWallRegionCounters * 8, map->stream));
    launch_wall_region_label(a, map->stream);
    GMW_HIP(ctx, hipGetLastError());
    GMW_HIP(ctx, hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, map->stream));
    GMW_HIP(ctx, hipStreamSynchronize(map->stream));   // the one count the host needs: it sizes the records
    const uint64_t ncomp = ctr[4];
    info->flagged_pos = ctr[0]; info->flagged_neg = ctr[1]; info->unusable = ctr[2]; info->empty = ctr[3];
    info->components = ncomp;
    uint64_t nreg = 0;
    if (ncomp) {
        GMW_HIP(ctx, map->rg_recs.reserve(ncomp * (sizeof(WallRegionAcc) + sizeof(gm_wall_region))));
        Carve recs{map->rg_recs.p};
        a.acc = recs.take<WallRegionAcc>(ncomp);
        a.out = recs.take<gm_wall_region>(ncomp);
        a.ncomp = (uint32_t)ncomp;
        GMW_HIP(ctx, hipMemsetAsync(a.acc, 0, ncomp * sizeof(WallRegionAcc), map->stream));
        launch_wall_region_reduce(a, map->stream);
        GMW_HIP(ctx, hipGetLastError());
        GMW_HIP(ctx, hipMemcpyAsync(&nreg, a.ctr + 5, 8, hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
    }
    info->regions = nreg;
    if (n_out) *n_out = (uint32_t)nreg;
    const bool fits = nreg <= capacity;
    if (regions && fits && nreg) {
        GMW_HIP(ctx, hipMemcpyAsync(regions, a.out, nreg * sizeof(gm_wall_region), hipMemcpyDeviceToHost, map->stream));
        GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        std::sort(regions, regions + nreg, [](const gm_wall_region &x, const gm_wall_region &y) { return x.label < y.label; });
    }
    if (cell_labels) {
        int32_t *stage = reinterpret_cast<int32_t *>(map->stage.p);   // (kStageCells raw records: room for as many labels)
        const uint64_t chunk = std::min(kStageCells, map->ncell);
        for (uint64_t done = 0; done < total; done += chunk) {
            const uint64_t c = std::min(chunk, total - done);
            launch_wall_region_labels(a, done, c, stage, map->stream);
            GMW_HIP(ctx, hipGetLastError());
            GMW_HIP(ctx, hipMemcpyAsync(cell_labels + done, stage, c * 4, hipMemcpyDeviceToHost, map->stream));
            GMW_HIP(ctx, hipStreamSynchronize(map->stream));
        }
    }
    if (!fits && (regions || capacity)) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_regions: region buffer too small");
    return GM_OK;
}

void gm_wall_cloud_default_params(gm_wall_cloud_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_cloud_params);
    p->block_stations = 1;
    p->block_sectors = 1;
    p->min_count = 1;
    p->exaggeration = 1.0;
}

gm_status gm_wall_cloud_directions(const gm_wall_params *p, const gm_wall_cloud_params *c, double *cos_sin, uint32_t capacity,
                                   uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return GM_ERR_INVALID_ARG;
    if (c && (c->struct_size != sizeof(gm_wall_cloud_params) || c->block_sectors < 1u)) return GM_ERR_INVALID_ARG;
    if (!cos_sin && capacity) return GM_ERR_INVALID_ARG;
    const uint32_t bk = std::min(c ? c->block_sectors : 1u, p->n_sectors);
    const uint32_t NK = (p->n_sectors + bk - 1u) / bk;
    if (n_out) *n_out = NK;
    if (capacity < NK) return GM_ERR_CAPACITY;
    cloud_directions(p->n_sectors, bk, cos_sin);
    return GM_OK;
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
    if (!n) return GM_OK;

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
    for (int k = 0; k < 3; ++k) {
        a.oa[k] = map->o[k] - cp.anchor[k];
        a.a[k] = map->a[k]; a.u[k] = map->u[k]; a.v[k] = map->v[k];
    }
    a.R = map->R;
    a.g = cp.exaggeration;
    a.t_min = map->prm.t_min;
    a.ds = map->prm.station_length;
    a.out = map->cl_stage.p;
    a.ctr = map->cl_ctr.p;

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
        launch_wall_cloud_compact(a, map->cl_scan.next(map->stream), map->stream);
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
    if (n_out) *n_out = total;
    if (points && total > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_wall_map_cloud: point buffer too small");
    return GM_OK;
}

void gm_wall_clearance_default_params(gm_wall_clearance_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_clearance_params);
    p->reference = GM_WALL_CLEAR_MIN;
    p->min_count = 8;
    p->margin = 0.10;
}

gm_status gm_wall_clearance_check_params(const gm_wall_params *p, const gm_wall_clearance_params *c, const int32_t *gauge_q,
                                         uint32_t n_gauges, const uint8_t *station_gauge, uint32_t n)
{
    long long T, Rq;
    const gm_wall_clearance_params cp = params_or(c, gm_wall_clearance_default_params);
    return clearance_ok(p, cp, gauge_q, n_gauges, station_gauge, n, T, Rq) ? GM_OK : GM_ERR_INVALID_ARG;
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

gm_status gm_wall_gauge_from_polygon(const gm_wall_params *p, const double *uv, uint32_t n_vertices, const double offset[2],
                                     int32_t *gauge_q, uint32_t capacity, uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || !uv || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return GM_ERR_INVALID_ARG;
    if (n_vertices < 3u || n_vertices > GM_WALL_GAUGE_MAX_VERTICES || (!gauge_q && capacity)) return GM_ERR_INVALID_ARG;
    if (offset && (!isfinite(offset[0]) || !isfinite(offset[1]))) return GM_ERR_INVALID_ARG;
    const uint32_t ns = p->n_sectors, nv = n_vertices;
    std::vector<double> P(2 * (size_t)nv);
    for (uint32_t i = 0; i < nv; ++i) {
        P[2 * i] = uv[2 * i] + (offset ? offset[0] : 0.0);
        P[2 * i + 1] = uv[2 * i + 1] + (offset ? offset[1] : 0.0);
    }
    if (!gauge_polygon_ok(P, nv)) return GM_ERR_INVALID_ARG;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<double> dirs(2 * (size_t)ns + 2), r(nv);
    for (uint32_t k = 0; k < ns; ++k) {
        const double f = (double)k / (double)ns;
        const double phi = two_pi * f;
        dirs[2 * k] = cos(phi);
        dirs[2 * k + 1] = sin(phi);
    }
    dirs[2 * ns] = dirs[0]; dirs[2 * ns + 1] = dirs[1];   // the last ray is the first
    for (uint32_t i = 0; i < nv; ++i) r[i] = sqrt(P[2 * i] * P[2 * i] + P[2 * i + 1] * P[2 * i + 1]);
    // where the ray of every sector start leaves the polygon at the farthest: the largest t >= 0 over the edges it meets
    std::vector<double> ray(ns, -1.0);
    for (uint32_t k = 0; k < ns; ++k) {
        const double *d = &dirs[2 * k];
        for (uint32_t i = 0; i < nv; ++i) {
            const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
            const double e[2] = {b[0] - a[0], b[1] - a[1]};
            const double den = cross2(e, d);
            if (den == 0.0) continue;   // parallel: its ends are vertices of the wedge
            const double s = -cross2(a, d) / den;
            if (!(s >= 0.0) || !(s <= 1.0)) continue;
            const double x[2] = {a[0] + s * e[0], a[1] + s * e[1]};
            const double t = x[0] * d[0] + x[1] * d[1];
            if (t >= 0.0 && t > ray[k]) ray[k] = t;
        }
    }
    std::vector<int32_t> out(ns);
    for (uint32_t k = 0; k < ns; ++k) {
        const double *d0 = &dirs[2 * k], *d1 = &dirs[2 * k + 2];
        double g = std::max(ray[k], ray[(k + 1u) % ns]);
        for (uint32_t i = 0; i < nv; ++i) {
            const double *v = &P[2 * i];
            if (ns == 1u || (cross2(d0, v) >= 0.0 && cross2(v, d1) >= 0.0)) g = std::max(g, r[i]);
        }
        const double q = ceil(g * 1048576.0);
        if (!(g > 0.0) || !(q < 2147483648.0)) return GM_ERR_INVALID_ARG;
        out[k] = (int32_t)q;
    }
    if (n_out) *n_out = ns;
    if (capacity < ns) return GM_ERR_CAPACITY;
    memcpy(gauge_q, out.data(), (size_t)ns * sizeof(int32_t));
    return GM_OK;
}

gm_status gm_wall_clearance_runs(const gm_wall_params *p, const gm_wall_clearance_station *stations, uint32_t n,
                                 uint32_t station0, uint32_t max_gap, gm_wall_clearance_run *runs, uint32_t capacity,
                                 uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || (!stations && n) || (!runs && capacity) ||
        (uint64_t)station0 + n > 4294967296ull)
        return GM_ERR_INVALID_ARG;
    auto flagged = [&](uint32_t i) { return stations[i].tight + stations[i].infringed > 0u; };
    std::vector<gm_wall_clearance_run> out;
    for (uint32_t i = 0; i < n;) {
        if (!flagged(i)) { ++i; continue; }
        uint32_t last = i;
        for (uint32_t j = i + 1u; j < n && (uint64_t)j - last <= (uint64_t)max_gap + 1u; ++j)
            if (flagged(j)) last = j;
        gm_wall_clearance_run r;
        memset(&r, 0, sizeof(r));
        r.station_from = station0 + i;
        r.station_to = station0 + last;
        uint32_t at = i;
        for (uint32_t j = i; j <= last; ++j) {
            if (stations[j].min_clearance < stations[at].min_clearance) at = j;
            r.tight += stations[j].tight;
            r.infringed += stations[j].infringed;
        }
        // one operation per statement: the same roundings as the twin's, whatever the compiler may contract
        const double from = (double)r.station_from * p->station_length;
        const double to = ((double)r.station_to + 1.0) * p->station_length;
        r.chainage_from = p->t_min + from;
        r.chainage_to = p->t_min + to;
        r.min_clearance = stations[at].min_clearance;
        r.min_clearance_m = (double)r.min_clearance * 0x1p-20;
        r.min_station = station0 + at;
        r.min_sector = stations[at].min_sector;
        const double num = 360.0 * ((double)r.min_sector * 2.0 + 1.0);
        r.angle_deg = num / ((double)p->n_sectors * 2.0);
        out.push_back(r);
        i = last + 1u;
    }
    if (n_out) *n_out = (uint32_t)out.size();
    if (runs && capacity < out.size()) return GM_ERR_CAPACITY;
    if (runs && !out.empty()) memcpy(runs, out.data(), out.size() * sizeof(gm_wall_clearance_run));
    return GM_OK;
}

void gm_wall_check_default_params(gm_wall_check_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_check_params);
    p->reference = GM_WALL_CHECK_MEAN;
    p->min_count = 8;
    p->threshold = 0.05;
    p->gate = 1.0;
}

gm_status gm_wall_check_classify(const gm_wall_check_params *prm, const gm_wall_raw_cell *cell, float e, int64_t *delta, uint32_t *cls)
{
    long long T;
    if (!prm || !cell || !delta || !cls || !check_prm_ok(*prm, T)) return GM_ERR_INVALID_ARG;
    *delta = 0;
    if (!(fabsf(e) <= (float)prm->gate)) {
        *cls = GM_WALL_CHECK_CLS_BEYOND_GATE;
        return GM_OK;
    }
    long long d;
    *cls = wall_check_rule(prm->reference, prm->min_count, T, cell->sum, cell->count, cell->min_key, cell->max_key, e, d);
    *delta = d;
    return GM_OK;
}

gm_status gm_wall_map_check_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_check_params *prm, gm_wall_add_info *add_info)
{
    if (!map || !ctx) return GM_ERR_INVALID_ARG;
    if (ctx != map->ctx) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_frame: the map belongs to another context");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    const gm_wall_check_params cp = params_or(prm, gm_wall_check_default_params);
    WallCheckArgs a;
    memset(&a, 0, sizeof(a));
    if (!check_prm_ok(cp, a.T))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_frame: struct_size mismatch or a parameter outside its limits");
    Slot &sl = ctx->slots[slot];
    if (!sl.submitted) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_check_frame: the slot holds no frame");
    GMW_OK(add_frame_args(map, pose, add_info, a.w));
    a.w.gate = (float)cp.gate;
    if (add_info) add_info->gate = a.w.gate;
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t n_cap = sl.n_in ? sl.n_in : 1u;
    ScanState scan;
    GMW_OK(check_prepare(map, slot, n_cap, sl.stream, scan));
    GMW_OK(check_wait_adds(map, slot, sl.stream));
    a.w.pts = sl.crop4;
    a.w.labels = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) ? sl.labels : nullptr;
    a.w.n_ptr = &sl.ctr->n_valid;
    a.w.n_host = sl.n_in;
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    a.out = map->checks[slot].stage.p;
    a.ctr = map->checks[slot].ctr.p;
    return check_enqueue(map, slot, a, n_cap, scan, sl.stream);
}

gm_status gm_wall_map_get_check(gm_wall_map *map, uint32_t slot, gm_wall_check_info *info, gm_wall_check_point *points,
                                uint32_t capacity, uint32_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->checks[slot].have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_check: no check was enqueued on this map and slot");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
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
    GMW_OK(add_frame_args(map, pose, add_info, a.w));
    a.w.gate = (float)cp.gate;
    if (add_info) add_info->gate = a.w.gate;
    StageCall sc{map, n, residual, cell, delta, cls};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    const uint32_t n_cap = n ? n : 1u;
    ScanState scan;
    GMW_OK(check_prepare(map, 0, n_cap, s, scan));
    GMW_OK(check_wait_adds(map, 0, s));
    GMW_OK(sc.upload(xyz, labels, a.w));
    a.delta = delta ? map->ck_delta.p : nullptr;
    a.cls = cls ? map->ck_cls.p : nullptr;
    a.reference = cp.reference;
    a.min_count = cp.min_count;
    a.row_is_index = 1u;
    a.out = map->checks[0].stage.p;
    a.ctr = map->checks[0].ctr.p;
    GMW_OK(check_enqueue(map, 0, a, n_cap, scan, s));
    GMW_OK(sc.close());
    return check_result(map, 0, info, points, capacity, n_out);
}

void gm_wall_locate_default_params(gm_wall_locate_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_locate_params);
    p->reference = GM_WALL_LOCATE_DESIGN;
    p->min_count = 8;
    p->gate = 0.25;
}

gm_status gm_wall_locate_check_params(const gm_wall_locate_params *p)
{
    return p && locate_prm_ok(*p) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_map_locate_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                   const gm_wall_locate_params *prm)
{
    if (!map || !ctx) return GM_ERR_INVALID_ARG;
    if (ctx != map->ctx) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_locate_frame: the map belongs to another context");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    const gm_wall_locate_params lp = params_or(prm, gm_wall_locate_default_params);
    if (!locate_prm_ok(lp))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_locate_frame: struct_size mismatch or a parameter outside its limits");
    Slot &sl = ctx->slots[slot];
    if (!sl.submitted) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_locate_frame: the slot holds no frame");
    WallLocateArgs a;
    GMW_OK(locate_args(map, slot, pose, lp, a));
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    GMW_OK(locate_prepare(map, slot, sl.stream, a));
    GMW_OK(check_wait_adds(map, slot, sl.stream));
    a.w.pts = sl.crop4;
    a.w.labels = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) ? sl.labels : nullptr;
    a.w.n_ptr = &sl.ctr->n_valid;
    a.w.n_host = sl.n_in;
    return locate_enqueue(map, slot, a, sl.stream);
}

gm_status gm_wall_map_get_locate(gm_wall_map *map, uint32_t slot, gm_wall_locate_info *info)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_get_locate: NULL info");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->locates[slot].have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_locate: no locate was enqueued on this map and slot");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
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
    WallLocateSlot &l = map->locates[0];
    const int64_t anchor = l.anchor;   // (a refused call leaves the slot's last result as it was)
    const double of[3] = {l.of[0], l.of[1], l.of[2]};
    WallLocateArgs a;
    GMW_OK(locate_args(map, 0, pose, lp, a));
    StageCall sc{map, n, residual, cell, nullptr, nullptr};
    gm_status st = sc.open();
    if (st == GM_OK) st = locate_prepare(map, 0, sc.sl->stream, a);
    if (st != GM_OK) {
        l.anchor = anchor;
        for (int k = 0; k < 3; ++k) l.of[k] = of[k];
        return st;
    }
    hipStream_t s = sc.sl->stream;
    GMW_OK(check_wait_adds(map, 0, s));
    GMW_OK(sc.upload(xyz, labels, a.w));
    GMW_OK(locate_enqueue(map, 0, a, s));
    GMW_OK(sc.close());
    return locate_result(map, 0, info);
}

void gm_wall_align_default_params(gm_wall_align_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_align_params);
    p->half_patch_stations = 20;
    p->max_station_shift = 8;
    p->max_sector_shift = 4;
    p->min_count = 8;
    p->min_frame_count = 4;
    p->min_overlap = 64;
    p->gate = 0.25;
    p->clip = 0.05;
    p->min_distinction = 1.5;
}

gm_status gm_wall_align_check_params(const gm_wall_align_params *p, uint32_t n_sectors)
{
    return p && align_prm_ok(*p, n_sectors) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_align_select(const gm_wall_params *wall, const gm_wall_align_params *prm, const double pose[12],
                               const gm_wall_align_score *table, uint32_t n_scores, gm_wall_align_info *info)
{
    if (!wall || !pose || !table || !info || check_params(wall) != GM_OK) return GM_ERR_INVALID_ARG;
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    if (!align_prm_ok(ap, wall->n_sectors)) return GM_ERR_INVALID_ARG;
    if (n_scores != (2u * ap.max_station_shift + 1u) * (2u * ap.max_sector_shift + 1u)) return GM_ERR_INVALID_ARG;
    double Rm[3][3], tr[3];
    if (pose_split(pose, Rm, tr)) return GM_ERR_INVALID_ARG;
    DesignFrame d;
    design_frame_of(*wall, d);
    const double rel[3] = {tr[0] - d.o[0], tr[1] - d.o[1], tr[2] - d.o[2]};
    if (!(fabs(floor((dot(rel, d.a) - wall->t_min) / wall->station_length)) < 4.0e18)) return GM_ERR_INVALID_ARG;
    align_select(d, *wall, ap, Rm, tr, table, info);
    return GM_OK;
}

gm_status gm_wall_map_align_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_align_params *prm, gm_wall_add_info *add_info)
{
    if (!map || !ctx) return GM_ERR_INVALID_ARG;
    if (ctx != map->ctx) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_align_frame: the map belongs to another context");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    if (!align_prm_ok(ap, map->prm.n_sectors))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_align_frame: struct_size mismatch or a parameter outside its limits");
    Slot &sl = ctx->slots[slot];
    if (!sl.submitted) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_align_frame: the slot holds no frame");
    WallAlignArgs a;
    GMW_OK(align_args(map, pose, ap, add_info, a));
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    GMW_OK(align_prepare(map, slot, sl.stream, a));
    a.w.pts = sl.crop4;
    a.w.labels = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) ? sl.labels : nullptr;
    a.w.n_ptr = &sl.ctr->n_valid;
    a.w.n_host = sl.n_in;
    return align_enqueue(map, slot, a, sl.n_in ? sl.n_in : 1u, ap, pose, sl.stream);
}

gm_status gm_wall_map_get_align(gm_wall_map *map, uint32_t slot, gm_wall_align_info *info, gm_wall_align_score *scores,
                                uint32_t capacity, uint32_t *n_out)
{
    if (!map) return GM_ERR_INVALID_ARG;
    gm_ctx *ctx = map->ctx;
    if (n_out) *n_out = 0;
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!map->aligns[slot].have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_get_align: no align was enqueued on this map and slot");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
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
    StageCall sc{map, n, residual, cell, nullptr, nullptr};
    GMW_OK(sc.open());
    hipStream_t s = sc.sl->stream;
    GMW_OK(align_prepare(map, 0, s, a));
    GMW_OK(sc.upload(xyz, labels, a.w));
    GMW_OK(align_enqueue(map, 0, a, n ? n : 1u, ap, pose, s));
    GMW_OK(sc.close());
    return align_result(map, 0, info, scores, capacity, n_out);
}

void gm_wall_object_default_params(gm_wall_object_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_wall_object_params);
    p->block_stations = 1;
    p->block_sectors = 1;
    p->min_block_points = 2;
    p->min_points = 8;
    p->connectivity = 8;
    p->half_window_stations = 128;
}

gm_status gm_wall_object_metrics(const gm_wall_params *p, const gm_wall_object_params *op, const gm_wall_object *o,
                                 struct gm_wall_object_metrics *out)
{
    if (!p || !o || !out || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || o->points < 1u) return GM_ERR_INVALID_ARG;
    if (op && op->struct_size != sizeof(gm_wall_object_params)) return GM_ERR_INVALID_ARG;
    if (!extent_metrics(*p, *o, out)) return GM_ERR_INVALID_ARG;
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double pts = (double)o->points;
    const double sx = (double)o->sum_x * 0x1p-16, sy = (double)o->sum_y * 0x1p-16, sz = (double)o->sum_z * 0x1p-16;
    out->centroid[0] = sx / pts;
    out->centroid[1] = sy / pts;
    out->centroid[2] = sz / pts;
    const double sum_m = (double)o->sum_delta * 0x1p-20;
    out->mean_m = sum_m / pts;
    out->peak_m = (double)o->peak * 0x1p-20;
    for (int k = 0; k < 3; ++k) out->size[k] = (double)o->box_max[k] - (double)o->box_min[k];
    return GM_OK;
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
    if (!c.have) return gm_fail(ctx, GM_ERR_NOT_READY, "gm_wall_map_check_objects: no check was enqueued on this map and slot");
    ObjectWindow win;
    if (!object_window(map->prm, op, c.anchor, win))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_map_check_objects: the window holds more than GM_WALL_OBJECT_MAX_BLOCKS blocks");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    if (c.outstanding) {   // that check only: the slot's stream may be busy with the next frame
        GMW_HIP(ctx, hipEventSynchronize(c.done));
        c.outstanding = false;
    }
    const uint32_t n_rows = (uint32_t)c.h_ctr[9];
    const bool rows_fit = !object_of_row || row_capacity >= n_rows;
    // (a check's own rows are never rejected: with nothing to launch they are all outside the window)
    const gm_status st = objects_run(map, c.stage.p, n_rows, 0u, op, win, info, objects, capacity, n_out, rows_fit ? object_of_row : nullptr,
                                     "gm_wall_map_check_objects: object buffer too small");
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
    if (!object_window(map->prm, op, anchor_station, win))
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_wall_check_objects: the window holds more than GM_WALL_OBJECT_MAX_BLOCKS blocks");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    uint32_t rejected = 0;
    if (n_rows && !win.nJ) {   // nothing will be launched: the one class that needs the rows, on the host
        for (uint32_t i = 0; i < n_rows; ++i) {
            uint32_t b[5];
            memcpy(b, &rows[i], sizeof(b));   // x y z delta e
            if (wall_object_rejected(b[0], b[1], b[2], b[4], rows[i].cell, wall_check_fix(rows[i].delta), (uint32_t)map->ncell)) ++rejected;
        }
    } else if (n_rows) {
        GMW_HIP(ctx, map->ob_rows.reserve(n_rows));
        GMW_HIP(ctx, hipMemcpyAsync(map->ob_rows.p, rows, (size_t)n_rows * sizeof(gm_wall_check_point), hipMemcpyHostToDevice, map->stream));
    }
    return objects_run(map, map->ob_rows.p, n_rows, rejected, op, win, info, objects, capacity, n_out, object_of_row,
                       "gm_wall_check_objects: object buffer too small");
}

}  // extern "C"
