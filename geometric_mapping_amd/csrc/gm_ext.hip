// gm_ext.hip -- C ABI entry points of the build-defined extensions (RANSAC
// scoring, segment moments, 1-NN, labels, compressed map).  Host logic only;
// kernels are in k_ransac.hip / k_nearest.hip.
#include <math.h>
#include <string.h>

#include <vector>

#include "gm_internal.hpp"

using namespace gm;

namespace {

#define GMX_HIP(ctx, call)                                                           \
    do {                                                                             \
        hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) {                                                     \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);         \
            return (e__ == hipErrorOutOfMemory) ? GM_ERR_OOM : GM_ERR_DEVICE;        \
        }                                                                            \
    } while (0)

// rows of 3 floats -> device float4 array `dst` (through the slot's pinned staging)
gm_status upload_xyz(gm_ctx *ctx, Slot &sl, const float *xyz, uint32_t n, float4 *dst)
{
    if (!n) return GM_OK;
    float4 *stage = (float4 *)sl.h_raw.p;
    for (uint32_t i = 0; i < n; ++i) stage[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f);
    GMX_HIP(ctx, hipMemcpyAsync(dst, stage, (size_t)n * 16, hipMemcpyHostToDevice, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));  // staging is reused by the caller right away
    return GM_OK;
}

gm_status prepare(gm_ctx *ctx, Slot *&sl, uint32_t n, uint32_t H)
{
    gm_status st = gm_begin_stage(ctx, sl);
    if (st != GM_OK) return st;
    st = gm_ensure_capacity(ctx, *sl, n, (size_t)n * 16, true);
    if (st != GM_OK) return st;
    return gm_ensure_ext(ctx, *sl, H ? H : 1);
}

gm_status upload_labels(gm_ctx *ctx, Slot &sl, const uint8_t *labels, uint32_t n)
{
    if (labels && n) GMX_HIP(ctx, hipMemcpyAsync(sl.labels, labels, n, hipMemcpyHostToDevice, sl.stream));
    return GM_OK;
}

gm_status score(gm_ctx *ctx, int model, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                const float *hyp, uint32_t H, double tau, int32_t *counts)
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || !hyp || !counts) return gm_fail(ctx, GM_ERR_INVALID_ARG, "NULL argument");
    gm_status st = prepare(ctx, slp, n, H);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    // caller rows (4 or 7 floats) -> internal rows of 8
    const int w = model == 0 ? 4 : 7;
    float *stage = (float *)sl.h_raw.p;  // capacity >= n*16 bytes; H*32 must fit too
    if ((size_t)H * 32 > sl.raw_cap) {
        st = gm_ensure_capacity(ctx, sl, n, (size_t)H * 32, true);
        if (st != GM_OK) return st;
        stage = (float *)sl.h_raw.p;
    }
    memset(stage, 0, (size_t)H * 32);
    for (uint32_t h = 0; h < H; ++h)
        for (int k = 0; k < w; ++k) stage[8 * (size_t)h + k] = hyp[(size_t)w * h + k];
    float *dh = model == 0 ? sl.hyp_plane : sl.hyp_cyl;
    GMX_HIP(ctx, hipMemcpyAsync(dh, stage, (size_t)H * 32, hipMemcpyHostToDevice, sl.stream));
    launch_score(model, sl.crop4, labels ? sl.labels : nullptr, want, nullptr, n, dh, sl.band, H, tau, sl.score_partial,
                 sl.cnt_plane, sl.best_plane, sl.stream);
    GMX_HIP(ctx, hipMemcpyAsync(counts, sl.cnt_plane, (size_t)H * 4, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    return GM_OK;
}

}  // namespace

namespace gm {
gm_status gm_upload_xyz(gm_ctx *ctx, Slot &sl, const float *xyz, uint32_t n, float4 *dst) { return upload_xyz(ctx, sl, xyz, n, dst); }
}  // namespace gm

extern "C" {

int gm_ext_available(void) { return 1; }

gm_status gm_score_planes(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                          const float *hyp4, uint32_t H, double tau, int32_t *counts)
{
    return score(ctx, 0, xyz, n, labels, want, hyp4, H, tau, counts);
}

gm_status gm_score_cylinders(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                             const float *hyp7, uint32_t H, double tau, int32_t *counts)
{
    return score(ctx, 1, xyz, n, labels, want, hyp7, H, tau, counts);
}

gm_status gm_score_frame(gm_ctx *ctx, uint32_t slot, int model, const float *hyp, uint32_t H, double tau,
                         uint32_t unlabelled_only, int32_t *counts)
{
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if (!hyp || !counts || (model != 0 && model != 1)) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_score_frame: bad argument");
    if (unlabelled_only && !(ctx->cfg.flags & (GM_CFG_RANSAC_PLANE | GM_CFG_RANSAC_CYLINDER)))
        return gm_fail(ctx, GM_ERR_NOT_READY, "unlabelled_only needs a context created with a GM_CFG_RANSAC_* flag");
    Slot &sl = ctx->slots[slot];
    st = gm_ensure_ext(ctx, sl, H);
    if (st != GM_OK) return st;
    // caller rows (4 or 7 floats) -> internal rows of 8
    const int w = model == 0 ? 4 : 7;
    std::vector<float> rows((size_t)H * 8, 0.f);
    for (uint32_t h = 0; h < H; ++h)
        for (int k = 0; k < w; ++k) rows[8 * (size_t)h + k] = hyp[(size_t)w * h + k];
    float *dh = model == 0 ? sl.hyp_plane : sl.hyp_cyl;
    GMX_HIP(ctx, hipMemcpyAsync(dh, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));  // `rows` is pageable and about to go away
    // exhaustive scorer over the slot's resident valid cloud (owned points only: halo rows never reach it)
    launch_score(model, sl.crop4, unlabelled_only ? sl.labels : nullptr, 0, &sl.ctr->n_valid, sl.last.n_valid, dh, sl.band,
                 H, tau, nullptr, sl.cnt_plane, sl.score_partial + 600, sl.stream);
    GMX_HIP(ctx, hipMemcpyAsync(counts, sl.cnt_plane, (size_t)H * 4, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    return GM_OK;
}

gm_status gm_plane_hypotheses(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                              uint64_t seed, uint32_t H, float *hyp4)
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || !hyp4) return gm_fail(ctx, GM_ERR_INVALID_ARG, "NULL argument");
    gm_status st = prepare(ctx, slp, n, H);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    launch_plane_hypotheses(sl.crop4, labels ? sl.labels : nullptr, want, nullptr, n, seed, H, sl.hyp_plane, nullptr,
                            sl.stream);
    if ((size_t)H * 32 > sl.raw_cap) {
        st = gm_ensure_capacity(ctx, sl, n, (size_t)H * 32, true);
        if (st != GM_OK) return st;
    }
    float *stage = (float *)sl.h_raw.p;
    GMX_HIP(ctx, hipMemcpyAsync(stage, sl.hyp_plane, (size_t)H * 32, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    for (uint32_t h = 0; h < H; ++h)
        for (int k = 0; k < 4; ++k) hyp4[4 * (size_t)h + k] = stage[8 * (size_t)h + k];
    return GM_OK;
}

gm_status gm_cylinder_hypotheses(gm_ctx *ctx, const float *xyz, const float *nxyzc, uint32_t n, const uint8_t *labels,
                                 uint32_t want, uint64_t seed, uint32_t H, float *hyp7)
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && (!xyz || !nxyzc)) || !hyp7) return gm_fail(ctx, GM_ERR_INVALID_ARG, "NULL argument");
    gm_status st = prepare(ctx, slp, n, H);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    if (n) GMX_HIP(ctx, hipMemcpyAsync(sl.normals4, nxyzc, (size_t)n * 16, hipMemcpyHostToDevice, sl.stream));
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    launch_cylinder_hypotheses(sl.crop4, sl.normals4, labels ? sl.labels : nullptr, want, nullptr, n, seed, H, sl.hyp_cyl,
                               nullptr, nullptr, 0.0, sl.stream);
    if ((size_t)H * 32 > sl.raw_cap) {
        st = gm_ensure_capacity(ctx, sl, n, (size_t)H * 32, true);
        if (st != GM_OK) return st;
    }
    float *stage = (float *)sl.h_raw.p;
    GMX_HIP(ctx, hipMemcpyAsync(stage, sl.hyp_cyl, (size_t)H * 32, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    for (uint32_t h = 0; h < H; ++h)
        for (int k = 0; k < 7; ++k) hyp7[7 * (size_t)h + k] = stage[8 * (size_t)h + k];
    return GM_OK;
}

gm_status gm_segment_moments(gm_ctx *ctx, const float *xyz, const float *nxyzc, const uint8_t *labels, uint32_t n,
                             uint32_t label, double mom16[16])
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || !mom16) return gm_fail(ctx, GM_ERR_INVALID_ARG, "NULL argument");
    gm_status st = prepare(ctx, slp, n, 1);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    if (n && nxyzc) GMX_HIP(ctx, hipMemcpyAsync(sl.normals4, nxyzc, (size_t)n * 16, hipMemcpyHostToDevice, sl.stream));
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    launch_segment_moments(sl.crop4, nxyzc ? sl.normals4 : nullptr, labels ? sl.labels : nullptr, label, nullptr, n,
                           sl.mom_partial, sl.mom_plane, sl.stream);
    GMX_HIP(ctx, hipMemcpyAsync(mom16, sl.mom_plane, 16 * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    return GM_OK;
}

gm_status gm_nearest(gm_ctx *ctx, const float *xyz, uint32_t n, const float *queries, uint32_t nq, int32_t *idx_out)
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || (nq && (!queries || !idx_out))) return gm_fail(ctx, GM_ERR_INVALID_ARG, "NULL argument");
    const uint32_t m = n > nq ? n : nq;
    gm_status st = prepare(ctx, slp, m, 1);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    st = upload_xyz(ctx, sl, queries, nq, sl.vox4);
    if (st != GM_OK) return st;
    launch_nearest(sl.crop4, nullptr, n, sl.vox4, nullptr, nq, sl.nn_best, sl.vox_nn, sl.stream);
    if (nq) GMX_HIP(ctx, hipMemcpyAsync(idx_out, sl.vox_nn, (size_t)nq * 4, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    return GM_OK;
}

static gm_status fetch_bytes(gm_ctx *ctx, Slot &sl, const void *dev, uint32_t avail, size_t elem, void *out,
                             uint32_t capacity, uint32_t *n_out)
{
    if (n_out) *n_out = avail;
    if (avail > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "output buffer too small");
    if (!avail) return GM_OK;
    if (!out) return gm_fail(ctx, GM_ERR_INVALID_ARG, "output pointer is NULL");
    GMX_HIP(ctx, hipMemcpyAsync(out, dev, (size_t)avail * elem, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    return GM_OK;
}

gm_status gm_get_voxel_nearest(gm_ctx *ctx, uint32_t slot, int32_t *idx, uint32_t capacity, uint32_t *n_out)
{
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if ((ctx->cfg.flags & (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID)) != (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID))
        return gm_fail(ctx, GM_ERR_NOT_READY, "context created without GM_CFG_NEAREST | GM_CFG_VOXEL_GRID");
    Slot &sl = ctx->slots[slot];
    return fetch_bytes(ctx, sl, sl.vox_nn, sl.last.n_voxels, 4, idx, capacity, n_out);
}

gm_status gm_get_voxel_normals(gm_ctx *ctx, uint32_t slot, float *nxyzc, uint32_t capacity, uint32_t *n_out)
{
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if ((ctx->cfg.flags & (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID)) != (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID))
        return gm_fail(ctx, GM_ERR_NOT_READY, "context created without GM_CFG_NEAREST | GM_CFG_VOXEL_GRID");
    Slot &sl = ctx->slots[slot];
    return fetch_bytes(ctx, sl, sl.vox_nrm4, sl.last.n_voxels, 16, nxyzc, capacity, n_out);
}

gm_status gm_get_labels(gm_ctx *ctx, uint32_t slot, uint8_t *labels, uint32_t capacity, uint32_t *n_out)
{
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if (!(ctx->cfg.flags & (GM_CFG_RANSAC_PLANE | GM_CFG_RANSAC_CYLINDER)))
        return gm_fail(ctx, GM_ERR_NOT_READY, "context created without a GM_CFG_RANSAC_* flag");
    Slot &sl = ctx->slots[slot];
    return fetch_bytes(ctx, sl, sl.labels, sl.last.n_valid, 1, labels, capacity, n_out);
}

gm_status gm_get_cylinder_fit(gm_ctx *ctx, uint32_t slot, gm_cylinder_fit *out)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!(ctx->cfg.flags & GM_CFG_CYLINDER_FIT))
        return gm_fail(ctx, GM_ERR_UNSUPPORTED, "gm_get_cylinder_fit: context created without GM_CFG_CYLINDER_FIT");
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if (!out) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_get_cylinder_fit: NULL argument");
    *out = ctx->slots[slot].last_fit;
    return GM_OK;
}

// getCylinder (tunnel_processing.hpp:56-59, the empty stub of src/tunnel_processing.cpp:149-154) as one stage call: the
// frame's four launches (k_cylfit.hip) on caller buffers
gm_status gm_fit_cylinder(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                          const float init7[7], double tau, gm_cylinder_fit *out, uint8_t *inlier_out)
{
    Slot *slp;
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || !init7 || !out) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_fit_cylinder: NULL argument");
    if (!(tau > 0.0) || !isfinite(tau)) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_fit_cylinder: tau must be > 0");
    gm_status st = prepare(ctx, slp, n, 1);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    float row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 7; ++k) row[k] = init7[k];
    GMX_HIP(ctx, hipMemcpyAsync(sl.fit_init, row, sizeof(row), hipMemcpyHostToDevice, sl.stream));
    if (n) GMX_HIP(ctx, hipMemsetAsync(sl.inl_mask, 0, n, sl.stream));
    CylFitArgs a;
    a.pts = sl.crop4; a.labels = labels ? sl.labels : nullptr; a.out = sl.inl_mask;
    a.want = want; a.want2 = want; a.mask_mode = 1;
    a.n_ptr = nullptr; a.n_host = n;
    a.init = sl.fit_init; a.best = nullptr;
    a.work = sl.fit_work; a.fit = sl.fit_stage; a.partial = sl.fit_partial; a.ticket = sl.fit_ticket;
    a.tau = tau;
    launch_cylinder_fit(a, sl.stream);
    gm_cylinder_fit f;
    GMX_HIP(ctx, hipMemcpyAsync(&f, sl.fit_stage, sizeof(f), hipMemcpyDeviceToHost, sl.stream));
    if (inlier_out && n) GMX_HIP(ctx, hipMemcpyAsync(inlier_out, sl.inl_mask, n, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    GMX_HIP(ctx, hipGetLastError());
    f.struct_size = (uint32_t)sizeof(gm_cylinder_fit);
    *out = f;
    return GM_OK;
}

// ---- wall deviation map (GM_CFG_SURFACE_MAP, k_surface.hip) ----

void gm_surface_default_params(gm_surface_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(gm_surface_params);
    p->n_stations = 40;
    p->n_sectors = 90;
    p->station_length = 0.25;
    p->t_min = -5.0;     // the default crop box is +-5 m
    p->gate = 0.25;
    p->up[2] = 1.0;
    p->forward[0] = 1.0;   // REP-103: x forward
}

gm_status gm_set_surface_params(gm_ctx *ctx, const gm_surface_params *p)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (gm_check_surface_params(p) != GM_OK)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_set_surface_params: NULL, struct_size mismatch or a parameter outside its limits");
    for (uint32_t i = 0; i < ctx->n_slots; ++i)
        if (ctx->slots[i].submitted && !ctx->slots[i].complete)
            return gm_fail(ctx, GM_ERR_NOT_READY, "gm_set_surface_params: a slot holds a submitted frame that has not been waited for");
    if (hipSetDevice(ctx->device) != hipSuccess) return gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
    ctx->surf = *p;
    const SurfParams d = surface_device_params(*p);
    for (uint32_t i = 0; i < ctx->n_slots; ++i) {   // (slots without map buffers upload ctx->surf when they allocate them)
        Slot &sl = ctx->slots[i];
        if (!sl.surf_prm) continue;
        GMX_HIP(ctx, hipMemcpyAsync(sl.surf_prm, &d, sizeof(d), hipMemcpyHostToDevice, sl.stream));
        GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    }
    return GM_OK;
}

gm_status gm_get_surface_map(gm_ctx *ctx, uint32_t slot, gm_surface_info *info, gm_surface_cell *cells, uint32_t capacity,
                             uint32_t *n_out)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!(ctx->cfg.flags & GM_CFG_SURFACE_MAP))
        return gm_fail(ctx, GM_ERR_UNSUPPORTED, "gm_get_surface_map: context created without GM_CFG_SURFACE_MAP");
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    if (!info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_get_surface_map: NULL info");
    Slot &sl = ctx->slots[slot];
    gm_surface_info inf;
    GMX_HIP(ctx, hipMemcpyAsync(&inf, sl.surf_info, sizeof(inf), hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    *info = inf;
    const uint32_t nc = inf.n_stations * inf.n_sectors;
    if (n_out) *n_out = nc;
    if (nc > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_get_surface_map: cell buffer too small");
    if (!nc) return GM_OK;
    if (!cells) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_get_surface_map: NULL cells");
    GMX_HIP(ctx, hipMemcpyAsync(cells, sl.surf_cells, (size_t)nc * sizeof(gm_surface_cell), hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    return GM_OK;
}

gm_status gm_get_surface_points(gm_ctx *ctx, uint32_t slot, float *residual, int32_t *cell, uint32_t capacity, uint32_t *n_out)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if (!(ctx->cfg.flags & GM_CFG_SURFACE_MAP))
        return gm_fail(ctx, GM_ERR_UNSUPPORTED, "gm_get_surface_points: context created without GM_CFG_SURFACE_MAP");
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    Slot &sl = ctx->slots[slot];
    const uint32_t n = sl.last.n_valid;
    if (n_out) *n_out = n;
    if (n > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_get_surface_points: output buffer too small");
    if (!n) return GM_OK;
    if (residual) GMX_HIP(ctx, hipMemcpyAsync(residual, sl.surf_res, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream));
    if (cell) GMX_HIP(ctx, hipMemcpyAsync(cell, sl.surf_cell, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    return GM_OK;
}

// the frame's map launch (k_surface.hip) on caller buffers, with the call's own parameter block and model row
gm_status gm_surface_map(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, const float model7[7],
                         const gm_surface_params *p, gm_surface_info *info, gm_surface_cell *cells, uint32_t capacity,
                         float *residual, int32_t *cell)
{
    if (!ctx) return GM_ERR_INVALID_ARG;
    if ((n && !xyz) || !model7 || !info) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_surface_map: NULL argument");
    gm_surface_params prm;
    if (p) prm = *p;
    else gm_surface_default_params(&prm);
    if (gm_check_surface_params(&prm) != GM_OK)
        return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_surface_map: struct_size mismatch or a parameter outside its limits");
    const uint32_t nc = prm.n_stations * prm.n_sectors;
    if (nc > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "gm_surface_map: cell buffer too small");
    if (!cells) return gm_fail(ctx, GM_ERR_INVALID_ARG, "gm_surface_map: NULL cells");
    Slot *slp;
    gm_status st = gm_begin_stage(ctx, slp);
    if (st != GM_OK) return st;
    Slot &sl = *slp;
    st = gm_ensure_capacity(ctx, sl, n ? n : 1u, (size_t)(n ? n : 1u) * 16, true);
    if (st != GM_OK) return st;
    st = gm_ensure_surface(ctx, sl);
    if (st != GM_OK) return st;
    st = upload_xyz(ctx, sl, xyz, n, sl.crop4);
    if (st != GM_OK) return st;
    st = upload_labels(ctx, sl, labels, n);
    if (st != GM_OK) return st;
    gm_cylinder_fit f;
    memset(&f, 0, sizeof(f));
    f.status = GM_FIT_OK;
    for (int k = 0; k < 7; ++k) f.model[k] = model7[k];
    const SurfParams d = surface_device_params(prm);
    GMX_HIP(ctx, hipMemcpyAsync(sl.surf_fit, &f, sizeof(f), hipMemcpyHostToDevice, sl.stream));
    GMX_HIP(ctx, hipMemcpyAsync(sl.surf_prm + 1, &d, sizeof(d), hipMemcpyHostToDevice, sl.stream));
    SurfArgs a;
    a.pts = sl.crop4; a.labels = labels ? sl.labels : nullptr; a.n_ptr = nullptr; a.n_host = n;
    a.fit = sl.surf_fit; a.prm = sl.surf_prm + 1;
    a.table = sl.surf_table; a.cells = sl.surf_cells; a.info = sl.surf_info; a.res = sl.surf_res; a.cell = sl.surf_cell;
    launch_surface_map(a, n, sl.stream);
    GMX_HIP(ctx, hipGetLastError());
    gm_surface_info inf;
    GMX_HIP(ctx, hipMemcpyAsync(&inf, sl.surf_info, sizeof(inf), hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipMemcpyAsync(cells, sl.surf_cells, (size_t)nc * sizeof(gm_surface_cell), hipMemcpyDeviceToHost, sl.stream));
    if (residual && n) GMX_HIP(ctx, hipMemcpyAsync(residual, sl.surf_res, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream));
    if (cell && n) GMX_HIP(ctx, hipMemcpyAsync(cell, sl.surf_cell, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream));
    GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    *info = inf;
    return GM_OK;
}

gm_status gm_get_compressed_map(gm_ctx *ctx, uint32_t slot, void *buf, size_t capacity, size_t *n_bytes)
{
    gm_status st = gm_check_slot(ctx, slot);
    if (st != GM_OK) return st;
    Slot &sl = ctx->slots[slot];
    const gm_frame_result &r = sl.last;
    uint32_t nprim = 0;
    const bool has_plane = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) && r.plane_inliers > 0 && isfinite(r.plane[0]);
    const bool has_cyl = (ctx->cfg.flags & GM_CFG_RANSAC_CYLINDER) && r.cylinder_inliers > 0 && isfinite(r.cylinder[0]);
    nprim = (has_plane ? 1u : 0u) + (has_cyl ? 1u : 0u);
    const uint32_t nvox = (ctx->cfg.flags & GM_CFG_VOXEL_GRID) ? r.n_voxels : 0;
    const size_t need = sizeof(gm_map_header) + (size_t)nprim * sizeof(gm_map_primitive) + (size_t)nvox * 16;
    if (n_bytes) *n_bytes = need;
    if (need > capacity) return gm_fail(ctx, GM_ERR_CAPACITY, "map buffer too small");
    if (!buf) return gm_fail(ctx, GM_ERR_INVALID_ARG, "map buffer is NULL");
    uint8_t *p = (uint8_t *)buf;
    gm_map_header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "GMAP", 4);
    h.version = 1;
    h.n_primitives = nprim;
    h.n_voxels = nvox;
    h.leaf = (float)ctx->cfg.voxelGridLeafSize;
    h.bound = (float)ctx->cfg.boxFilterBound;
    h.n_points = r.n_valid;
    for (int k = 0; k < 3; ++k) { h.eigenvalues[k] = r.eigenvalues[k]; h.center_axis[k] = r.center_axis[k]; }
    memcpy(p, &h, sizeof(h)); p += sizeof(h);
    if (has_plane) {
        gm_map_primitive q;
        memset(&q, 0, sizeof(q));
        q.type = 1; q.inliers = r.plane_inliers;
        for (int k = 0; k < 4; ++k) q.params[k] = (float)r.plane_refit[k];
        memcpy(p, &q, sizeof(q)); p += sizeof(q);
    }
    if (has_cyl) {
        gm_map_primitive q;
        memset(&q, 0, sizeof(q));
        q.type = 2; q.inliers = r.cylinder_inliers;
        for (int k = 0; k < 7; ++k) q.params[k] = r.cylinder[k];
        if ((ctx->cfg.flags & GM_CFG_CYLINDER_FIT) && !(sl.last_fit.status & GM_FIT_FAILED_MASK)) {   // the fitted row
            q.inliers = sl.last_fit.inliers;
            for (int k = 0; k < 7; ++k) q.params[k] = sl.last_fit.model[k];
        }
        memcpy(p, &q, sizeof(q)); p += sizeof(q);
    }
    if (nvox) {
        GMX_HIP(ctx, hipMemcpyAsync(p, sl.vox4, (size_t)nvox * 16, hipMemcpyDeviceToHost, sl.stream));
        GMX_HIP(ctx, hipStreamSynchronize(sl.stream));
    }
    return GM_OK;
}

}  // extern "C"
