// gm_group_cut.hpp -- the host side of a group's slab cut (gm_group.hip, DESIGN.md par. 6).  No device and no HIP: the
// C ABI's structs and the standard library only, so that the threaded passes run on a CPU under sanitizers
// (host/gm_group_cut_test.cpp).  cut_plan, the caller's allocation of the ranks' row buffers, then cut_scatter: both on T
// threads (cut_threads is the library's policy), the same bytes out for every T.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <thread>
#include <vector>

#include "../../include/gm_hip.h"

namespace gm {

inline float load_f32(const uint8_t *p, bool bswap)
{
    uint32_t u;
    memcpy(&u, p, 4);
    if (bswap) u = __builtin_bswap32(u);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// fn(t) for t in [0, T) on T threads (the caller's included)
template <class F>
void parallel_for(uint32_t T, F fn)
{
    if (T <= 1) { fn(0u); return; }
    std::vector<std::thread> th;
    th.reserve(T - 1);
    for (uint32_t t = 1; t < T; ++t) th.emplace_back([&fn, t]() { fn(t); });
    fn(0u);
    for (auto &x : th) x.join();
}

// pcl::VoxelGrid's lattice index of a coordinate, as every kernel computes it (k_normals.hip voxel_sums, k_voxel.hip)
inline long long lattice_cell(float x, float inv_leaf) { return (long long)floorf(x * inv_leaf); }

// smallest float t with lattice_cell(t) >= k: the plane between cells k-1 and k in float space (the map is monotone)
inline float lattice_plane(long long k, float inv_leaf)
{
    float t = (float)((double)k / (double)inv_leaf);
    for (int it = 0; it < 64 && lattice_cell(t, inv_leaf) >= k; ++it) t = nextafterf(t, -std::numeric_limits<float>::infinity());
    for (int it = 0; it < 128 && lattice_cell(t, inv_leaf) < k; ++it) t = nextafterf(t, std::numeric_limits<float>::infinity());
    return t;
}

// threads of the cut of an n-row frame: the machine's, GM_GROUP_THREADS instead when set, 16 at most, one below 262144 rows
inline uint32_t cut_threads(uint32_t n)
{
    uint32_t T = std::thread::hardware_concurrency();
    if (const char *e = getenv("GM_GROUP_THREADS")) T = (uint32_t)atoi(e);
    if (T > 16) T = 16;
    if (T < 1 || n < 262144u) T = 1;
    return T;
}

struct CutPlan {
    std::vector<double> edges;   // [R + 1], edges[0] = -inf, edges[R] = +inf
    double halo = 0.0;
    bool on_lattice = false;     // every inner edge is a plane of the voxel lattice
    uint32_t n_inside = 0;       // rows inside the box
    std::vector<uint32_t> total;               // [R] rows sent to each rank
    std::vector<std::vector<uint32_t>> off;    // [T][R] where thread t's rows start in rank r's buffers
};

// membership: rank r takes the rows with x in [edge[r] - halo, edge[r+1] + halo)   (NaN rows fail both comparisons:
// every rank's crop would drop them anyway)
inline bool cut_takes(const CutPlan &plan, uint32_t r, double x) { return x >= plan.edges[r] - plan.halo && x < plan.edges[r + 1] + plan.halo; }

// the first of thread t's rows when T threads share n (thread T's: n)
inline uint32_t cut_first(uint32_t n, uint32_t t, uint32_t T) { return (uint32_t)((uint64_t)n * t / T); }

// The plan for the host rows of `cloud` and R ranks, on T >= 1 threads.  xs: scratch, the x of every row on return.
inline void cut_plan(const gm_config &cfg, uint32_t R, const gm_cloud &cloud, uint32_t T, std::vector<float> &xs, CutPlan &plan)
{
    const uint32_t n = cloud.n_points;
    const uint64_t step = cloud.point_step;
    const bool bswap = (cloud.flags & GM_CLOUD_BIGENDIAN) != 0;
    const uint8_t *base = (const uint8_t *)cloud.data;
    const float lo = (float)(-cfg.boxFilterBound), hi = (float)cfg.boxFilterBound;
    const float inv_leaf = 1.0f / (float)cfg.voxelGridLeafSize;
    // histogram bins: lattice cells of the box along x (several cells per bin when the lattice is very fine); when the
    // lattice is too coarse to balance the ranks, 4096 uniform bins instead (a voxel may then straddle an edge: the
    // dense tables of the ranks are merged exactly, see merge_voxels of gm_group.hip)
    const long long c_lo = lattice_cell(lo, inv_leaf), ncell = lattice_cell(hi, inv_leaf) - c_lo + 1;
    plan.on_lattice = (cfg.flags & GM_CFG_VOXEL_GRID) != 0 && ncell >= (long long)4 * R;
    int shift = 0;
    while (plan.on_lattice && (ncell >> shift) > (1ll << 20)) ++shift;
    const uint32_t nbins = plan.on_lattice ? (uint32_t)((ncell + (1ll << shift) - 1) >> shift) : 4096u;
    const double ubin = (double)nbins / ((double)hi - (double)lo > 0 ? (double)hi - (double)lo : 1.0);
    xs.resize(n);
    std::vector<std::vector<uint32_t>> hist(T, std::vector<uint32_t>(nbins, 0u));
    std::vector<uint32_t> inside(T, 0u);
    parallel_for(T, [&](uint32_t t) {
        const uint32_t i0 = cut_first(n, t, T), i1 = cut_first(n, t + 1, T);
        std::vector<uint32_t> &h = hist[t];
        uint32_t in = 0;
        for (uint32_t i = i0; i < i1; ++i) {
            const uint8_t *row = base + (size_t)i * step;
            const float x = load_f32(row + cloud.off_x, bswap), y = load_f32(row + cloud.off_y, bswap), z = load_f32(row + cloud.off_z, bswap);
            xs[i] = x;
            if (std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && !(x < lo || y < lo || z < lo || x > hi || y > hi || z > hi)) {
                uint32_t b;
                if (plan.on_lattice) b = (uint32_t)((lattice_cell(x, inv_leaf) - c_lo) >> shift);
                else { const double u = ((double)x - (double)lo) * ubin; b = u < 0 ? 0u : (uint32_t)u; }
                ++h[b < nbins ? b : nbins - 1];
                ++in;
            }
        }
        inside[t] = in;
    });
    uint64_t n_in = 0;
    for (uint32_t t = 0; t < T; ++t) n_in += inside[t];
    plan.n_inside = (uint32_t)n_in;
    // edges: the bin boundary at which the running count first reaches g / R of the in-box rows
    plan.edges.assign(R + 1, 0.0);
    plan.edges[0] = -std::numeric_limits<double>::infinity();
    plan.edges[R] = std::numeric_limits<double>::infinity();
    uint64_t run = 0;
    uint32_t g = 1;
    for (uint32_t b = 0; b < nbins && g < R; ++b) {
        uint64_t c = 0;
        for (uint32_t t = 0; t < T; ++t) c += hist[t][b];
        run += c;
        while (g < R && run * R >= n_in * (uint64_t)g && n_in) {   // the edge behind bin b
            if (plan.on_lattice) plan.edges[g] = (double)lattice_plane(c_lo + ((long long)(b + 1) << shift), inv_leaf);
            else plan.edges[g] = (double)(float)((double)lo + (double)(b + 1) / ubin);
            ++g;
        }
    }
    for (; g < R; ++g) plan.edges[g] = n_in ? plan.edges[g - 1] : 0.0;   // (an empty frame: every edge at 0)
    for (uint32_t k = 1; k < R; ++k) if (plan.edges[k] < plan.edges[k - 1]) plan.edges[k] = plan.edges[k - 1];
    plan.halo = 1.01 * cfg.neighborRadius;
    std::vector<std::vector<uint32_t>> cnt(T, std::vector<uint32_t>(R, 0u));
    parallel_for(T, [&](uint32_t t) {
        const uint32_t i0 = cut_first(n, t, T), i1 = cut_first(n, t + 1, T);
        std::vector<uint32_t> &c = cnt[t];
        for (uint32_t i = i0; i < i1; ++i) {
            const double x = (double)xs[i];
            for (uint32_t r = 0; r < R; ++r) c[r] += cut_takes(plan, r, x) ? 1u : 0u;
        }
    });
    plan.total.assign(R, 0u);
    plan.off.assign(T, std::vector<uint32_t>(R, 0u));
    for (uint32_t r = 0; r < R; ++r)
        for (uint32_t t = 0; t < T; ++t) { plan.off[t][r] = plan.total[r]; plan.total[r] += cnt[t][r]; }
}

// With the T and xs of the plan: rank r's rows, point_step bytes each, into rows[r] (plan.total[r] of them) and the input
// row of each into ids[r], both in ascending input row.
inline void cut_scatter(const gm_cloud &cloud, uint32_t T, const std::vector<float> &xs, const CutPlan &plan, uint8_t *const *rows,
                        uint32_t *const *ids)
{
    const uint32_t n = cloud.n_points, R = (uint32_t)plan.total.size();
    const uint64_t step = cloud.point_step;
    const uint8_t *base = (const uint8_t *)cloud.data;
    parallel_for(T, [&](uint32_t t) {
        const uint32_t i0 = cut_first(n, t, T), i1 = cut_first(n, t + 1, T);
        std::vector<uint32_t> at(plan.off[t]);
        for (uint32_t i = i0; i < i1; ++i) {
            const double x = (double)xs[i];
            for (uint32_t r = 0; r < R; ++r)
                if (cut_takes(plan, r, x)) {
                    memcpy(rows[r] + (size_t)at[r] * step, base + (size_t)i * step, step);
                    ids[r][at[r]] = i;
                    ++at[r];
                }
        }
    });
}

}  // namespace gm
