// k_surface.hip -- BUILD-DEFINED EXTENSION: wall deviation map against the fitted cylinder (GM_CFG_SURFACE_MAP).
//
// The semantics are stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/surface_np.py.  One streaming pass
// over the valid cloud with a scatter-reduce into n_stations x n_sectors cells.
//
// Shape: ONE launch per frame, kSurfThreads per block, one block per kSurfPointsPerBlock points of the frame's capacity
// (at most kSurfMaxBlocks): every block pays a fixed cost (zeroing its table, flushing the cells it touched), so a small
// frame runs on few blocks.  The cells do not depend on the grid (integer sums, min / max), so a frame, a replayed graph,
// another slot and the gm_surface_map stage call give the same bytes.
//   1. every thread derives the map frame from the fit row in fp64 (a few dozen flops, the same bits in every thread);
//   2. a block zeroes its private LDS table: sum i64 of rint(e 2^20), count u32, ~ordered(min e) u32, ordered(max e)
//      u32 -- 20 B per cell, GM_SURF_MAX_CELLS = 4096 cells = 80 KiB of static LDS (no scratch; 80 VGPRs, so one
//      1024-thread block per CU: 16 waves; -Rpass-analysis=kernel-resource-usage);
//   3. the point stream of gm_point_stream.hpp (stream_points): per point the class, e and the cell, coalesced stores of
//      e and the cell index, and LDS integer atomics.  A wave whose lanes hold runs of one cell (lidar frames: ring by azimuth, ~20 consecutive
//      points per 4-degree sector) first reduces each run into its head lane (segmented shuffles), so a run costs one
//      set of LDS atomics instead of ~20 on one address; a wave without such runs skips that step;
//   4. the block flushes its touched cells to the global table, lane <-> cell (contiguous), integer device atomics,
//      and adds its class counts;
//   5. the block that takes the last ticket converts the global table into gm_surface_cell records and the info block,
//      re-zeroes the table and the counters for the next launch (the table is zeroed at allocation), resets the ticket.
// No floating-point atomics and no host round trip: the model row is the device-side fit record and the point count
// the device word n_valid.
#include <math.h>
#include <string.h>

#include "gm_internal.hpp"
#include "gm_point_stream.hpp"

namespace gm {

constexpr int kSurfThreads = 1024;
constexpr uint32_t kSurfMaxBlocks = 256;          // one per CU
constexpr uint32_t kSurfPointsPerBlock = 16384;   // 16 points per thread before the grid grows
constexpr int kSurfUnroll = 2;   // points per thread and trip, loads issued together
constexpr int kSurfWaves = kSurfThreads / kWave;
constexpr uint32_t kSurfCells = GM_SURF_MAX_CELLS;
constexpr float kFix = 1048576.0f;   // 2^20: e * 2^20 is exact in fp32, |e| <= gate <= 8 keeps it below 2^24

// global table (bytes): sum i64 [cells] | count u32 [cells] | ~ordered(min) u32 [cells] | ordered(max) u32 [cells]
// | class counters u32 [4] (mapped, outside, beyond_gate, plane) | ticket u32 | pad
struct SurfTable {
    unsigned long long *sum;
    uint32_t *cnt, *lo, *hi, *ctr;
};
__device__ inline SurfTable surf_table(uint8_t *base)
{
    SurfTable t;
    t.sum = reinterpret_cast<unsigned long long *>(base);
    t.cnt = reinterpret_cast<uint32_t *>(base + 8 * (size_t)kSurfCells);
    t.lo = t.cnt + kSurfCells;
    t.hi = t.lo + kSurfCells;
    t.ctr = t.hi + kSurfCells;
    return t;
}
size_t surface_table_bytes() { return (size_t)kSurfCells * 20 + 32; }

struct SurfFrame {
    float o[3], a[3], u[3], v[3];
    float R;
    uint32_t status;   // GM_SURF_*
};

// The map frame of the include/gm_hip.h block: fp64 from the fp32 row, rounded to fp32 once.
__device__ inline SurfFrame surf_frame(const gm_cylinder_fit *fit, const SurfParams &p)
{
    SurfFrame f;
    double c[3], d[3];
    for (int k = 0; k < 3; ++k) { c[k] = fit->model[k]; d[k] = fit->model[3 + k]; }
    const double R = fit->model[6];
    const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const bool ok = !(fit->status & GM_FIT_FAILED_MASK) && isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) &&
                    isfinite(R) && isfinite(dn) && dn > 0.0;
    if (!ok) {
        const float nan = __builtin_nanf("");
        for (int k = 0; k < 3; ++k) f.o[k] = f.a[k] = f.u[k] = f.v[k] = nan;
        f.R = nan;
        f.status = GM_SURF_NO_MODEL;
        return f;
    }
    double a[3];
    const double s = d[0] * p.forward[0] + d[1] * p.forward[1] + d[2] * p.forward[2];
    for (int k = 0; k < 3; ++k) a[k] = (s >= 0.0 ? d[k] : -d[k]) / dn;
    const double ca = c[0] * a[0] + c[1] * a[1] + c[2] * a[2];
    const double ua = p.up[0] * a[0] + p.up[1] * a[1] + p.up[2] * a[2];
    double u[3];
    for (int k = 0; k < 3; ++k) u[k] = p.up[k] - ua * a[k];
    const double ul = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double upl = sqrt(p.up[0] * p.up[0] + p.up[1] * p.up[1] + p.up[2] * p.up[2]);
    f.status = GM_SURF_OK;
    if (ul < 0.1 * upl) {   // vertical shaft: `up` says nothing about the sectors
        double e2[3];
        fit_basis(a, u, e2);
        f.status |= GM_SURF_UP_FALLBACK;
    } else {
        for (int k = 0; k < 3; ++k) u[k] /= ul;
    }
    const double v[3] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]};
    for (int k = 0; k < 3; ++k) {
        f.o[k] = (float)(c[k] - ca * a[k]);
        f.a[k] = (float)a[k];
        f.u[k] = (float)u[k];
        f.v[k] = (float)v[k];
    }
    f.R = fit->model[6];
    return f;
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_map(SurfArgs a)
{
    __shared__ unsigned long long s_sum[kSurfCells];
    __shared__ uint32_t s_cnt[kSurfCells];
    __shared__ uint32_t s_lo[kSurfCells];   // ~ordered(min e): 0 = empty, atomicMax keeps the minimum
    __shared__ uint32_t s_hi[kSurfCells];   // ordered(max e): 0 = empty
    const SurfParams p = *a.prm;
    const SurfFrame F = surf_frame(a.fit, p);
    const bool model = F.status != GM_SURF_NO_MODEL;
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n_host;
    const uint32_t nsec = p.n_sectors, ncell = p.n_stations * p.n_sectors;   // <= kSurfCells (checked on the host)
    const float nst_f = (float)p.n_stations;
    const SurfTable T = surf_table(a.table);
    const int lane = lane_id();

    for (uint32_t c = threadIdx.x; c < ncell; c += kSurfThreads) { s_sum[c] = 0ull; s_cnt[c] = 0u; s_lo[c] = 0u; s_hi[c] = 0u; }
    __syncthreads();

    uint32_t cls[4] = {0u, 0u, 0u, 0u};   // mapped, outside, beyond_gate, plane
    stream_points<kSurfThreads, kSurfUnroll>(a.pts, a.labels, n, [&](uint64_t i, bool in, const float4 &q, uint32_t lab) {
        float e = __builtin_nanf("");
        int cell = -1;
        if (in && model) {
            if (lab == 1u) {
                ++cls[3];
            } else {
                float t, wx, wy, wz;
                e = surf_residual(q, F.o, F.a, F.R, t, wx, wy, wz);
                if (!(fabsf(e) <= p.gate)) {
                    ++cls[2];
                } else {
                    const float jf = surf_station(t, p.t_min, p.station_length);
                    if (!(jf >= 0.0f && jf < nst_f)) {
                        ++cls[1];
                    } else {
                        const uint32_t kk = surf_sector(wx, wy, wz, F.u, F.v, p.two_pi, p.sector_angle, nsec);
                        cell = (int)((uint32_t)jf * nsec + kk);
                        ++cls[0];
                    }
                }
            }
        }
        if (in) { a.res[i] = e; a.cell[i] = cell; }
        // the point's contribution: count, fixed-point sum, ~ordered(e), ordered(e) (all 0, neutral, unless mapped)
        uint32_t cn = 0u, lo = 0u, hi = 0u;
        unsigned long long sm = 0ull;
        if (cell >= 0) {
            cn = 1u;
            sm = (unsigned long long)(long long)__float2int_rn(__fmul_rn(e, kFix));
            hi = float_to_ordered(e);
            lo = ~hi;
        }
        if (surf_merge_runs(cell, cn, sm, lo, hi)) {
            atomicAdd(&s_cnt[cell], cn);
            atomicAdd(&s_sum[cell], sm);
            atomicMax(&s_lo[cell], lo);
            atomicMax(&s_hi[cell], hi);
        }
    });
    __syncthreads();
    // flush the touched cells, lane <-> cell, integer device atomics
    for (uint32_t c = threadIdx.x; c < ncell; c += kSurfThreads) {
        const uint32_t cn = s_cnt[c];
        if (!cn) continue;
        atomicAdd(&T.cnt[c], cn);
        atomicAdd(&T.sum[c], s_sum[c]);
        atomicMax(&T.lo[c], s_lo[c]);
        atomicMax(&T.hi[c], s_hi[c]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = wave_sum(cls[k]);
        if (lane == 0 && v) atomicAdd(&T.ctr[k], v);
    }
    __threadfence();
    __syncthreads();   // (every thread is past its reads of s_cnt: word 0 carries the ticket's verdict)
    if (threadIdx.x == 0) s_cnt[0] = atomicAdd(&T.ctr[4], 1u) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!s_cnt[0]) return;
    __threadfence();

    // last block: global table -> records, re-zeroed for the next launch
    uint32_t hit = 0u;
    for (uint32_t c = threadIdx.x; c < ncell; c += kSurfThreads) {
        const uint32_t cn = __hip_atomic_load(&T.cnt[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long sm = __hip_atomic_load(&T.sum[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t lo = __hip_atomic_load(&T.lo[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hi = __hip_atomic_load(&T.hi[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gm_surface_cell r;
        if (cn) {
            r.count = cn;
            r.mean = (float)(((double)(long long)sm * 0x1p-20) / (double)cn);
            r.min = ordered_to_float(~lo);
            r.max = ordered_to_float(hi);
            ++hit;
        } else {
            r.count = 0u;
            r.mean = r.min = r.max = __builtin_nanf("");
        }
        a.cells[c] = r;
        __hip_atomic_store(&T.cnt[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&T.sum[c], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&T.lo[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&T.hi[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    hit = wave_sum(hit);
    __syncthreads();   // (every thread has read word 0)
    if (lane == 0) s_cnt[threadIdx.x / kWave] = hit;
    __syncthreads();
    if (threadIdx.x != 0) return;
    gm_surface_info info;
    info.struct_size = (uint32_t)sizeof(gm_surface_info);
    info.status = F.status;
    info.n_stations = p.n_stations;
    info.n_sectors = p.n_sectors;
    info.mapped = atomicExch(&T.ctr[0], 0u);
    info.outside = atomicExch(&T.ctr[1], 0u);
    info.beyond_gate = atomicExch(&T.ctr[2], 0u);
    info.plane = atomicExch(&T.ctr[3], 0u);
    uint32_t cells_hit = 0u;
    for (int w = 0; w < kSurfWaves; ++w) cells_hit += s_cnt[w];
    info.cells_hit = cells_hit;
    info.reserved = 0u;
    for (int k = 0; k < 3; ++k) { info.o[k] = F.o[k]; info.a[k] = F.a[k]; info.u[k] = F.u[k]; info.v[k] = F.v[k]; }
    info.R = F.R;
    info.t_min = p.t_min;
    info.station_length = p.station_length;
    info.sector_angle = p.sector_angle;
    *a.info = info;
    atomicExch(&T.ctr[4], 0u);   // ready for the next launch
}

uint32_t surface_blocks(uint32_t n_cap)
{
    const uint32_t b = (uint32_t)(((uint64_t)n_cap + kSurfPointsPerBlock - 1) / kSurfPointsPerBlock);
    return b < 1u ? 1u : (b > kSurfMaxBlocks ? kSurfMaxBlocks : b);
}

void launch_surface_map(const SurfArgs &a, uint32_t n_cap, hipStream_t s)
{
    hipLaunchKernelGGL(k_surface_map, dim3(surface_blocks(n_cap)), dim3(kSurfThreads), 0, s, a);
}

SurfParams surface_device_params(const gm_surface_params &q)
{
    SurfParams p;
    memset(&p, 0, sizeof(p));
    const double two_pi = 6.283185307179586476925286766559;
    p.n_stations = q.n_stations;
    p.n_sectors = q.n_sectors;
    p.station_length = (float)q.station_length;
    p.t_min = (float)q.t_min;
    p.gate = (float)q.gate;
    p.sector_angle = (float)(two_pi / (double)q.n_sectors);
    p.two_pi = (float)two_pi;
    for (int k = 0; k < 3; ++k) { p.up[k] = q.up[k]; p.forward[k] = q.forward[k]; }
    return p;
}

// the limits of include/gm_hip.h (the fp32 binning constants must be finite too)
gm_status gm_check_surface_params(const gm_surface_params *p)
{
    if (!p || p->struct_size != sizeof(gm_surface_params)) return GM_ERR_INVALID_ARG;
    if (p->n_stations < 1u || p->n_sectors < 1u || (uint64_t)p->n_stations * p->n_sectors > GM_SURF_MAX_CELLS)
        return GM_ERR_INVALID_ARG;
    if (!(p->station_length > 0.0) || !isfinite(p->station_length) || !((float)p->station_length > 0.0f) ||
        !isfinite(p->t_min) || !isfinite((float)p->t_min) || !(p->gate > 0.0) || !(p->gate <= 8.0))
        return GM_ERR_INVALID_ARG;
    double up2 = 0.0, fw2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(p->up[k]) || !isfinite(p->forward[k])) return GM_ERR_INVALID_ARG;
        up2 += p->up[k] * p->up[k];
        fw2 += p->forward[k] * p->forward[k];
    }
    if (!(up2 > 0.0) || !(fw2 > 0.0) || !isfinite(up2) || !isfinite(fw2)) return GM_ERR_INVALID_ARG;
    return GM_OK;
}

}  // namespace gm
