// gm_device.hpp -- device-side helpers shared by the gfx950 kernels.
// Wave = 64 lanes everywhere (CDNA4); nothing here is written for 32-wide warps.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gm_hip.h"

namespace gm {

constexpr int kWave = 64;

// Per-frame device counters.  Zeroed by one hipMemsetAsync at the head of a
// frame; every data-dependent size of the pipeline lives here so that no stage
// needs a host round-trip.
// state of one chained-scan launch (gm_compact.hpp)
struct ScanState {
    unsigned long long *status;  // [>= grid size] tile records
    uint32_t *ticket;            // 0 between launches
    uint32_t epoch;              // 1 .. 2^30-1, different from the previous launches' on this array
    const uint32_t *frame_ptr;   // graph replay (kernel arguments are frozen): epoch = f(*frame_ptr, epoch), see scan_epoch()
};

// Epoch of a chained-scan launch.  Launches enqueued one by one take it from the host (a per-slot counter, range
// [1, 2^29)); launches replayed from a captured graph cannot -- their arguments are frozen -- and derive it from the
// slot's device-side frame counter (bumped by the frame's opening kernel) and the launch's index in the frame, range
// [2^29, 2^30): the two ranges never meet, so records of the one kind are never taken for records of the other.
__device__ __forceinline__ uint32_t scan_epoch(const ScanState &st)
{
    return st.frame_ptr ? 0x20000000u + (((*st.frame_ptr) * 32u + st.epoch) & 0x1FFFFFFFu) : st.epoch;
}

#ifndef GM_TILE_CLASSES
#define GM_TILE_CLASSES 8
#endif
constexpr int kTileListClasses = GM_TILE_CLASSES;   // cost classes of k_normals' tile list (k_normals.hip)

struct DevCounters {
    uint32_t n_cropped;   // points surviving the crop box
    uint32_t n_valid;     // points with a finite normal (and owned, when sharded)
    uint32_t n_tiles;     // (unused since the tile list has cost classes: n_tiles_c below)
    uint32_t first_drop_enc;   // 0xFFFFFFFF - (first cropped index without a finite normal); 0 = none (NaN-normal compaction)
    uint32_t n_voxels;    // occupied voxels
    uint32_t vox_n;       // points entering the voxel grid (= n_valid)
    uint32_t mm[6];       // ordered-uint encodings: min x,y,z then max x,y,z of the valid cloud
    uint32_t scratch_total;
    uint32_t pad[5];      // (diagnostic builds count candidate streams here)
    // tiles per cost class (k_rows_and_tiles files a tile by its x extent; k_normals runs class 0 first), one counter per
    // 128-byte line: every cutter block adds to every class, and returning atomics on one line are served one after the
    // other (~88 per us) -- eight counters in one line cost the tile builder 4.5 us
    uint32_t n_tiles_c[kTileListClasses][32];
};
static_assert(sizeof(DevCounters) % 8 == 0, "zero-filled in 8-byte words");

// Voxel-grid parameters derived on the device from the min/max of the cloud
// (pcl::VoxelGrid::applyFilter: min_b_, div_b_, divb_mul_).
struct VoxelParams {
    float inv_leaf;
    int32_t min_b[3];
    int32_t div_b[3];
    int32_t mul1, mul2;
    uint32_t passthrough;
};

// Uniform cell grid used for the fixed-radius search (stands in for the FLANN
// kd-tree of src/tunnel_processing.cpp:62-63: same neighbour sets).
struct GridParams {
    float ox, oy, oz;   // origin (lower corner)
    float inv_h;        // 1 / cell edge in y and z, edge >= 1.001 * radius
    float inv_hx;       // 1 / cell edge in x = fine * inv_h: x is binned `fine` times finer, so that
                        // the points of one x-row are sorted by x and candidate ranges can be cut to
                        // [xmin - r, xmax + r] of a tile instead of whole cells
    int32_t nx, ny, nz; // cells per axis (nx counts the fine x cells)
    int32_t xreach;     // fine x cells that cover the radius (fine + 1)
    float r2;           // (float)(radius*radius): KdTreeFLANN::radiusSearch's cast
    float r2_scale;     // power of two s with r2 * s ~ 2^100: k_normals evaluates d2 < r2 as clamp01(fma(d2, -s, r2 * s)),
                        // exact because one ulp of a d2 next to r2, times s, is >= 2^76
    float snap;         // power of two >= one ulp of the largest coordinate of the grid box: tile origins of the
                        // matrix-core kernel are multiples of it, which makes point - origin exact up to the rounding of a
                        // radius-sized number
    int32_t D;          // y/z rows per radius (1 .. 4): the cells are 1.001 r / D wide in y and z, a tile's candidates lie
                        // in the (2D+1)^2 rows around its own.  D > 1 pays when a tile is short against the radius (many
                        // neighbours per point): the far rows need a shorter x-window, sqrt(r^2 - gap_y^2 - gap_z^2).
    int16_t reach[5][5];// [|row offset y|][|row offset z|]: fine x cells that cover that window half-width; 0 = no row
    float dscale;       // power of two >= 1 / band: the distance MFMA of k_normals computes T = (r2 - d2) * dscale, so that
                        // one v_cvt_pk_bf16_f32 with clamp turns two of them into two 0/1 weights (every T in (0, 1) lies
                        // inside the band and is re-evaluated exactly)
    float dband;        // band * dscale, in [1, 2)
    float band;         // half-width of the band around r2 inside which the distance MFMA's value does not decide a pair
                        // (2e-5 * (1.001 r)^2, whatever D is: analytic worst case of the distance product 1.7e-5 of that
                        // square, largest error measured by the diagnostic build over every tested pair of the 1 M-point frame
                        // 4.2e-6 -- profiles/r02_distance_mfma_error.json, tools/microbench/mfma_probe.hip)
};

// Dense voxel table (fast path of the VoxelGrid stage): when the crop box bounds
// the voxel lattice to a small table, per-voxel sums are accumulated as exact
// 64-bit fixed-point integers (order-free, so bit-reproducible) right where the
// normals are produced, and the sorted output is a compaction of the table.
struct VoxCell {
    unsigned long long sx, sy, sz;  // sum of (coord - lo) * scale, rounded to integer per point
    uint32_t cnt, pad;
};
struct VoxDense {
    uint32_t enabled;
    int32_t i_lo;        // floor(lo * inv_leaf): lattice index of the box's lower face
    int32_t dim;         // lattice cells per axis covered by the box
    float inv_leaf;      // 1 / (float)leaf, as pcl::VoxelGrid computes it
    float lo;            // lower face of the crop box
    float own_lo, own_hi;// slab ownership (multi-GPU), +-inf otherwise
    double scale, inv_scale;
    uint32_t xcd_chunk;  // k_normals launch option riding along: blocks per XCD chunk of the tile mapping (0 = round-robin)
    uint32_t pad_;
};

// extension outputs (RANSAC plane / cylinder; no reference counterpart)
struct FrameExt {
    float plane[4];
    float cylinder[7];
    uint32_t plane_inliers, cylinder_inliers;
    uint32_t pad;
    double plane_refit[4];
    double cyl_axis_refit[3];
};

// e1, e2 perpendicular to the unit d (the basis synth._basis builds): e1 = (h x d) / |h x d|, e2 = d x e1.  The cylinder
// regression's Jacobian frame (k_cylfit.hip) and the surface map's fallback sector direction (k_surface.hip).
__host__ __device__ inline void fit_basis(const double d[3], double e1[3], double e2[3])
{
    const double h[3] = {0.0, fabs(d[2]) < 0.9 ? 0.0 : 1.0, fabs(d[2]) < 0.9 ? 1.0 : 0.0};
    double u[3] = {h[1] * d[2] - h[2] * d[1], h[2] * d[0] - h[0] * d[2], h[0] * d[1] - h[1] * d[0]};
    const double inv = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int k = 0; k < 3; ++k) e1[k] = u[k] * inv;
    e2[0] = d[1] * e1[2] - d[2] * e1[1];
    e2[1] = d[2] * e1[0] - d[0] * e1[2];
    e2[2] = d[0] * e1[1] - d[1] * e1[0];
}

// surface map parameters as the map kernel reads them from the device (k_surface.hip): the fp32 binning constants are
// rounded once on the host from gm_surface_params, so a captured graph picks up gm_set_surface_params
struct SurfParams {
    uint32_t n_stations, n_sectors;
    float station_length, t_min, gate, sector_angle, two_pi;
    uint32_t pad;
    double up[3], forward[3];
};

// working model of the cylinder regression between its launches (k_cylfit.hip): the current (c, d, r), the hypothesis
// direction (axis sign), status and the size of the last Gauss-Newton step
struct CylFitWork {
    double c[3], d[3], r;
    double d_hyp[3];
    double last_step;
    uint32_t status, passes;
};

struct FrameOut {        // device -> host result record (one small D2H per frame)
    DevCounters ctr;
    float evals[3];
    float evecs[9];      // column-major
    double scatter[6];
    VoxelParams vox;
    FrameExt ext;
    gm_cylinder_fit fit; // GM_CFG_CYLINDER_FIT (k_cylfit.hip); untouched otherwise
};

// ---- wave-level primitives ---------------------------------------------------

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

__device__ __forceinline__ uint64_t lanemask_lt()
{
    return (1ull << lane_id()) - 1ull;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, kWave));
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// inclusive scan of one value per lane across the wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        uint32_t t = __shfl_up(v, o, kWave);
        if (lane_id() >= o) v += t;
    }
    return v;
}

// LDS traffic of ONE wave is issued and serviced in order; this only stops the
// compiler from moving accesses across the point.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// total order on floats as unsigned ints (for atomicMin/atomicMax)
__device__ __forceinline__ uint32_t float_to_ordered(float f)
{
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ordered_to_float(uint32_t o)
{
    uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}

// ---- the per-point chain of the wall maps (include/gm_hip.h states it): k_surface.hip bins against the frame's fitted
// cylinder, k_wall.hip against the design cylinder seen from the frame.  fp32 with explicit roundings, so both kernels,
// every grid and every launch site give the same bits.
__device__ __forceinline__ float surf_dot3(float x, float y, float z, const float (&b)[3])
{
    return __fmaf_rn(x, b[0], __fmaf_rn(y, b[1], __fmul_rn(z, b[2])));
}
// q = p - o, t = q.a, w = q - t a; returns rho = |w|
__device__ __forceinline__ float surf_rho(const float4 &p, const float (&o)[3], const float (&a)[3], float &t, float &wx, float &wy,
                                          float &wz)
{
    const float qx = __fsub_rn(p.x, o[0]), qy = __fsub_rn(p.y, o[1]), qz = __fsub_rn(p.z, o[2]);
    t = surf_dot3(qx, qy, qz, a);
    wx = __fmaf_rn(-t, a[0], qx); wy = __fmaf_rn(-t, a[1], qy); wz = __fmaf_rn(-t, a[2], qz);
    return __fsqrt_rn(__fmaf_rn(wx, wx, __fmaf_rn(wy, wy, __fmul_rn(wz, wz))));
}
// the same, returning e = |w| - R
__device__ __forceinline__ float surf_residual(const float4 &p, const float (&o)[3], const float (&a)[3], float R, float &t,
                                               float &wx, float &wy, float &wz)
{
    return __fsub_rn(surf_rho(p, o, a, t, wx, wy, wz), R);
}
// floor((t - t_min) / ds), still a float: the caller checks the range before it converts
__device__ __forceinline__ float surf_station(float t, float t_min, float ds)
{
    return floorf(__fdiv_rn(__fsub_rn(t, t_min), ds));
}
// k = min(floor(phi / dtheta), n_sectors - 1), phi = atan2(w.v, w.u) folded to [0, 2 pi)
__device__ __forceinline__ uint32_t surf_sector(float wx, float wy, float wz, const float (&u)[3], const float (&v)[3],
                                                float two_pi, float sector_angle, uint32_t nsec)
{
    const float th = atan2f(surf_dot3(wx, wy, wz, v), surf_dot3(wx, wy, wz, u));
    const float phi = th < 0.0f ? __fadd_rn(th, two_pi) : th;
    const uint32_t kk = (uint32_t)floorf(__fdiv_rn(phi, sector_angle));
    return kk < nsec - 1u ? kk : nsec - 1u;
}
// sqrt rounded to nearest, as the curved chains' rule has every operation.  (__fsqrt_rn is not that here: without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers make it the bare v_sqrt_f32, which is good to an ulp and moved e by one on
// a tenth of an arc frame's points against the rule's twin, tests/test_gpu_wall_curved_chain.py.  The builtin is the
// compiler's correctly rounded expansion, v_sqrt_f32 and one fma test of each neighbour, which hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt keeps on.)
__device__ __forceinline__ float sqrt_rn(float x)
{
    return __builtin_sqrtf(x);
}
// ---- the same chain on a circular-arc design axis (include/gm_hip.h states it; k_wall.hip's and k_wall_check.hip's arc
// instantiations).  (o, a, n, b): the section at the anchor station in sensor coordinates.  Returns e; t: the arc length
// from the anchor section, (yc, z): the offset in the point's own section along n(s) and b; cy <= 0: a quarter turn or more
// from the anchor section (the caller classes it beyond_gate).
// The chain itself also hands out rho = e + R before the subtraction and (cs, sn) = (cy, cx) / d, the cosine and sine of
// the turn psi from the anchor section to the point's own (the alignment's locate builds the radial direction from them);
// arc_residual is the chain for the callers that bin.
__device__ __forceinline__ float arc_chain(const float4 &p, const float (&o)[3], const float (&a)[3], const float (&n)[3],
                                           const float (&b)[3], float kappa, float R, float &t, float &yc, float &z, float &cy,
                                           float &rho, float &cs, float &sn)
{
    const float qx = __fsub_rn(p.x, o[0]), qy = __fsub_rn(p.y, o[1]), qz = __fsub_rn(p.z, o[2]);
    const float x = surf_dot3(qx, qy, qz, a), y = surf_dot3(qx, qy, qz, n);
    z = surf_dot3(qx, qy, qz, b);
    const float cx = __fmul_rn(kappa, x);
    cy = __fmaf_rn(-kappa, y, 1.0f);
    const float d = sqrt_rn(__fmaf_rn(cx, cx, __fmul_rn(cy, cy)));
    t = __fdiv_rn(atan2f(cx, cy), kappa);
    const float h = __fmaf_rn(x, x, __fmul_rn(y, y));
    yc = __fdiv_rn(__fmaf_rn(-kappa, h, __fadd_rn(y, y)), __fadd_rn(1.0f, d));
    cs = __fdiv_rn(cy, d);
    sn = __fdiv_rn(cx, d);
    rho = sqrt_rn(__fmaf_rn(yc, yc, __fmul_rn(z, z)));
    return __fsub_rn(rho, R);
}
__device__ __forceinline__ float arc_residual(const float4 &p, const float (&o)[3], const float (&a)[3], const float (&n)[3],
                                              const float (&b)[3], float kappa, float R, float &t, float &yc, float &z, float &cy)
{
    float rho, cs, sn;
    return arc_chain(p, o, a, n, b, kappa, R, t, yc, z, cy, rho, cs, sn);
}
// surf_sector on (yc, z): phi = atan2(yc vn + z vb, yc un + z ub)
__device__ __forceinline__ uint32_t arc_sector(float yc, float z, float un, float ub, float vn, float vb, float two_pi,
                                               float sector_angle, uint32_t nsec)
{
    const float th = atan2f(__fmaf_rn(yc, vn, __fmul_rn(z, vb)), __fmaf_rn(yc, un, __fmul_rn(z, ub)));
    const float phi = th < 0.0f ? __fadd_rn(th, two_pi) : th;
    const uint32_t kk = (uint32_t)floorf(__fdiv_rn(phi, sector_angle));
    return kk < nsec - 1u ? kk : nsec - 1u;
}
// A map on a circular-arc design axis (gm_wall_map_create_arc): what the arc instantiations take by value beside WallArgs
// (gm_internal.hpp), whose o, a are then o', a' at the anchor section (u, v are reported, not read).
struct WallArc {
    float n[3], b[3];          // n', b' in sensor coordinates
    float kappa, un, ub, vn, vb;
};
// A map on a clothoid design axis (gm_wall_map_create_clothoid): the arc block, whose kappa is then kappa_f at the anchor
// section, plus the curvature's rate.
struct WallClothoid {
    WallArc arc;
    float rate;
};
// The design axis a chain is instantiated for, and the axis as a kernel argument: nothing on a straight map.  (The
// straight and the arc arguments are the two WallArcArg the kernels have always taken; the clothoid's is a type of its own.)
enum : int { kAxisStraight = 0, kAxisArc = 1, kAxisClothoid = 2 };
template <bool kArc>
struct WallArcArg { static constexpr int kAxis = kAxisStraight; };
template <>
struct WallArcArg<true> {
    static constexpr int kAxis = kAxisArc;
    WallArc arc;
};
struct WallClothoidArg {
    static constexpr int kAxis = kAxisClothoid;
    WallClothoid cl;
};

// ---- the same chain on a clothoid design axis (include/gm_hip.h states it).  (o, a, n, b): the section at the anchor
// station in sensor coordinates, kappa there, rate along the chainage.  The foot of the perpendicular by a start on the
// osculating arc (on the tangent where |kappa| < 1e-6: a uniform branch) and GM_WALL_CLOTHOID_STEPS Newton steps, a fixed
// count, so every grid and launch site gives the same bits.  Returns e; t: the arc length from the anchor section,
// (yc, z): the offset in the point's own section; ok <= 0: the point is beyond_gate whatever e says (the start a quarter
// turn away, a Newton denominator <= 0.25, a t that is not finite, a final |g| above GM_WALL_CLOTHOID_G_BOUND).
// (sin, cos) of the header's sincos rule: a three-term reduction by pi / 2 and the two Cephes single-precision polynomials
// on [-pi / 4, pi / 4], every operation rounded to nearest.  Fifteen of them per point: the library's sinf / cosf, each
// with its large-argument reduction inlined, made the unrolled point loops too long to unroll and their per-item arrays
// private memory.  An angle of 2^20 or more, or a NaN, gives NaN without an integer conversion (such a point is then
// classed by its g).
__device__ __forceinline__ void clothoid_sincos(float ps, float &sn, float &cs)
{
    const bool fin = fabsf(ps) < 1048576.0f;
    const float k = fin ? rintf(__fmul_rn(ps, 0.63661977236758134f)) : 0.0f;
    float r = __fmaf_rn(-k, 1.5703125f, ps);
    r = __fmaf_rn(-k, 4.837512969970703125e-4f, r);
    r = __fmaf_rn(-k, 7.54978995489188216e-8f, r);
    const float z = __fmul_rn(r, r);
    float ps_ = __fmaf_rn(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps_ = __fmaf_rn(ps_, z, -1.6666654611e-1f);
    const float s = __fmaf_rn(__fmul_rn(ps_, z), r, r);
    float pc = __fmaf_rn(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = __fmaf_rn(pc, z, 4.166664568298827e-2f);
    const float c = __fadd_rn(__fmaf_rn(__fmul_rn(pc, z), z, __fmul_rn(-0.5f, z)), 1.0f);
    const int q = (int)k & 3;
    const float s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    const float nan = __builtin_nanf("");
    sn = fin ? ((q & 2) ? -s1 : s1) : nan;
    cs = fin ? (((q + 1) & 2) ? -c1 : c1) : nan;
}
// node i of the 4-node Gauss-Legendre rule on [0, 1]: (c_i, w_i) = (c, w)
template <bool kFirst>
__device__ __forceinline__ void clothoid_node(float kappa, float hr, float t, float c, float w, float &sx, float &sy)
{
    const float sg = __fmul_rn(t, c);
    const float ps = __fmul_rn(__fmaf_rn(hr, sg, kappa), sg);
    float sn, cs;
    clothoid_sincos(ps, sn, cs);
    sx = kFirst ? __fmul_rn(w, cs) : __fmaf_rn(cs, w, sx);
    sy = kFirst ? __fmul_rn(w, sn) : __fmaf_rn(sn, w, sy);
}
// E(t) of the header: g and yc of the trial t
// (sn, cs): the sine and cosine of ps = psi(t), the turn from the anchor section to the section at t
__device__ __forceinline__ void clothoid_eval(float x, float y, float kappa, float hr, float t, float &g, float &yc, float &sn, float &cs)
{
    float sx, sy;
    clothoid_node<true>(kappa, hr, t, 0.06943184420297371f, 0.17392742256872692f, sx, sy);
    clothoid_node<false>(kappa, hr, t, 0.33000947820757187f, 0.32607257743127305f, sx, sy);
    clothoid_node<false>(kappa, hr, t, 0.6699905217924281f, 0.32607257743127305f, sx, sy);
    clothoid_node<false>(kappa, hr, t, 0.9305681557970262f, 0.17392742256872692f, sx, sy);
    const float dx = __fsub_rn(x, __fmul_rn(t, sx)), dy = __fsub_rn(y, __fmul_rn(t, sy));
    const float ps = __fmul_rn(__fmaf_rn(hr, t, kappa), t);
    clothoid_sincos(ps, sn, cs);
    g = __fmaf_rn(dx, cs, __fmul_rn(dy, sn));
    yc = __fmaf_rn(dy, cs, -__fmul_rn(dx, sn));
}
// The chain; as arc_chain it also hands out rho and the (cs, sn) of the closing evaluation.  clothoid_residual is the chain
// for the callers that bin.
__device__ __forceinline__ float clothoid_chain(const float4 &p, const float (&o)[3], const float (&a)[3], const float (&n)[3],
                                                const float (&b)[3], float kappa, float rate, float R, float &t, float &yc,
                                                float &z, float &ok, float &rho, float &cs, float &sn)
{
    const float qx = __fsub_rn(p.x, o[0]), qy = __fsub_rn(p.y, o[1]), qz = __fsub_rn(p.z, o[2]);
    const float x = surf_dot3(qx, qy, qz, a), y = surf_dot3(qx, qy, qz, n);
    z = surf_dot3(qx, qy, qz, b);
    const float cy = __fmaf_rn(-kappa, y, 1.0f);
    t = fabsf(kappa) < 1.0e-6f ? x : __fdiv_rn(atan2f(__fmul_rn(kappa, x), cy), kappa);
    const float hr = __fmul_rn(0.5f, rate);
    bool good = cy > 0.0f;
    float g;
#pragma unroll
    for (int it = 0; it < GM_WALL_CLOTHOID_STEPS; ++it) {
        clothoid_eval(x, y, kappa, hr, t, g, yc, sn, cs);
        const float den = __fmaf_rn(-__fmaf_rn(t, rate, kappa), yc, 1.0f);
        good = good && den > 0.25f;
        t = __fadd_rn(t, __fdiv_rn(g, den));
    }
    clothoid_eval(x, y, kappa, hr, t, g, yc, sn, cs);
    good = good && fabsf(t) < __builtin_inff() && fabsf(g) <= GM_WALL_CLOTHOID_G_BOUND;
    ok = good ? 1.0f : 0.0f;
    rho = sqrt_rn(__fmaf_rn(yc, yc, __fmul_rn(z, z)));
    return __fsub_rn(rho, R);
}
__device__ __forceinline__ float clothoid_residual(const float4 &p, const float (&o)[3], const float (&a)[3], const float (&n)[3],
                                                   const float (&b)[3], float kappa, float rate, float R, float &t, float &yc,
                                                   float &z, float &ok)
{
    float rho, cs, sn;
    return clothoid_chain(p, o, a, n, b, kappa, rate, R, t, yc, z, ok, rho, cs, sn);
}

// ---- the head of the chain against a map (k_wall_add*, the check's predicate, k_wall_align_bin): label, residual, gate,
// station relative to the anchor, range, sector.  w: the WallArgs.  in_range(jl) is the caller's range rule (the map's
// stations by wall_station, an align's patch rows); the sector, and its atan2f, is computed only for a point that passed
// gate and range.  The point's class goes to count(a literal kChain*); returns whether it is kChainMapped.  e is set
// unless the point is plane, jl from kChainOutside on, kk for kChainMapped.
enum : uint32_t { kChainPlane = 0u, kChainBeyondGate = 1u, kChainOutside = 2u, kChainMapped = 3u };
template <class Axis, class Args, class InRange, class Count>
__device__ __forceinline__ bool wall_chain(const float4 &q, uint32_t lab, const Args &w, const Axis &c, InRange in_range, Count count,
                                           float &e, float &jl, uint32_t &kk)
{
    constexpr int kAxis = Axis::kAxis;
    if (lab == 1u) { count(kChainPlane); return false; }
    float t, wx, wy, wz;   // (arc: wx = yc, wy = z, wz = cy; clothoid: wx = yc, wy = z, wz = ok)
    if constexpr (kAxis == kAxisClothoid)
        e = clothoid_residual(q, w.o, w.a, c.cl.arc.n, c.cl.arc.b, c.cl.arc.kappa, c.cl.rate, w.R, t, wx, wy, wz);
    else if constexpr (kAxis == kAxisArc) e = arc_residual(q, w.o, w.a, c.arc.n, c.arc.b, c.arc.kappa, w.R, t, wx, wy, wz);
    else e = surf_residual(q, w.o, w.a, w.R, t, wx, wy, wz);
    if (!(fabsf(e) <= w.gate) || (kAxis != kAxisStraight && !(wz > 0.0f))) { count(kChainBeyondGate); return false; }
    jl = surf_station(t, 0.0f, w.station_length);
    if (!in_range(jl)) { count(kChainOutside); return false; }
    if constexpr (kAxis == kAxisClothoid)
        kk = arc_sector(wx, wy, c.cl.arc.un, c.cl.arc.ub, c.cl.arc.vn, c.cl.arc.vb, w.two_pi, w.sector_angle, w.n_sectors);
    else if constexpr (kAxis == kAxisArc)
        kk = arc_sector(wx, wy, c.arc.un, c.arc.ub, c.arc.vn, c.arc.vb, w.two_pi, w.sector_angle, w.n_sectors);
    else kk = surf_sector(wx, wy, wz, w.u, w.v, w.two_pi, w.sector_angle, w.n_sectors);
    count(kChainMapped);
    return true;
}
// the map's station of jl, -1 outside [0, n_stations) (|jl| < 2^62 before the conversion: a far point of a stage call must
// not overflow it)
template <class Args>
__device__ __forceinline__ int64_t wall_station(const Args &w, float jl)
{
    const int64_t j = fabsf(jl) < 4.0e18f ? w.anchor + (int64_t)jl : -1;
    return j >= 0 && j < (int64_t)w.n_stations ? j : -1;
}
// ---- run merging: the common start of the segmented reductions (surf_merge_runs here, wc_merge_runs in k_wall_cloud.hip,
// k_wall_region_reduce, k_wall_object_reduce).  Runs of one key in consecutive lanes are folded into the run's head lane
// before anything goes to memory.  wave_runs finds the runs; the ladder stays with its caller, because its fields do:
//     if (r.any) for (o = 1; o < kWave; o <<= 1) { w.. = __shfl_down(v.., o, kWave); if (r.lane + o <= r.tail) fold v.., w..; }
// with EVERY shuffle of a step ahead of the one branch: the step's ds_bpermute are then issued back to back and waited for
// once.  Folding value by value (shuffle, select, next value) saves a dozen VGPRs and costs a wait per value: measured 7 %
// on k_wall_region_reduce over a sparsely flagged 2^24-cell map.  Wave-uniform: every lane is at the shuffles.
struct WaveRuns {
    int lane, tail;   // tail: the last lane of this lane's run (set when any)
    bool dup, any;    // dup: this lane continues the run of the lane below; any: some lane of the wave does
};
// key < 0: this lane has nothing.  A lane with key >= 0 && !dup adds what the ladder left it.
__device__ __forceinline__ WaveRuns wave_runs(int key)
{
    WaveRuns r;
    r.lane = threadIdx.x & (kWave - 1);
    const int prev = __shfl_up(key, 1, kWave);
    r.dup = r.lane > 0 && key >= 0 && prev == key;
    const unsigned long long dmask = __ballot(r.dup);
    r.any = dmask != 0ull;
    r.tail = r.lane;
    if (r.any) {
        const unsigned long long above = r.lane < kWave - 1 ? (~dmask & (~0ull << (r.lane + 1))) : 0ull;
        r.tail = above ? __ffsll((long long)above) - 2 : kWave - 1;
    }
    return r;
}
// runs of one cell (lidar rings put ~20 consecutive points into one sector).  Returns whether this lane still has to add
// its (merged) contribution.
__device__ __forceinline__ bool surf_merge_runs(int cell, uint32_t &cn, unsigned long long &sm, uint32_t &lo, uint32_t &hi)
{
    const WaveRuns r = wave_runs(cell);
    if (r.any) {
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t ocn = __shfl_down(cn, o, kWave), olo = __shfl_down(lo, o, kWave),
                           ohi = __shfl_down(hi, o, kWave);
            const unsigned long long osm = __shfl_down(sm, o, kWave);
            if (r.lane + o <= r.tail) {
                cn += ocn; sm += osm;
                lo = lo > olo ? lo : olo;
                hi = hi > ohi ? hi : ohi;
            }
        }
    }
    return cell >= 0 && !r.dup;
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// first index in sorted keys[0..n) whose key is >= key
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *__restrict__ keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int cell_coord(float x, float o, float inv_h, int n)
{
    int c = (int)floorf((x - o) * inv_h);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

__device__ __forceinline__ uint32_t cell_key(const GridParams &g, float x, float y, float z)
{
    int cx = cell_coord(x, g.ox, g.inv_hx, g.nx);
    int cy = cell_coord(y, g.oy, g.inv_h, g.ny);
    int cz = cell_coord(z, g.oz, g.inv_h, g.nz);
    return (uint32_t)((cz * g.ny + cy) * g.nx + cx);
}

// ---- symmetric 3x3 eigen-solvers (fp64) --------------------------------------

// Cyclic Jacobi; a = {xx,xy,xz,yy,yz,zz}.  w ascending, V column-major.
// One thread, once per frame (the K11 epilogue) -- clarity over speed.
__host__ __device__ inline void jacobi_eig3(const double a6[6], double w[3], double V[9])
{
    double a[3][3] = {{a6[0], a6[1], a6[2]}, {a6[1], a6[3], a6[4]}, {a6[2], a6[4], a6[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        double dg = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (off <= 1e-40 * dg || off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (a[ord[j]][ord[j]] < a[ord[i]][ord[i]]) { int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    for (int c = 0; c < 3; ++c) {
        w[c] = a[ord[c]][ord[c]];
        for (int r = 0; r < 3; ++r) V[3 * c + r] = v[r][ord[c]];
    }
}

// Symmetric 3x3 eigen-decomposition the way Eigen::SelfAdjointEigenSolver<MatrixXf>::compute reaches it for a
// dynamic-size matrix (/root/reference src/tunnel_processing.cpp:129): scale by max|a_ij|, one Householder reflection
// to tridiagonal form, implicit symmetric QR steps with Wilkinson shift and Givens rotations accumulated into the
// eigenvector matrix, ascending sort -- in the scalar type T with T's convergence thresholds.  The SIGNS of the
// returned eigenvectors (arbitrary mathematically, visible on /eigenBasisOutput as the arrow directions) depend on the
// number of QR sweeps, i.e. on the precision the iteration runs in: T = float reproduces the sign pattern of the
// reference's MatrixXf solve.  a = {xx,xy,xz,yy,yz,zz}; w ascending, V column-major.
// One rounding can change the number of sweeps, so every product is rounded (no contraction to FMAs, whatever the build's
// -ffp-contract): the device pass, the x86-64 host pass and the oracle's restatement then run one and the same sequence.
template <class T>
__host__ __device__ inline void eigen_tridiag_qr3(const T a6[6], T w[3], T V[9])
{
#pragma clang fp contract(off)
    typedef T double_;   // (the body below is written once for both scalar types)
    double_ scale = 0.0;
    for (int k = 0; k < 6; ++k) { const double_ t = a6[k] < 0 ? -a6[k] : a6[k]; if (t > scale) scale = t; }
    if (!(scale > 0.0)) scale = 1.0;
    const double_ a00 = a6[0] / scale, a10 = a6[1] / scale, a20 = a6[2] / scale, a11 = a6[3] / scale, a21 = a6[4] / scale,
                 a22 = a6[5] / scale;
    double_ Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double_ diag[3], sub[2];
    const double_ tiny = sizeof(T) == 4 ? (T)1.17549435e-38 : (T)2.2250738585072014e-308;
    if (a20 * a20 <= tiny) {              // column already tridiagonal: no reflection
        diag[0] = a00; diag[1] = a11; diag[2] = a22; sub[0] = a10; sub[1] = a21;
    } else {
        double_ beta = (T)sqrt((double)(a10 * a10 + a20 * a20));
        if (a10 >= 0) beta = -beta;
        const double_ ess = a20 / (a10 - beta), tau = (beta - a10) / beta;
        const double_ v[2] = {1.0, ess};
        double_ B[2][2] = {{a11, a21}, {a21, a22}};
        const double_ p0 = tau * (B[0][0] * v[0] + B[0][1] * v[1]), p1 = tau * (B[1][0] * v[0] + B[1][1] * v[1]);
        const double_ K = -0.5 * tau * (p0 * v[0] + p1 * v[1]);
        const double_ ww[2] = {p0 + K * v[0], p1 + K * v[1]};
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) B[i][j] -= v[i] * ww[j] + ww[i] * v[j];
        diag[0] = a00; diag[1] = B[0][0]; diag[2] = B[1][1]; sub[0] = beta; sub[1] = B[1][0];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) Q[1 + i][1 + j] = (i == j ? 1.0 : 0.0) - tau * v[i] * v[j];
    }
    int end = 2, start = 0, iter = 0;
    const double_ prec = sizeof(T) == 4 ? (T)(2.0 * 1.1920928955078125e-7) : (T)(2.0 * 2.220446049250313e-16);
    while (end > 0) {
        for (int i = start; i < end; ++i) {
            const double_ s = sub[i] < 0 ? -sub[i] : sub[i];
            const double_ d = (diag[i] < 0 ? -diag[i] : diag[i]) + (diag[i + 1] < 0 ? -diag[i + 1] : diag[i + 1]);
            if (s <= d * prec || s <= tiny) sub[i] = 0.0;
        }
        while (end > 0 && sub[end - 1] == 0.0) --end;
        if (end <= 0) break;
        if (++iter > 90) break;
        start = end - 1;
        while (start > 0 && sub[start - 1] != 0.0) --start;
        const double_ td = (diag[end - 1] - diag[end]) * 0.5, e = sub[end - 1];
        double_ mu = diag[end];
        if (td == 0.0) mu -= (e < 0 ? -e : e);
        else {
            const double_ h = (T)sqrt((double)(td * td + e * e));
            mu -= (e * e) / (td + (td > 0 ? h : -h));
        }
        double_ x = diag[start] - mu, z = sub[start];
        for (int k = start; k < end; ++k) {
            double_ c, s;   // Givens rotation taking (x, z) to (r, 0), Eigen's JacobiRotation::makeGivens conventions
            if (z == 0.0) { c = x < 0 ? -1.0 : 1.0; s = 0.0; }
            else if (x == 0.0) { c = 0.0; s = z < 0 ? 1.0 : -1.0; }
            else if ((x < 0 ? -x : x) > (z < 0 ? -z : z)) {
                const double_ t = z / x; double_ u = (T)sqrt((double)((T)1 + t * t));
                if (x < 0) u = -u;
                c = 1.0 / u; s = -t * c;
            } else {
                const double_ t = x / z; double_ u = (T)sqrt((double)((T)1 + t * t));
                if (z < 0) u = -u;
                s = -1.0 / u; c = -t * s;
            }
            const double_ sdk = s * diag[k] + c * sub[k], dkp1 = s * sub[k] + c * diag[k + 1];
            diag[k] = c * (c * diag[k] - s * sub[k]) - s * (c * sub[k] - s * diag[k + 1]);
            diag[k + 1] = s * sdk + c * dkp1;
            sub[k] = c * sdk - s * dkp1;
            if (k > start) sub[k - 1] = c * sub[k - 1] - s * z;
            x = sub[k];
            if (k < end - 1) { z = -s * sub[k + 1]; sub[k + 1] = c * sub[k + 1]; }
            for (int r = 0; r < 3; ++r) {
                const double_ xi = Q[r][k], yi = Q[r][k + 1];
                Q[r][k] = c * xi - s * yi;
                Q[r][k + 1] = s * xi + c * yi;
            }
        }
    }
    for (int i = 0; i < 2; ++i) {          // ascending selection sort, columns follow
        int k = i;
        for (int j = i + 1; j < 3; ++j) if (diag[j] < diag[k]) k = j;
        if (k != i) {
            const double_ t = diag[i]; diag[i] = diag[k]; diag[k] = t;
            for (int r = 0; r < 3; ++r) { const double_ u = Q[r][i]; Q[r][i] = Q[r][k]; Q[r][k] = u; }
        }
    }
    for (int c = 0; c < 3; ++c) {
        w[c] = diag[c] * scale;
        for (int r = 0; r < 3; ++r) V[3 * c + r] = Q[r][c];
    }
}


// Accurate eigenpairs (fp64 Jacobi) with the column signs of the reference's float solve (above, T = float).
__host__ __device__ inline void eig3_sym_eigen_signs(const double a6[6], double w[3], double V[9])
{
    jacobi_eig3(a6, w, V);
    float af[6], wf[3], Vf[9];
    for (int k = 0; k < 6; ++k) af[k] = (float)a6[k];
    eigen_tridiag_qr3<float>(af, wf, Vf);
    for (int c = 0; c < 3; ++c) {
        const double d = V[3 * c] * (double)Vf[3 * c] + V[3 * c + 1] * (double)Vf[3 * c + 1] + V[3 * c + 2] * (double)Vf[3 * c + 2];
        if (d < 0.0)
            for (int r = 0; r < 3; ++r) V[3 * c + r] = -V[3 * c + r];
    }
}

// inlier band of a cylinder hypothesis: (r-tau)^2 < dist_axis^2 < (r+tau)^2, both ends in fp32
__host__ __device__ inline void cyl_band(float r, double tau, float &lo2, float &hi2)
{
    const double lo = (double)r - tau, hi = (double)r + tau;
    lo2 = lo > 0 ? (float)(lo * lo) : -1.0f;
    hi2 = (float)(hi * hi);
}

// cylinder inlier predicate of the RANSAC scorers and label passes: lo2 < |v|^2 - (v.d)^2 < hi2, v = p - point on axis
__device__ __forceinline__ bool cyl_inlier(float x, float y, float z, float px, float py, float pz, float dx, float dy,
                                           float dz, float lo2, float hi2)
{
    const float vx = __fsub_rn(x, px), vy = __fsub_rn(y, py), vz = __fsub_rn(z, pz);
    const float t = __fmaf_rn(vx, dx, __fmaf_rn(vy, dy, __fmul_rn(vz, dz)));
    const float vv = __fmaf_rn(vx, vx, __fmaf_rn(vy, vy, __fmul_rn(vz, vz)));
    const float q = __fmaf_rn(-t, t, vv);
    return q > lo2 && q < hi2;
}

// ---- the frame's closing step: fixed-order reduction of the scatter partials + 3x3 eigen + result record -------------
// (SelfAdjointEigenSolver, /root/reference src/tunnel_processing.cpp:129-137.)  One 256-thread block; shared by
// k_frame_finalize and, when a RANSAC model is part of the frame, the tail of k_ext_finalize (one launch less).
// red: __shared__ double[256 * 6].
__device__ __forceinline__ void frame_finalize_block(const double *__restrict__ partials, uint32_t nblocks,
                                                     const DevCounters *__restrict__ ctr,
                                                     const VoxelParams *__restrict__ voxp, FrameOut *__restrict__ out,
                                                     double *red, uint32_t row_tile = 0)
{
    // row_tile != 0: the rows are the NaN-normal compaction's, one per row_tile cropped points (gm_compact.hpp); tiles
    // past the end of the cropped cloud wrote none
    if (row_tile) {
        const uint32_t rows = (ctr->n_cropped + row_tile - 1u) / row_tile;
        nblocks = rows < nblocks ? rows : nblocks;
    }
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] += partials[b * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) red[threadIdx.x * 6 + k] = m[k];
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride)
#pragma unroll
            for (int k = 0; k < 6; ++k) red[threadIdx.x * 6 + k] += red[(threadIdx.x + stride) * 6 + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double M[6], w[3], V[9];
        for (int k = 0; k < 6; ++k) { M[k] = red[k]; out->scatter[k] = M[k]; }
        eig3_sym_eigen_signs(M, w, V);   // fp64 Jacobi pairs, column signs of Eigen's float tridiagonal-QR solve
        for (int k = 0; k < 3; ++k) out->evals[k] = (float)w[k];
        for (int k = 0; k < 9; ++k) out->evecs[k] = (float)V[k];
        if (ctr) out->ctr = *ctr;
        if (voxp) out->vox = *voxp;
    }
}

}  // namespace gm
