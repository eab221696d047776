// k_wall_clearance.hip -- BUILD-DEFINED EXTENSION: the surveyed wall against a structure gauge (gm_wall_map_clearance),
// the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_clearance_np.py.  Two passes, both
// streams over the SoA table (count always; min_key or sum of the usable gauged cells only), integers throughout:
//   1. k_wall_clear_stations  one wave per station row of the window, the rows dealt to the waves of a capped grid.  Lanes
//      take consecutive sectors, so the table and the gauge row are read coalesced (the gauge rows, <= 16 KiB each, stay
//      in L2).  Each lane keeps its class counts and the least (c, sector) it met as one packed word; shuffles reduce
//      them across the wave and lane 0 writes the 32-byte record.  The totals gather in LDS and leave with one integer
//      atomic per block and counter; the window's least clearance is one 64-bit integer maximum of the inverted
//      (c biased, cell) word.  No floating-point atomics: the result does not depend on the grid or the order.
//   2. k_compact<WallClearPred, WallClearEmit>  (gm_compact.hpp) per chunk of whole stations: the predicate recomputes
//      the class and keeps tight and infringed, with (count, c) as its payload; the emit step writes the 16-byte row at
//      the survivor's rank in the staging buffer, so the rows leave in cell order from one launch.
// Not fused: the list is skipped altogether by a count query and by a window whose totals say it is empty.
#include "gm_compact.hpp"
#include "gm_internal.hpp"

namespace gm {

static_assert(sizeof(gm_wall_clearance_station) == 32 && sizeof(gm_wall_clearance_cell) == 16, "the records of include/gm_hip.h");
constexpr int kWkThreads = 256, kWkWaves = kWkThreads / kWave;
constexpr uint32_t kWkMaxBlocks = 2048;
constexpr unsigned long long kWkNone = ~0ull;   // no usable gauged cell yet: above every packed word

// Class (kWallClear*) of window cell (station row j, sector k) whose map-wide index is cell; c and count of a usable
// gauged one.
__device__ __forceinline__ uint32_t wk_classify(const WallClearArgs &a, const int32_t *__restrict__ G, uint32_t k, uint64_t cell,
                                                uint32_t &count, long long &c)
{
    const long long g = G[k];
    count = a.map.cnt[cell];
    c = 0;
    if (g == 0) return kWallClearUngauged;
    if (count == 0u) return kWallClearEmpty;
    if (count < a.min_count) return kWallClearUnusable;
    const long long w = a.reference == GM_WALL_CLEAR_MEAN ? wall_clear_value(GM_WALL_CLEAR_MEAN, (long long)a.map.sum[cell], count, 0u)
                                                          : wall_clear_value(GM_WALL_CLEAR_MIN, 0, count, a.map.lo[cell]);
    c = a.Rq + w - g;
    return wall_clear_class(c, a.T);
}

__device__ __forceinline__ unsigned long long wk_wave_min(unsigned long long v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, kWave);
        v = t < v ? t : v;
    }
    return v;
}

// ---- 1. stations ----

__global__ __launch_bounds__(kWkThreads) void k_wall_clear_stations(WallClearArgs a)
{
    __shared__ uint32_t s_cls[8];                 // the six classes, stations_tight, stations_infringed
    __shared__ unsigned long long s_min;          // least (c biased, cell) of the block
    if (threadIdx.x < 8) s_cls[threadIdx.x] = 0u;
    if (threadIdx.x == 8) s_min = kWkNone;
    __syncthreads();
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x / kWave, nsec = a.nsec;
    // wave-uniform trips: a row per wave
    for (uint32_t j = blockIdx.x * kWkWaves + wave; j < a.n; j += gridDim.x * kWkWaves) {
        const uint32_t g = a.station_gauge ? a.station_gauge[j] : 0u;
        const int32_t *__restrict__ G = a.gauge + (size_t)g * nsec;
        const uint64_t row = a.first + (uint64_t)j * nsec;
        uint32_t cls[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        unsigned long long best = kWkNone;        // (c + bias) << 12 | sector: the smallest sector among equals
        for (uint32_t k = lane; k < nsec; k += kWave) {
            uint32_t count;
            long long c;
            const uint32_t cl = wk_classify(a, G, k, row + k, count, c);
#pragma unroll
            for (uint32_t q = 0; q < 6u; ++q) cls[q] += cl == q ? 1u : 0u;
            if (cl >= kWallClearInfringed) {
                const unsigned long long key = ((unsigned long long)(c + kWallClearBias) << 12) | k;
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 6u; ++q) cls[q] = wave_sum(cls[q]);
        best = wk_wave_min(best);
        if (lane == 0) {
            gm_wall_clearance_station r;
            const bool any = best != kWkNone;
            const long long cmin = (long long)(best >> 12) - kWallClearBias;
            const uint32_t kmin = (uint32_t)(best & 0xFFFull);
            r.min_clearance = any ? cmin : 0x7FFFFFFFFFFFFFFFll;
            r.min_sector = any ? kmin : 0xFFFFFFFFu;
            r.usable = cls[kWallClearInfringed] + cls[kWallClearTight] + cls[kWallClearClear];
            r.tight = cls[kWallClearTight];
            r.infringed = cls[kWallClearInfringed];
            r.unsurveyed = cls[kWallClearEmpty] + cls[kWallClearUnusable];
            r.gauge = g;
            a.stations[j] = r;
#pragma unroll
            for (uint32_t q = 0; q < 6u; ++q)
                if (cls[q]) atomicAdd(&s_cls[q], cls[q]);
            if (r.tight + r.infringed) atomicAdd(&s_cls[6], 1u);
            if (r.infringed) atomicAdd(&s_cls[7], 1u);
            if (any) atomicMin(&s_min, ((unsigned long long)(cmin + kWallClearBias) << 24) | (row + kmin));
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint32_t c = s_cls[threadIdx.x];
        if (c) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)c);
    } else if (threadIdx.x == 8) {
        if (s_min != kWkNone) atomicMax(&a.ctr[8], ~s_min);
    }
}

// ---- 2. compact + emit ----

struct WallClearPred {
    WallClearArgs a;
    struct Payload { uint32_t count; long long c; };
    __device__ __forceinline__ bool operator()(uint32_t i, Payload &p) const
    {
        const uint32_t jl = i / a.nsec, k = i - jl * a.nsec, j = a.j0 + jl;   // window station j < n
        const uint32_t g = a.station_gauge ? a.station_gauge[j] : 0u;
        const uint32_t cl = wk_classify(a, a.gauge + (size_t)g * a.nsec, k, a.first + (uint64_t)j * a.nsec + k, p.count, p.c);
        return cl == kWallClearInfringed || cl == kWallClearTight;
    }
};

struct WallClearEmit {
    static constexpr bool kHasFinish = false, kHasPrepare = false;
    WallClearArgs a;
    __device__ __forceinline__ void operator()(uint32_t src, uint32_t dst, const WallClearPred::Payload &p) const
    {
        gm_wall_clearance_cell r;
        r.cell = (uint32_t)(a.first + (uint64_t)a.j0 * a.nsec + src);   // < 2^24
        r.count = p.count;
        r.clearance = p.c;
        a.out[dst] = r;
    }
};

void launch_wall_clear_stations(const WallClearArgs &a, hipStream_t s)
{
    uint32_t b = (a.n + kWkWaves - 1u) / kWkWaves;   // n >= 1
    b = b > kWkMaxBlocks ? kWkMaxBlocks : b;
    hipLaunchKernelGGL(k_wall_clear_stations, dim3(b), dim3(kWkThreads), 0, s, a);
}

void launch_wall_clear_list(const WallClearArgs &a, const ScanState &st, hipStream_t s)
{
    const uint32_t nc = a.nj * a.nsec;   // 1 .. 2^20 (one station of <= 4096 sectors at the least)
    WallClearPred pred{a};
    WallClearEmit emit{a};
    hipLaunchKernelGGL((k_compact<WallClearPred, WallClearEmit>), dim3(compact_grid(nc)), dim3(kCpThreads), 0, s, pred, emit,
                       (const uint32_t *)nullptr, nc, st, reinterpret_cast<uint32_t *>(a.ctr + 9), (uint32_t *)nullptr);
}

}  // namespace gm
