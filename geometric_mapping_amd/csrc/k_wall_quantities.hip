// k_wall_quantities.hip -- BUILD-DEFINED EXTENSION: over- and underbreak per section and zone (gm_wall_map_quantities),
// the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_quantities_np.py.  One kernel per
// chunk of whole sections, a wave per section, the sections dealt to the waves of a capped grid as k_wall_clear_stations
// deals its rows; integers throughout:
//   - lanes take consecutive sectors, 64 at a time, and walk the section's S rows, so every row of the SoA table is read
//     coalesced: count and sum only, 12 of a cell's 20 bytes (24 with a baseline).  The two line rows (<= 16 KiB each) and
//     the zone table stay in L2.
//   - the six classes are counted by ballots: wave-uniform words.  The per-zone figures stay in the lane: eight words
//     (the packed counts, the points, the three areas, the two peaks) for the zone its columns lie in.  Only when some
//     lane's zone changes -- at a zone border, not once per group of 64 columns -- are the lanes' words folded into the
//     wave's 8 x 8 words of LDS, zone by zone in wave-uniform trips: sums by shuffles, a peak as the maximum of one packed
//     (value, ~sector) word, so that ties resolve to the smallest sector; lane 0 adds the trip's result.  Lane z writes
//     the record of zone z at the end.
//   - the profile row leaves coalesced; the class totals gather in LDS and leave with one integer atomic per block and
//     counter.
// No floating point, no floating-point atomics, no ticket: the bytes do not depend on the chunk, the grid, the block
// shape or the order.
#include "gm_internal.hpp"

namespace gm {

static_assert(sizeof(gm_wall_quantity) == 88 && sizeof(gm_wall_quantities_info) == 96, "the records of include/gm_hip.h");
static_assert(GM_WALL_QUANTITY_MAX_ZONES == 8u && kWave == 64, "a wave's accumulators are 8 zones x 8 words: one per lane");
constexpr int kWqThreads = 256, kWqWaves = kWqThreads / kWave;
constexpr uint32_t kWqMaxBlocks = 2048;
// a zone's words: under | within << 32, over | unsurveyed << 32, points, under_area, over_area, excess_area, the two keys
constexpr int kWqWords = 8;
constexpr uint32_t kWqNoZone = 0xFFFFFFFFu;   // a lane that holds nothing yet

__device__ __forceinline__ unsigned long long wq_wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, kWave);
        v = t > v ? t : v;
    }
    return v;
}

// count and sum of column k of table T over window stations [j0, j1): k_wall_sections' merge
__device__ __forceinline__ void wq_merge(const WallTable &T, uint64_t first, uint32_t nsec, uint32_t j0, uint32_t j1, uint32_t k,
                                         unsigned long long &cn, unsigned long long &sm)
{
    cn = 0ull;
    sm = 0ull;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint64_t c = first + (uint64_t)j * nsec + k;
        const uint32_t cc = T.cnt[c];
        const unsigned long long cs = T.sum[c];   // (loaded whatever the count says: the loads of a column do not wait for each other)
        cn += cc;
        sm += cc ? cs : 0ull;
    }
}

__global__ __launch_bounds__(kWqThreads) void k_wall_quantities(WallQuantityArgs a)
{
    __shared__ unsigned long long s_acc[kWqWaves][GM_WALL_QUANTITY_MAX_ZONES * kWqWords];
    __shared__ uint32_t s_cls[kWallQuantityCounters];
    if (threadIdx.x < (uint32_t)kWallQuantityCounters) s_cls[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x / kWave, nsec = a.nsec, nz = a.n_zones;
    unsigned long long *acc = s_acc[wave];
    // wave-uniform trips: a section per wave
    for (uint32_t i = blockIdx.x * kWqWaves + wave; i < a.nsect; i += gridDim.x * kWqWaves) {
        const uint32_t sec = a.sec0 + i;
        const uint32_t j0 = sec * a.S;                               // < n: the section exists
        const uint32_t j1 = a.n - j0 < a.S ? a.n : j0 + a.S;
        const uint32_t prof = a.section_profile ? a.section_profile[sec] : 0u;
        const int32_t *__restrict__ lo = a.lo + (size_t)prof * nsec;
        const int32_t *__restrict__ hi = a.hi + (size_t)prof * nsec;
        acc[lane] = 0ull;
        wave_lds_fence();
        uint32_t cls[6] = {0u, 0u, 0u, 0u, 0u, 0u};                  // wave-uniform
        uint32_t cur = kWqNoZone;                                    // the zone of this lane's words (< n_zones: the host checked the table)
        unsigned long long st[kWqWords] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        // the lanes' words into the wave's, zone by zone in wave-uniform trips: sums by shuffles, a peak as the maximum of
        // its packed (value, ~sector) word; lane 0 adds the trip's result
        auto flush = [&]() {
            unsigned long long todo = __ballot(cur != kWqNoZone);
            while (todo) {
                const uint32_t zz = (uint32_t)__shfl((int)cur, (int)__builtin_ctzll(todo), kWave);
                const bool mine = cur == zz;
                todo &= ~__ballot(mine);
                unsigned long long r[kWqWords];   // (a word that is 0 in every lane of the zone -- no UNDER column, no excess -- is not reduced)
#pragma unroll
                for (int q = 0; q < 6; ++q) r[q] = __ballot(mine && st[q] != 0ull) ? wave_sum(mine ? st[q] : 0ull) : 0ull;
                r[6] = __ballot(mine && st[6] != 0ull) ? wq_wave_max(mine ? st[6] : 0ull) : 0ull;
                r[7] = __ballot(mine && st[7] != 0ull) ? wq_wave_max(mine ? st[7] : 0ull) : 0ull;
                if (lane == 0) {
                    unsigned long long *w = acc + zz * kWqWords;
#pragma unroll
                    for (int q = 0; q < 6; ++q) w[q] += r[q];
                    w[6] = r[6] > w[6] ? r[6] : w[6];
                    w[7] = r[7] > w[7] ? r[7] : w[7];
                }
            }
            cur = kWqNoZone;
#pragma unroll
            for (int q = 0; q < kWqWords; ++q) st[q] = 0ull;
        };
        for (uint32_t base = 0; base < nsec; base += kWave) {
            const uint32_t k = base + (uint32_t)lane;
            const bool valid = k < nsec;
            uint32_t z = GM_WALL_QUANTITY_UNMEASURED;
            WallQuantityColumn c;
            c.cls = GM_WALL_QUANTITY_CLASS_UNMEASURED;
            c.usable = false;
            c.v = c.line = c.under = c.over = c.excess = 0;
            unsigned long long cn = 0ull;
            if (valid) {
                unsigned long long sm, bcn = 0ull, bsm = 0ull;
                z = a.zone ? a.zone[k] : 0u;
                wq_merge(a.map, a.first, nsec, j0, j1, k, cn, sm);
                if (a.has_base) wq_merge(a.base, a.first, nsec, j0, j1, k, bcn, bsm);
                c = wall_quantity_column(a.Rq, cn, (long long)sm, a.has_base != 0u, bcn, (long long)bsm, a.min_count, lo[k], hi[k],
                                         z == GM_WALL_QUANTITY_UNMEASURED);
                if (a.rows) a.rows[(size_t)i * nsec + k] = c.usable ? (int32_t)c.v : kWallQuantityNoValue;
            }
            const bool measured = valid && z != GM_WALL_QUANTITY_UNMEASURED;
            const bool under = measured && c.cls == GM_WALL_QUANTITY_CLASS_UNDER;
            const bool over = measured && c.cls == GM_WALL_QUANTITY_CLASS_OVER;
            const bool within = measured && c.cls == GM_WALL_QUANTITY_CLASS_WITHIN;
            const bool above = measured && c.usable && c.line > 0;   // x > L: WITHIN or OVER
            cls[GM_WALL_QUANTITY_CLASS_UNMEASURED] += (uint32_t)__popcll(__ballot(valid && !measured));
            cls[GM_WALL_QUANTITY_CLASS_EMPTY] += (uint32_t)__popcll(__ballot(measured && c.cls == GM_WALL_QUANTITY_CLASS_EMPTY));
            cls[GM_WALL_QUANTITY_CLASS_UNUSABLE] += (uint32_t)__popcll(__ballot(measured && c.cls == GM_WALL_QUANTITY_CLASS_UNUSABLE));
            cls[GM_WALL_QUANTITY_CLASS_UNDER] += (uint32_t)__popcll(__ballot(under));
            cls[GM_WALL_QUANTITY_CLASS_OVER] += (uint32_t)__popcll(__ballot(over));
            cls[GM_WALL_QUANTITY_CLASS_WITHIN] += (uint32_t)__popcll(__ballot(within));
            // A lane keeps the figures of the zone its columns lie in; they are folded into the wave's words only when a
            // lane's zone changes, so at a zone border and not once per group.
            if (__ballot(measured && cur != kWqNoZone && cur != z)) flush();
            if (measured) {
                const unsigned long long kinv = (unsigned long long)(4095u - k);
                const unsigned long long ku = under ? ((unsigned long long)(-c.line) << 12) | kinv : 0ull;
                const unsigned long long ko = above ? ((unsigned long long)c.line << 12) | kinv : 0ull;
                cur = z;
                st[0] += (under ? 1ull : 0ull) | (within ? 1ull << 32 : 0ull);
                st[1] += (over ? 1ull : 0ull) | (c.usable ? 0ull : 1ull << 32);
                st[2] += c.usable ? cn : 0ull;
                st[3] += (unsigned long long)c.under;    // (0 unless UNDER, as the two below are 0 outside their columns)
                st[4] += (unsigned long long)c.over;
                st[5] += (unsigned long long)c.excess;
                st[6] = ku > st[6] ? ku : st[6];
                st[7] = ko > st[7] ? ko : st[7];
            }
        }
        flush();
        wave_lds_fence();
        if ((uint32_t)lane < nz) {
            const unsigned long long *w = acc + (uint32_t)lane * kWqWords;
            gm_wall_quantity r;
            r.station_from = a.station0 + j0;
            r.stations = j1 - j0;
            r.zone = (uint32_t)lane;
            r.profile = prof;
            r.under = (uint32_t)w[0];
            r.within = (uint32_t)(w[0] >> 32);
            r.over = (uint32_t)w[1];
            r.unsurveyed = (uint32_t)(w[1] >> 32);
            r.points = w[2];
            r.under_area = (long long)w[3];
            r.over_area = (long long)w[4];
            r.excess_area = (long long)w[5];
            r.peak_under = (long long)(w[6] >> 12);
            r.peak_over = (long long)(w[7] >> 12);
            r.peak_under_sector = w[6] ? 4095u - (uint32_t)(w[6] & 0xFFFull) : 0xFFFFFFFFu;
            r.peak_over_sector = w[7] ? 4095u - (uint32_t)(w[7] & 0xFFFull) : 0xFFFFFFFFu;
            a.records[(size_t)i * nz + (uint32_t)lane] = r;
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t q = 0; q < 6u; ++q)
                if (cls[q]) atomicAdd(&s_cls[q], cls[q]);
            if (cls[GM_WALL_QUANTITY_CLASS_UNDER]) atomicAdd(&s_cls[6], 1u);
            if (cls[GM_WALL_QUANTITY_CLASS_OVER]) atomicAdd(&s_cls[7], 1u);
        }
        wave_lds_fence();   // the next section of this wave rewrites the accumulators
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kWallQuantityCounters) {
        const uint32_t c = s_cls[threadIdx.x];
        if (c) atomicAdd(&a.ctr[threadIdx.x], (unsigned long long)c);
    }
}

void launch_wall_quantities(const WallQuantityArgs &a, hipStream_t s)
{
    uint32_t b = (a.nsect + kWqWaves - 1u) / kWqWaves;   // nsect >= 1
    b = b > kWqMaxBlocks ? kWqMaxBlocks : b;
    hipLaunchKernelGGL(k_wall_quantities, dim3(b), dim3(kWqThreads), 0, s, a);
}

}  // namespace gm
