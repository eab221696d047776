// k_wall_sections.hip -- BUILD-DEFINED EXTENSION: a robust profile fit per chainage section (gm_wall_map_sections), the
// device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_sections_np.py.  One kernel, launched
// once per fitting pass and once more for the evaluation (gm_wall.hip solves the small systems between the launches).
// A wave per section, the sections of a chunk dealt to the waves of a capped grid; integers throughout:
//   A. lanes take consecutive sectors, 64 at a time, so the SoA table is read coalesced.  A lane merges the stations of
//      its column (count u64, sum i64, as k_wall_cloud_merge does), forms m, the model of the pass before, rho and
//      whether the column is SELECTED (usable and |rho| <= thr), and leaves m -- or "not selected" -- in the wave's LDS
//      strip.  The class counts and the largest cyclic gap come from ballots: wave-uniform words, no lane of its own;
//      rss, the points and the two peaks (packed (rho, sector) words) are reduced by shuffles.
//   B. (fitting launches) lanes take the entries of the normal equations, 45 + 9 at the most.  Each walks the strip
//      with ONE accumulator: the strip word is a broadcast read, the basis row (<= 36 B of a table of <= 147 KB that
//      stays in L2) one line.  No 54 live accumulators per lane and no 54-value wave reduction.
// No atomics, no ticket, no floating point: the bytes do not depend on the grid, the block shape or the order.
#include "gm_internal.hpp"

namespace gm {

static_assert(sizeof(gm_wall_section_sums) == 448 && sizeof(gm_wall_section) == 144, "the records of include/gm_hip.h");
static_assert(sizeof(WallSectionOut) == 512 && sizeof(WallSectionModel) == 80, "16-byte multiples: the chunk arrays are carved back to back");
constexpr int kWsThreads = 128, kWsWaves = kWsThreads / kWave;   // 16 KiB of strip per wave
constexpr uint32_t kWsMaxBlocks = 8192;
constexpr int32_t kWsNone = -2147483647 - 1;   // the strip word of a column that is not selected (|m| <= 2^24)
constexpr uint32_t kWsTri = 45;                // slots of N

template <class T>
__device__ __forceinline__ T ws_wave_min(T v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, kWave);
        v = t < v ? t : v;
    }
    return v;
}

template <class T>
__device__ __forceinline__ T ws_wave_max(T v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, kWave);
        v = t > v ? t : v;
    }
    return v;
}

// count and sum of column k of table T over window stations [j0, j1)
__device__ __forceinline__ void ws_merge(const WallTable &T, uint64_t first, uint32_t nsec, uint32_t j0, uint32_t j1, uint32_t k,
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

// The longest cyclic run of sectors that are not selected, fed 64 sectors at a time in order.  Every word is wave-uniform.
struct WsGap {
    uint32_t run = 0u, lead = 0u, best = 0u;   // the open run at the end so far, the run before the first selected, the longest closed
    bool seen = false;
    // sel: the selected lanes of this group (a subset of its nv valid ones)
    __device__ __forceinline__ void feed(unsigned long long sel, uint32_t nv)
    {
        if (!sel) {
            run += nv;
            return;
        }
        const uint32_t head = (uint32_t)__builtin_ctzll(sel), top = 63u - (uint32_t)__builtin_clzll(sel);
        const uint32_t g = run + head;
        if (!seen) lead = g;
        else best = g > best ? g : best;
        seen = true;
        // the longest run strictly between two selected lanes of the group
        unsigned long long z = ~sel & ((2ull << top) - 1ull) & ~((1ull << head) - 1ull);
        uint32_t len = 0u;
        while (z) {
            z &= z << 1;
            ++len;
        }
        best = len > best ? len : best;
        run = nv - 1u - top;
    }
    __device__ __forceinline__ uint32_t close(uint32_t nsec) const
    {
        if (!seen) return nsec;
        const uint32_t g = run + lead;
        return g > best ? g : best;
    }
};

__global__ __launch_bounds__(kWsThreads) void k_wall_sections(WallSectionArgs a)
{
    __shared__ int32_t s_m[kWsWaves][GM_WALL_MAX_SECTORS];
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x / kWave, nsec = a.nsec, P = a.P;
    int32_t *strip = s_m[wave];
    // phase B's entry of this lane: N[ep][eq] in packed order, then r[ep]
    const uint32_t NP = P * (P + 1u) / 2u, NE = NP + P;
    uint32_t ep = 0u, eq = 0u;
    const bool is_r = (uint32_t)lane >= NP;
    if (is_r) {
        ep = (uint32_t)lane - NP;
    } else {
        uint32_t e = (uint32_t)lane;
        while (e >= P - ep) {
            e -= P - ep;
            ++ep;
        }
        eq = ep + e;
    }
    // wave-uniform trips: a section per wave
    for (uint32_t i = blockIdx.x * kWsWaves + wave; i < a.nsect; i += gridDim.x * kWsWaves) {
        const WallSectionModel &mdl = a.model[i];
        if (!mdl.alive) continue;
        long long c[kWallSectionCoefs];
#pragma unroll
        for (uint32_t p = 0; p < kWallSectionCoefs; ++p) c[p] = p < P ? mdl.c[p] : 0ll;
        const uint32_t j0 = (a.sec0 + i) * a.S;                      // < n: the section exists
        const uint32_t j1 = a.n - j0 < a.S ? a.n : j0 + a.S;

        // ---- A: columns ----
        uint32_t n_empty = 0u, n_usable = 0u, n_unusable = 0u, n_sel = 0u;
        WsGap gap;
        unsigned long long rss = 0ull, pts = 0ull;
        unsigned long long kout = 0ull;      // (rho + bias) << 12 | 4095 - k: the largest; 0: no usable column
        unsigned long long kin = ~0ull;      // (rho + bias) << 12 | k: the smallest
        for (uint32_t base = 0; base < nsec; base += kWave) {
            const uint32_t k = base + (uint32_t)lane;
            bool empty = false, usable = false, sel = false;
            if (k < nsec) {
                unsigned long long cn, sm, bcn = 0ull, bsm = 0ull;
                ws_merge(a.map, a.first, nsec, j0, j1, k, cn, sm);
                if (a.has_base) ws_merge(a.base, a.first, nsec, j0, j1, k, bcn, bsm);
                empty = cn == 0ull && bcn == 0ull;
                usable = cn >= (unsigned long long)a.min_count && (!a.has_base || bcn >= (unsigned long long)a.min_count);
                int32_t word = kWsNone;
                if (usable) {
                    long long q = wall_section_value((long long)sm, cn);
                    if (a.has_base)   // (wraps instead of overflowing on merged cells of no survey)
                        q = (long long)((unsigned long long)q - (unsigned long long)wall_section_value((long long)bsm, bcn));
                    const long long m = wall_section_sat(q);
                    const int32_t *__restrict__ Bk = a.basis + (size_t)k * P;
                    long long acc = 1ll << 19;
#pragma unroll
                    for (uint32_t p = 0; p < kWallSectionCoefs; ++p)
                        if (p < P) acc += (long long)Bk[p] * c[p];
                    const long long rho = m - (acc >> 20);
                    sel = (rho < 0 ? -rho : rho) <= a.thr;
                    const unsigned long long key = (unsigned long long)(rho + kWallSectionBias) << 12;
                    const unsigned long long ko = key | (unsigned long long)(4095u - k), ki = key | (unsigned long long)k;
                    kout = ko > kout ? ko : kout;
                    kin = ki < kin ? ki : kin;
                    if (sel) {
                        rss += (unsigned long long)rho * (unsigned long long)rho;   // (wraps in a pass without a threshold)
                        pts += cn;
                        word = (int32_t)m;
                    }
                }
                strip[k] = word;
            }
            const unsigned long long bs = __ballot(sel), be = __ballot(empty), bu = __ballot(usable);
            const uint32_t nv = nsec - base < (uint32_t)kWave ? nsec - base : (uint32_t)kWave;
            const uint32_t ce = (uint32_t)__popcll(be), cu = (uint32_t)__popcll(bu);
            n_empty += ce;
            n_usable += cu;
            n_unusable += nv - ce - cu;
            n_sel += (uint32_t)__popcll(bs);
            gap.feed(bs, nv);
        }
        rss = wave_sum(rss);
        pts = wave_sum(pts);
        kout = ws_wave_max(kout);
        kin = ws_wave_min(kin);
        WallSectionOut &o = a.out[i];
        if (lane == 0) {
            o.sums.fitted = n_sel;
            o.sums.largest_gap = gap.close(nsec);
            o.sums.points = pts;
            o.rss = rss;
            const bool any = kout != 0ull;
            o.peak_out = any ? (long long)(kout >> 12) - kWallSectionBias : 0ll;
            o.peak_in = any ? (long long)(kin >> 12) - kWallSectionBias : 0ll;
            o.peak_out_sector = any ? 4095u - (uint32_t)(kout & 0xFFFull) : 0xFFFFFFFFu;
            o.peak_in_sector = any ? (uint32_t)(kin & 0xFFFull) : 0xFFFFFFFFu;
            o.empty = n_empty;
            o.unusable = n_unusable;
            o.usable = n_usable;
            o.pad0 = 0u;
            o.pad1[0] = 0ull;
            o.pad1[1] = 0ull;
        }

        // ---- B: the normal equations ----
        wave_lds_fence();
        if (a.fit) {
            long long acc = 0ll;
            if ((uint32_t)lane < NE) {
#pragma unroll 8
                for (uint32_t k = 0; k < nsec; ++k) {   // (no branch on the strip word: the loads of the trips overlap)
                    const int32_t mk = strip[k];
                    const int32_t *__restrict__ Bk = a.basis + (size_t)k * P;
                    const long long other = is_r ? (long long)mk : (long long)Bk[eq];
                    const long long term = (long long)Bk[ep] * other;
                    acc += mk != kWsNone ? term : 0ll;
                }
            }
            if ((uint32_t)lane < NP) o.sums.N[lane] = acc;
            else if ((uint32_t)lane < NE) o.sums.r[(uint32_t)lane - NP] = acc;
            if ((uint32_t)lane >= NP && (uint32_t)lane < kWsTri) o.sums.N[lane] = 0ll;
            if ((uint32_t)lane >= P && (uint32_t)lane < kWallSectionCoefs) o.sums.r[lane] = 0ll;
        }
        wave_lds_fence();   // the next section of this wave rewrites the strip
    }
}

void launch_wall_sections(const WallSectionArgs &a, hipStream_t s)
{
    uint32_t b = (a.nsect + kWsWaves - 1u) / kWsWaves;   // nsect >= 1
    b = b > kWsMaxBlocks ? kWsMaxBlocks : b;
    hipLaunchKernelGGL(k_wall_sections, dim3(b), dim3(kWsThreads), 0, s, a);
}

}  // namespace gm
