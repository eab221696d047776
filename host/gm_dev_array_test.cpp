// gm_dev_array_test.cpp -- the memory owners of csrc/gm_dev_array.hpp on the CPU.  Plain g++ (no device, no HIP
// runtime): the four HIP calls the owners use are defined here on top of malloc / free, with a count of live blocks and
// an "N-th allocation fails" switch.  Built with -fsanitize=address,undefined by tests/test_host_dev_array.py: a block
// freed twice, used after its release or never freed ends the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../geometric_mapping_amd/csrc/gm_dev_array.hpp"
#include "../include/gm_hip.h"

namespace {
long g_live[2] = {0, 0};   // blocks out: device, pinned
long g_peak[2] = {0, 0};   // the most at once since the last reset
long g_allocs = 0;         // allocation calls so far
long g_fail_at = -1;       // the allocation call with this index fails (once)

hipError_t stub_alloc(int kind, void **p, size_t bytes)
{
    if (g_allocs++ == g_fail_at) {
        *p = reinterpret_cast<void *>(0x10);   // (a failed call leaves garbage behind: the owner must not keep it)
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    if (++g_live[kind] > g_peak[kind]) g_peak[kind] = g_live[kind];
    return hipSuccess;
}
hipError_t stub_free(int kind, void *p)
{
    if (p) --g_live[kind];
    std::free(p);
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc(0, p, bytes); }
hipError_t hipFree(void *p) { return stub_free(0, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return stub_alloc(1, p, bytes); }
hipError_t hipHostFree(void *p) { return stub_free(1, p); }
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// how the callers map an owner's error (GM_HIP, GMW_HIP)
static gm_status status_of(hipError_t e) { return e == hipSuccess ? GM_OK : (e == hipErrorOutOfMemory ? GM_ERR_OOM : GM_ERR_DEVICE); }

struct Rec { double v[3]; uint32_t n; };

template <template <class> class Array>
static int run(int kind)
{
    const long long live0 = gm::g_live_buffers.load();
    REQUIRE(g_live[kind] == 0);
    {
        Array<Rec> a;
        uint32_t gen = 0;
        // empty: null, reserve(0) keeps it so and moves nothing
        REQUIRE(!a && a.p == nullptr && a.cap == 0);
        REQUIRE(a.reserve(0, &gen) == hipSuccess && a.p == nullptr && gen == 0 && gm::g_live_buffers.load() == live0);
        // first block
        REQUIRE(a.reserve(100, &gen) == hipSuccess && a && a.cap == 100 && gen == 1);
        REQUIRE(g_live[kind] == 1 && gm::g_live_buffers.load() == live0 + 1);
        for (uint32_t i = 0; i < 100; ++i) a[i].n = i;              // reads like a pointer: [], ->, +, conversion, ?:
        a->n = 7;
        Rec *raw = a;
        const Rec *q = a + 99;
        REQUIRE(raw == a.p && raw[0].n == 7 && q->n == 99 && (*a).n == 7 && &a->v[1] == &raw->v[1]);
        Array<Rec> other;
        REQUIRE((gen ? a : other) == raw && static_cast<const void *>(a) == raw);
        // no-op reserves: same block, the generation stays
        const long allocs = g_allocs;
        REQUIRE(a.reserve(100, &gen) == hipSuccess && a.reserve(5, &gen) == hipSuccess && a.reserve(0, &gen) == hipSuccess);
        REQUIRE(a.reserve(100) == hipSuccess);
        REQUIRE(a.p == raw && a.cap == 100 && gen == 1 && g_allocs == allocs);
        // growth: the old block goes before the new one comes (never two at once), contents are not kept, never shrinks
        g_peak[kind] = g_live[kind];
        REQUIRE(a.reserve(101, &gen) == hipSuccess && a.cap == 101 && gen == 2 && g_peak[kind] == 1 && g_live[kind] == 1);
        std::memset(a.p, 0xAB, sizeof(Rec) * 101);                  // (the whole new block is ours)
        REQUIRE(a.reserve(50, &gen) == hipSuccess && a.cap == 101 && gen == 2);
        REQUIRE(gm::g_live_buffers.load() == live0 + 1);
        // move: the block changes hands once, the source is empty and may be destroyed or reused
        raw = a;
        Array<Rec> b(std::move(a));
        REQUIRE(b.p == raw && b.cap == 101 && a.p == nullptr && a.cap == 0 && g_live[kind] == 1);
        REQUIRE(a.reserve(3, &gen) == hipSuccess && gen == 3 && g_live[kind] == 2 && gm::g_live_buffers.load() == live0 + 2);
        std::vector<Array<Rec>> v;                                  // (a std::vector of owners grows)
        for (int k = 0; k < 9; ++k) {
            v.emplace_back();
            REQUIRE(v.back().reserve(4 + k) == hipSuccess);
        }
        REQUIRE(g_live[kind] == 11 && v[0].cap == 4 && v[8].cap == 12);
        // explicit release, twice
        b.release();
        b.release();
        REQUIRE(!b && b.cap == 0 && g_live[kind] == 10);
        // a failed growth: the old block is gone, the array is empty, the generation moved, the error maps as before
        REQUIRE(a.cap == 3);
        g_fail_at = g_allocs;
        const hipError_t e = a.reserve(1000, &gen);
        REQUIRE(e == hipErrorOutOfMemory && status_of(e) == GM_ERR_OOM && a.p == nullptr && a.cap == 0 && gen == 4);
        REQUIRE(g_live[kind] == 9 && gm::g_live_buffers.load() == live0 + 9);
        REQUIRE(a.reserve(1000, &gen) == hipSuccess && a.cap == 1000 && gen == 5);   // ... and the retry starts over
    }
    REQUIRE(g_live[kind] == 0 && gm::g_live_buffers.load() == live0);

    // a group of arrays grown together (a slot's frame buffers): the allocation fails at every position in turn, during
    // the first growth and during a regrowth.  The group is then destructible and the next call completes it.
    for (int regrow = 0; regrow < 2; ++regrow)
        for (int pos = 0; pos < 4; ++pos) {
            Array<float> g0;
            Array<uint8_t> g1;
            Array<Rec> g2;
            Array<double> g3;
            uint32_t gen = 0, cap = 0;   // cap: the group's size, 0 until every array is in place
            auto grow = [&](uint32_t n) -> hipError_t {
                cap = 0;
                hipError_t e = g0.reserve(n, &gen);
                if (e == hipSuccess) e = g1.reserve(n, &gen);
                if (e == hipSuccess) e = g2.reserve(16, &gen);   // (a size that does not follow n: allocated once)
                if (e == hipSuccess) e = g3.reserve(2 * (uint64_t)n, &gen);
                if (e == hipSuccess) cap = n;
                return e;
            };
            uint32_t n = 10;
            if (regrow) {
                REQUIRE(grow(n) == hipSuccess && cap == 10 && gen == 4);
                n = 20;
            }
            const uint32_t gen0 = gen;
            const void *fixed = g2.p;
            // (on a regrowth g2 does not allocate: three allocations, the last position never fails)
            const int n_allocs = regrow ? 3 : 4;
            g_fail_at = g_allocs + pos;
            const hipError_t e = grow(n);
            if (pos >= n_allocs) {
                REQUIRE(e == hipSuccess && cap == n);
                g_fail_at = -1;
            } else {
                REQUIRE(e == hipErrorOutOfMemory && cap == 0);
                const bool held[4] = {g0.p != nullptr, g1.p != nullptr, g2.p != nullptr, g3.p != nullptr};
                const int failed = regrow && pos == 2 ? 3 : pos;   // the array whose allocation failed
                for (int k = 0; k < 4; ++k) {
                    if (k == failed) REQUIRE(!held[k]);
                    else if (k < failed || regrow) REQUIRE(held[k]);
                    else REQUIRE(!held[k]);
                }
                REQUIRE(gen == gen0 + (uint32_t)pos + 1);
                REQUIRE(grow(n) == hipSuccess && cap == n);
            }
            REQUIRE(g0.cap == n && g1.cap == n && g2.cap == 16 && g3.cap == 2 * n && g0 && g1 && g2 && g3);
            if (regrow) REQUIRE(g2.p == fixed);
            REQUIRE(g_live[kind] == 4);
        }
    REQUIRE(g_live[kind] == 0 && gm::g_live_buffers.load() == live0);
    return 0;
}

int main()
{
    if (run<gm::DevArray>(0)) return 1;
    if (run<gm::HostArray>(1)) return 1;
    // the two kinds go through their own calls and share the one count
    {
        gm::DevArray<int> d;
        gm::HostArray<int> h;
        REQUIRE(d.reserve(8) == hipSuccess && h.reserve(8) == hipSuccess);
        REQUIRE(g_live[0] == 1 && g_live[1] == 1 && gm::g_live_buffers.load() == 2);
        uint8_t block[64];
        gm::Carve c{block};
        REQUIRE(c.take<uint32_t>(3) == (void *)block && c.take<uint8_t>(1) == block + 12 && c.at == block + 13);
    }
    REQUIRE(g_live[0] == 0 && g_live[1] == 0 && gm::g_live_buffers.load() == 0);
    std::printf("gm_dev_array_test ok\n");
    return 0;
}
