// gm_wall_cloud_test -- the host mirror's wall cloud: a 65 x 65 wall map (oblique design, chainage 5 km) is filled with
// deterministic raw cells through gm_wall_map_add_raw, and Processor::wallMapCloud is compared, byte for byte, with a
// direct gm_wall_map_cloud call and with a scalar C++ restatement of the rule of include/gm_hip.h on the cells read back
// (gm_wall_map_read_raw), the map's reported design frame (gm_wall_map_info) and gm_wall_cloud_directions' table -- at
// the map's resolution, decimated with ragged blocks, through a sub-window, and with one block wider than the map.
// Prints "gm_wall_cloud_test ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gm_tunnel_processing.hpp"

using namespace gm_host;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
    } while (0)

static unsigned long long lcg(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static uint32_t ordered(float e)
{
    uint32_t b;
    std::memcpy(&b, &e, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static float unordered(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// one rounding each, whatever the compiler would like to contract
static double mul(double a, double b) { volatile double r = a * b; return r; }
static double add(double a, double b) { volatile double r = a + b; return r; }

static const unsigned kN = 65, kNs = 65;

// the rule, one block at a time
static std::vector<gm_wall_cloud_point> restate(const std::vector<gm_wall_raw_cell> &raw, const gm_wall_params &prm, const gm_wall_info &wi,
                                                unsigned station0, unsigned n, const gm_wall_cloud_params &cp, gm_wall_cloud_info &info)
{
    std::vector<gm_wall_cloud_point> out;
    const unsigned bs = cp.block_stations < n ? cp.block_stations : (n ? n : 1), bk = cp.block_sectors < kNs ? cp.block_sectors : kNs;
    const unsigned NJ = (n + bs - 1) / bs, NK = (kNs + bk - 1) / bk;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    info.station0 = station0; info.n_stations = n; info.n_sectors = kNs;
    info.blocks_stations = NJ; info.blocks_sectors = NK;
    info.blocks = (uint64_t)NJ * NK;
    std::vector<double> dirs(2 * NK);
    uint32_t got = 0;
    EXPECT(gm_wall_cloud_directions(&prm, &cp, &dirs[0], NK, &got) == GM_OK && got == NK);
    for (unsigned J = 0; J < NJ; ++J)
        for (unsigned K = 0; K < NK; ++K) {
            const unsigned j0 = station0 + J * bs, ns = (station0 + n - j0 < bs) ? station0 + n - j0 : bs;
            const unsigned k0 = K * bk, nk = (kNs - k0 < bk) ? kNs - k0 : bk;
            uint64_t count = 0;
            int64_t sum = 0;
            uint32_t lo = 0, hi = 0, cells = 0;
            for (unsigned j = j0; j < j0 + ns; ++j)
                for (unsigned k = k0; k < k0 + nk; ++k) {
                    const gm_wall_raw_cell &c = raw[(size_t)j * kNs + k];
                    count += c.count; sum += c.sum;
                    lo = lo > c.min_key ? lo : c.min_key;
                    hi = hi > c.max_key ? hi : c.max_key;
                    cells += c.count ? 1u : 0u;
                }
            if (!count) { ++info.empty; continue; }
            if (count < cp.min_count) { ++info.below_min_count; continue; }
            ++info.points;
            const double m = mul((double)sum, 1.0 / 1048576.0) / (double)count;
            const double h = mul((double)(2 * j0 + ns), 0.5);
            const double tc = add(prm.t_min, mul(h, prm.station_length));
            const double rho = add(wi.R, mul(cp.exaggeration, m));
            const double c = dirs[2 * K], s = dirs[2 * K + 1];
            float xyz[3];
            for (int i = 0; i < 3; ++i) {
                const double w = add(mul(c, wi.u[i]), mul(s, wi.v[i]));
                xyz[i] = (float)add(add(add(wi.o[i], -cp.anchor[i]), mul(tc, wi.a[i])), mul(rho, w));
            }
            gm_wall_cloud_point p;
            std::memset(&p, 0, sizeof(p));
            p.x = xyz[0]; p.y = xyz[1]; p.z = xyz[2];
            p.mean = (float)m;
            p.min = unordered(~lo);
            p.max = unordered(hi);
            p.block = J * NK + K;
            p.cells = cells;
            p.count = count;
            out.push_back(p);
        }
    return out;
}

static bool same(const std::vector<gm_wall_cloud_point> &a, const std::vector<gm_wall_cloud_point> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(gm_wall_cloud_point)) == 0);
}
static bool same(const gm_wall_cloud_info &a, const gm_wall_cloud_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main()
{
    try {
        EXPECT(sizeof(gm_wall_cloud_point) == 40);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = 5000.0;
        prm.station_length = 0.3;
        prm.radius = 3.1;
        prm.point[0] = 3.0; prm.point[1] = -1.0; prm.point[2] = 0.5;
        prm.direction[0] = 0.9; prm.direction[1] = 0.2; prm.direction[2] = -0.1;
        gm_wall_cloud_params cp;
        gm_wall_cloud_default_params(&cp);
        EXPECT(cp.struct_size == sizeof(gm_wall_cloud_params) && cp.block_stations == 1 && cp.block_sectors == 1 && cp.min_count == 1 &&
               cp.exaggeration == 1.0 && cp.anchor[0] == 0.0 && cp.anchor[1] == 0.0 && cp.anchor[2] == 0.0 && cp.reserved == 0);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.wallMapCloud(0, kN, cp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        gm_wall_cloud_info info, info2, info3;
        EXPECT(proc.wallMapCloud(0, kN, cp, &info).empty() && info.blocks == kN * kNs && info.empty == info.blocks);

        // half of the cells filled: counts 1 .. 20, sums of both signs
        std::vector<gm_wall_raw_cell> raw(kN * kNs);
        std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
        unsigned long long seed = 4711;
        for (size_t i = 0; i < raw.size(); ++i) {
            if (lcg(seed) & 1) continue;
            const uint32_t cnt = 1 + (uint32_t)(lcg(seed) % 20);
            const float lo = -0.25f * (float)(lcg(seed) % 1000) / 1000.0f, hi = 0.25f * (float)(lcg(seed) % 1000) / 1000.0f;
            const double mean = lo + (hi - lo) * (double)(lcg(seed) % 1000) / 1000.0;
            raw[i].sum = (int64_t)std::floor(mean * cnt * 1048576.0 + 0.5);
            raw[i].count = cnt;
            raw[i].min_key = ~ordered(lo);
            raw[i].max_key = ordered(hi);
        }
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK && nc == back.size());
        EXPECT(std::memcmp(&back[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        const gm_wall_info wi = proc.wallMapInfo();

        // an anchor near the window, as a publisher would set it
        for (int i = 0; i < 3; ++i) cp.anchor[i] = wi.o[i] + 5000.0 * wi.a[i];
        struct Case { unsigned s0, n, bs, bk, min_count; double g; };
        const Case cases[] = {{0, kN, 1, 1, 1, 1.0}, {0, kN, 7, 5, 8, 50.0}, {3, 40, 2, 3, 1, 0.0}, {0, kN, 64, 64, 1, 1.0},
                              {10, 55, 200, 5000, 1, 1.0}, {60, 0, 4, 4, 1, 1.0}};
        for (size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++t) {
            const Case &c = cases[t];
            cp.block_stations = c.bs; cp.block_sectors = c.bk; cp.min_count = c.min_count; cp.exaggeration = c.g;
            const std::vector<gm_wall_cloud_point> got = proc.wallMapCloud(c.s0, c.n, cp, &info);
            // the ABI directly
            uint64_t count = 0;
            EXPECT(gm_wall_map_cloud(proc.wallMap(), c.s0, c.n, &cp, &info2, 0, 0, &count) == GM_OK && count == got.size());
            std::vector<gm_wall_cloud_point> direct(count ? count : 1);
            EXPECT(gm_wall_map_cloud(proc.wallMap(), c.s0, c.n, &cp, &info2, &direct[0], count, &count) == GM_OK);
            direct.resize(count);
            EXPECT(same(got, direct) && same(info, info2));
            // the rule restated
            const std::vector<gm_wall_cloud_point> want = restate(back, prm, wi, c.s0, c.n, cp, info3);
            EXPECT(same(got, want) && same(info, info3));
            EXPECT(info.points + info.below_min_count + info.empty == info.blocks && info.points == got.size());
            for (size_t i = 1; i < got.size(); ++i) EXPECT(got[i - 1].block < got[i].block);
            std::printf("case %zu: window %u+%u, blocks %ux%u -> %llu blocks, %llu points, %llu below min_count, %llu empty\n", t, c.s0,
                        c.n, c.bs, c.bk, (unsigned long long)info.blocks, (unsigned long long)info.points,
                        (unsigned long long)info.below_min_count, (unsigned long long)info.empty);
            if (t == 0) EXPECT(got.size() > 1500 && got.size() < 2700);
            if (t == 4) EXPECT(got.size() == 1 && got[0].block == 0 && info.blocks == 1);
            if (t == 5) EXPECT(got.empty() && info.blocks == 0);
        }
        // the map was not changed
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&back[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        refused = false;
        try { proc.wallMapCloud(64, 2, cp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        cp.min_count = 0;
        refused = false;
        try { proc.wallMapCloud(0, kN, cp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_cloud_test ok\n");
    return 0;
}
