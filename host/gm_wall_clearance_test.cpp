// gm_wall_clearance_test -- the host mirror's clearance: a 65 x 90 wall map (chainage 100 m) is filled with deterministic
// raw cells through gm_wall_map_add_raw, with an intrusion planted at stations 20 .. 23, sectors 10 .. 12.  The gauge is
// Processor::wallGaugeFromPolygon of a regular 360-gon of radius 1.8 m.  Processor::wallMapClearance is compared, byte for
// byte, with a direct gm_wall_map_clearance call and with a scalar C++ restatement of the rule of include/gm_hip.h on the
// cells read back, in both references, through a sub-window and with per-station tables; gm_wall_clearance_runs of the
// station records must name the intrusion's chainage.  Prints "gm_wall_clearance_test ok" on success.
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
static int64_t fix(float e)
{
    const volatile float p = e * 1048576.0f;
    if (p != p) return 0;
    if (p >= 2147483648.0f) return 2147483647ll;
    if (p <= -2147483648.0f) return -2147483647ll - 1;
    return (int64_t)std::nearbyint((double)p);   // to nearest, ties to even
}

static const unsigned kN = 65, kNs = 90;

// the rule, one cell at a time
static gm_wall_clearance_info restate(const std::vector<gm_wall_raw_cell> &raw, const gm_wall_params &prm, unsigned station0, unsigned n,
                                      const std::vector<int32_t> &gauge, const std::vector<uint8_t> &sg, const gm_wall_clearance_params &cp,
                                      std::vector<gm_wall_clearance_station> &stations, std::vector<gm_wall_clearance_cell> &cells)
{
    gm_wall_clearance_info info;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    info.station0 = station0; info.n_stations = n; info.n_sectors = kNs;
    info.margin_q = (int64_t)std::floor(cp.margin * 1048576.0 + 0.5);
    info.radius_q = (int64_t)std::floor(prm.radius * 1048576.0 + 0.5);
    info.min_clearance = INT64_MAX;
    info.min_cell = UINT32_MAX;
    stations.clear();
    cells.clear();
    for (unsigned j = 0; j < n; ++j) {
        gm_wall_clearance_station s;
        std::memset(&s, 0, sizeof(s));
        s.min_clearance = INT64_MAX;
        s.min_sector = UINT32_MAX;
        s.gauge = sg.empty() ? 0 : sg[j];
        for (unsigned k = 0; k < kNs; ++k) {
            const uint32_t cell = (station0 + j) * kNs + k;
            const gm_wall_raw_cell &c = raw[cell];
            const int64_t G = gauge[(size_t)s.gauge * kNs + k];
            if (G == 0) { ++info.ungauged; continue; }
            if (c.count == 0) { ++info.empty; ++s.unsurveyed; continue; }
            if (c.count < cp.min_count) { ++info.unusable; ++s.unsurveyed; continue; }
            int64_t w;
            if (cp.reference == GM_WALL_CLEAR_MEAN) {
                w = c.sum / (int64_t)c.count;
                w = w > (1 << 30) ? (1 << 30) : (w < -(1 << 30) ? -(1 << 30) : w);
            } else {
                w = fix(unordered(~c.min_key));
            }
            const int64_t cl = info.radius_q + w - G;
            ++s.usable;
            if (cl < s.min_clearance) { s.min_clearance = cl; s.min_sector = k; }
            if (cl < info.min_clearance) { info.min_clearance = cl; info.min_cell = cell; }
            if (cl < 0) { ++info.infringed; ++s.infringed; }
            else if (cl < info.margin_q) { ++info.tight; ++s.tight; }
            else { ++info.clear; continue; }
            gm_wall_clearance_cell r;
            r.cell = cell; r.count = c.count; r.clearance = cl;
            cells.push_back(r);
        }
        if (s.tight + s.infringed) ++info.stations_tight;
        if (s.infringed) ++info.stations_infringed;
        stations.push_back(s);
    }
    return info;
}

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(T)) == 0);
}
static bool same(const gm_wall_clearance_info &a, const gm_wall_clearance_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main()
{
    try {
        EXPECT(sizeof(gm_wall_clearance_station) == 32 && sizeof(gm_wall_clearance_cell) == 16);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = 100.0;
        gm_wall_clearance_params cp;
        gm_wall_clearance_default_params(&cp);
        EXPECT(cp.struct_size == sizeof(gm_wall_clearance_params) && cp.reference == GM_WALL_CLEAR_MIN && cp.min_count == 8 &&
               cp.margin == 0.10 && cp.reserved == 0);

        // the gauge: a regular 360-gon of radius 1.8 m, and a second table 0.25 m larger with the invert not gauged
        std::vector<double> uv;
        const double pi = 3.14159265358979323846;
        for (int i = 0; i < 360; ++i) { uv.push_back(1.8 * std::cos(pi * i / 180.0)); uv.push_back(1.8 * std::sin(pi * i / 180.0)); }
        std::vector<int32_t> gauge = Processor::wallGaugeFromPolygon(prm, uv);
        EXPECT(gauge.size() == kNs);
        for (unsigned k = 0; k < kNs; ++k) EXPECT(std::fabs(gauge[k] / 1048576.0 - 1.8) < 1e-5);
        bool refused = false;
        const double outside[2] = {5.0, 0.0};
        try { Processor::wallGaugeFromPolygon(prm, uv, outside); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);   // the axis is outside
        std::vector<int32_t> two(gauge);
        for (unsigned k = 0; k < kNs; ++k) two.push_back((k >= 40 && k < 50) ? 0 : gauge[k] + (1 << 18));

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        std::vector<gm_wall_clearance_station> st, st2, st3;
        std::vector<gm_wall_clearance_cell> ce, ce2, ce3;
        const std::vector<uint8_t> none;
        refused = false;
        try { proc.wallMapClearance(0, kN, gauge, none, cp, st, ce); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        gm_wall_clearance_info info = proc.wallMapClearance(0, kN, gauge, none, cp, st, ce);
        EXPECT(ce.empty() && st.size() == kN && info.empty == (uint64_t)kN * kNs && info.min_clearance == INT64_MAX);

        // every cell surveyed 10 times within a centimetre of the design; two stations thin; the intrusion 0.3 m inside
        std::vector<gm_wall_raw_cell> raw(kN * kNs);
        std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
        for (unsigned j = 0; j < kN; ++j)
            for (unsigned k = 0; k < kNs; ++k) {
                gm_wall_raw_cell &c = raw[j * kNs + k];
                const bool hit = j >= 20 && j <= 23 && k >= 10 && k <= 12;
                c.count = (j == 50 || j == 51) ? (k % 2 ? 3 : 0) : 10;
                if (!c.count) continue;
                const float lo = hit ? -0.3f : -0.01f, hi = hit ? -0.2f : 0.01f;
                c.sum = (int64_t)c.count * (hit ? -(1 << 18) : (int64_t)(k % 7) - 3);
                c.min_key = ~ordered(lo);
                c.max_key = ordered(hi);
            }
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK && nc == back.size());

        std::vector<uint8_t> sg(kN);
        for (unsigned j = 0; j < kN; ++j) sg[j] = (j / 8) % 2;
        struct Case { unsigned s0, n, reference; double margin; bool tables; };
        const Case cases[] = {{0, kN, GM_WALL_CLEAR_MIN, 0.10, false}, {0, kN, GM_WALL_CLEAR_MEAN, 0.10, false},
                              {15, 20, GM_WALL_CLEAR_MIN, 0.25, false}, {0, kN, GM_WALL_CLEAR_MEAN, 0.05, true},
                              {3, 60, GM_WALL_CLEAR_MIN, 0.0, true}, {30, 0, GM_WALL_CLEAR_MIN, 0.10, false}};
        for (size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++t) {
            const Case &c = cases[t];
            cp.reference = c.reference; cp.margin = c.margin;
            const std::vector<int32_t> &g = c.tables ? two : gauge;
            const std::vector<uint8_t> s(c.tables ? std::vector<uint8_t>(sg.begin() + c.s0, sg.begin() + c.s0 + c.n) : none);
            info = proc.wallMapClearance(c.s0, c.n, g, s, cp, st, ce);
            // the ABI directly
            gm_wall_clearance_info info2;
            uint64_t count = 0;
            EXPECT(gm_wall_map_clearance(proc.wallMap(), c.s0, c.n, &g[0], c.tables ? 2 : 1, s.empty() ? 0 : &s[0], &cp, &info2, 0, 0, 0, 0,
                                         &count) == GM_OK && count == ce.size());
            st2.assign(c.n ? c.n : 1, gm_wall_clearance_station());
            ce2.assign(count ? count : 1, gm_wall_clearance_cell());
            EXPECT(gm_wall_map_clearance(proc.wallMap(), c.s0, c.n, &g[0], c.tables ? 2 : 1, s.empty() ? 0 : &s[0], &cp, &info2, &st2[0],
                                         c.n, &ce2[0], count, &count) == GM_OK);
            st2.resize(c.n);
            ce2.resize(count);
            EXPECT(same(st, st2) && same(ce, ce2) && same(info, info2));
            // the rule restated
            const gm_wall_clearance_info info3 = restate(back, prm, c.s0, c.n, g, s, cp, st3, ce3);
            EXPECT(same(st, st3) && same(ce, ce3) && same(info, info3));
            EXPECT(info.ungauged + info.empty + info.unusable + info.infringed + info.tight + info.clear == (uint64_t)c.n * kNs);
            std::printf("case %zu: window %u+%u -> %llu infringed, %llu tight, %llu clear, %llu unusable, %llu empty, %llu not gauged\n", t,
                        c.s0, c.n, (unsigned long long)info.infringed, (unsigned long long)info.tight, (unsigned long long)info.clear,
                        (unsigned long long)info.unusable, (unsigned long long)info.empty, (unsigned long long)info.ungauged);
            if (t == 0) {
                EXPECT(info.infringed == 12 && info.stations_infringed == 4 && info.tight == 0 && info.min_cell == 20 * kNs + 10);
                EXPECT(info.unusable == 90 && info.empty == 90);
                // the runs name the intrusion's chainage: stations 20 .. 23 of 0.25 m from 100 m
                uint32_t nr = 0;
                EXPECT(gm_wall_clearance_runs(&prm, &st[0], kN, 0, 0, 0, 0, &nr) == GM_OK && nr == 1);
                gm_wall_clearance_run run;
                EXPECT(gm_wall_clearance_runs(&prm, &st[0], kN, 0, 0, &run, 1, &nr) == GM_OK && nr == 1);
                EXPECT(run.station_from == 20 && run.station_to == 23 && run.chainage_from == 105.0 && run.chainage_to == 106.0);
                EXPECT(run.infringed == 12 && run.tight == 0 && run.min_station == 20 && run.min_sector == 10 && run.angle_deg == 42.0);
                EXPECT(run.min_clearance == info.min_clearance && std::fabs(run.min_clearance_m + 0.1) < 1e-4);
            }
            if (t == 2) {   // a margin above the wall's 0.19 m: every station of the window is short of it, one run
                uint32_t nr = 0;
                gm_wall_clearance_run run;
                EXPECT(gm_wall_clearance_runs(&prm, &st[0], c.n, c.s0, 2, &run, 1, &nr) == GM_OK && nr == 1);
                EXPECT(run.station_from == 15 && run.station_to == 34 && run.chainage_from == 103.75 && run.chainage_to == 108.75);
                EXPECT(run.min_station == 20 && run.infringed == 12 && info.tight == 20 * kNs - 12 && run.tight == info.tight);
            }
            if (t == 5) EXPECT(st.empty() && ce.empty() && info.min_cell == UINT32_MAX);
        }
        // the map was not changed
        std::vector<gm_wall_raw_cell> again(raw.size());
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &again[0], again.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&again[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        refused = false;
        try { proc.wallMapClearance(64, 2, gauge, none, cp, st, ce); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        cp.min_count = 0;
        refused = false;
        try { proc.wallMapClearance(0, kN, gauge, none, cp, st, ce); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_clearance_test ok\n");
    return 0;
}
