// gm_wall_check_test -- the host mirror's wall-map check: an 80 x 90 wall map is filled with deterministic raw cells
// through gm_wall_map_add_raw, a synthetic tunnel frame with a displaced strip goes through processFrame, and
// Processor::checkWallMap is compared, byte for byte, with a direct gm_wall_map_check_frame / gm_wall_map_get_check call,
// with the stage call gm_wall_map_check_points on the frame's /choppedCloud, and with a scalar C++ restatement of the
// integer rule of include/gm_hip.h on the cells read back (gm_wall_map_read_raw) and the per-point (e, cell) pairs of an
// add to a scratch map whose gate is the check's -- for both references.  Prints "gm_wall_check_test ok" on success.
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
static double uni(unsigned long long &s) { return (double)(lcg(s) % 1000000) / 1000000.0; }

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
// (int64) rint(e 2^20): one fp32 product, rounded to nearest even (every value here is far inside the int32 range)
static int64_t fix(float e)
{
    volatile float p = e * 1048576.0f;
    return (int64_t)std::nearbyint((double)p);
}

static const unsigned kN = 80, kNs = 90;

// the rule, one point at a time
static std::vector<gm_wall_check_point> restate(const PointCloud &cloud, const std::vector<float> &e, const std::vector<int32_t> &cell,
                                                const std::vector<gm_wall_raw_cell> &raw, const gm_wall_check_params &cp,
                                                gm_wall_check_info &info)
{
    std::vector<gm_wall_check_point> out;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    const int64_t T = (int64_t)std::nearbyint(cp.threshold * 1048576.0);
    info.threshold_q = T;
    info.n_points = (uint32_t)cloud.size();
    const float gate = (float)cp.gate;
    for (size_t i = 0; i < cloud.size(); ++i) {
        if (!(std::fabs(e[i]) <= gate)) { ++info.beyond_gate; continue; }
        if (cell[i] < 0) { ++info.outside; continue; }
        const gm_wall_raw_cell &c = raw[(size_t)cell[i]];
        if (c.count < cp.min_count) { ++info.unsurveyed; continue; }
        const int64_t eq = fix(e[i]);
        int64_t delta;
        if (cp.reference == GM_WALL_CHECK_ENVELOPE) {
            const int64_t lq = fix(unordered(~c.min_key)), hq = fix(unordered(c.max_key));
            delta = eq > hq ? eq - hq : (eq < lq ? eq - lq : 0);
        } else {
            delta = eq - c.sum / (int64_t)c.count;
        }
        if (delta < T && delta > -T) { ++info.unchanged; continue; }
        if (delta >= T) { ++info.changed_pos; if (delta > info.peak_pos) info.peak_pos = delta; }
        else { ++info.changed_neg; if (delta < info.peak_neg) info.peak_neg = delta; }
        gm_wall_check_point p;
        p.x = cloud[i].x; p.y = cloud[i].y; p.z = cloud[i].z;
        p.delta = (float)delta * (1.0f / 1048576.0f);
        p.e = e[i];
        p.cell = cell[i];
        p.index = (uint32_t)i;
        std::memcpy(&p.row, &cloud[i].pad, 4);
        out.push_back(p);
        // the host-only classifier says the same of this pair
        int64_t d2 = 0;
        uint32_t cls = 99;
        EXPECT(gm_wall_check_classify(&cp, &c, e[i], &d2, &cls) == GM_OK && d2 == delta &&
               cls == (uint32_t)(delta >= T ? GM_WALL_CHECK_CLS_CHANGED_POS : GM_WALL_CHECK_CLS_CHANGED_NEG));
    }
    return out;
}

static bool same(const std::vector<gm_wall_check_point> &a, const std::vector<gm_wall_check_point> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(gm_wall_check_point)) == 0);
}
static bool same(const gm_wall_check_info &a, const gm_wall_check_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main()
{
    try {
        EXPECT(sizeof(gm_wall_check_point) == 32);
        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        EXPECT(cp.struct_size == sizeof(gm_wall_check_params) && cp.reference == GM_WALL_CHECK_MEAN && cp.min_count == 8 &&
               cp.reserved == 0 && cp.threshold == 0.05 && cp.gate == 1.0);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = -10.0;
        const double pose[12] = {1, 0, 0, 0.125, 0, 1, 0, 0.0625, 0, 0, 1, -0.03125};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.checkWallMap(pose, cp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.checkWallMap(pose, cp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no frame yet

        // the survey: nine cells in ten filled, counts 1 .. 20, means within 2 cm of the design, a spread of up to 5 cm
        std::vector<gm_wall_raw_cell> raw(kN * kNs);
        std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
        unsigned long long seed = 4711;
        for (size_t i = 0; i < raw.size(); ++i) {
            if (lcg(seed) % 10 == 0) continue;
            const uint32_t cnt = 1 + (uint32_t)(lcg(seed) % 20);
            const float lo = -0.05f * (float)uni(seed), hi = 0.05f * (float)uni(seed);
            const double mean = 0.4 * (lo + (hi - lo) * uni(seed));
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

        // the frame: a tunnel of radius 2 along the design axis, 1 cm of noise, a strip of the ring (16 %) moved out by 10 cm.
        // With survey means within 2 cm and a 4 cm threshold: the strip is changed+, the rest unchanged, and the quarter
        // of the cells that are empty or hold fewer than 4 points is unsurveyed
        const unsigned n = 20000;
        std::vector<float> rows(4 * n);
        for (unsigned i = 0; i < n; ++i) {
            const double t = -4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
            const double r = 2.0 + 0.02 * (uni(seed) - 0.5) + (phi < 1.0 ? 0.1 : 0.0);
            // (map coordinates minus the pose's translation: the sensor sits off the axis, the wall on the design)
            rows[4 * i] = (float)(t - pose[3]); rows[4 * i + 1] = (float)(r * std::cos(phi) - pose[7]);
            rows[4 * i + 2] = (float)(r * std::sin(phi) - pose[11]);
            rows[4 * i + 3] = 0.0f;
        }
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        const PointCloud cloud = proc.choppedCloud();
        EXPECT(cloud.size() == fr.n_valid);
        std::vector<float> xyz(3 * cloud.size());
        for (size_t i = 0; i < cloud.size(); ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }

        gm_wall_map *scratch = 0;
        for (int ref = 0; ref < 2; ++ref) {
            cp.reference = (uint32_t)ref;
            cp.min_count = 4;
            cp.threshold = 0.04;
            cp.gate = 0.5;
            gm_wall_check_info info, info2, info3, info4;
            const std::vector<gm_wall_check_point> got = proc.checkWallMap(pose, cp, &info);
            // the ABI directly
            gm_wall_add_info ai;
            EXPECT(gm_wall_map_check_frame(proc.wallMap(), proc.ctx(), 0, pose, &cp, &ai) == GM_OK && ai.gate == 0.5f);
            uint32_t count = 0;
            EXPECT(gm_wall_map_get_check(proc.wallMap(), 0, &info2, 0, 0, &count) == GM_OK && count == got.size());
            std::vector<gm_wall_check_point> direct(count ? count : 1);
            EXPECT(gm_wall_map_get_check(proc.wallMap(), 0, &info2, &direct[0], count, &count) == GM_OK);
            direct.resize(count);
            EXPECT(same(got, direct) && same(info, info2));
            // the per-point chain: an add to a scratch map on the same grid whose gate is the check's
            if (!scratch) {
                gm_wall_params sp = prm;
                sp.gate = cp.gate;
                EXPECT(gm_wall_map_create(proc.ctx(), &sp, &scratch) == GM_OK);
            }
            std::vector<float> e(cloud.size());
            std::vector<int32_t> cell(cloud.size());
            EXPECT(gm_wall_map_add_points(scratch, &xyz[0], (uint32_t)cloud.size(), 0, pose, 0, &e[0], &cell[0]) == GM_OK);
            const std::vector<gm_wall_check_point> want = restate(cloud, e, cell, back, cp, info3);
            info3.status = info.status;
            EXPECT(same(got, want) && same(info, info3));
            // the stage call on the same cloud: the same rows but for row = index
            std::vector<gm_wall_check_point> staged(cloud.size());
            std::vector<uint8_t> cls(cloud.size());
            EXPECT(gm_wall_map_check_points(proc.wallMap(), &xyz[0], (uint32_t)cloud.size(), 0, pose, &cp, 0, &info4, &staged[0],
                                            (uint32_t)staged.size(), &count, 0, 0, 0, &cls[0]) == GM_OK);
            staged.resize(count);
            EXPECT(count == got.size() && same(info, info4));
            for (size_t i = 0; i < staged.size() && i < got.size(); ++i) {
                EXPECT(staged[i].row == staged[i].index && cls[staged[i].index] >= GM_WALL_CHECK_CLS_CHANGED_POS);
                staged[i].row = got[i].row;
            }
            EXPECT(same(got, staged));
            const uint32_t sum = info.plane + info.beyond_gate + info.outside + info.unsurveyed + info.unchanged + info.changed_pos + info.changed_neg;
            EXPECT(sum == info.n_points && info.n_points == cloud.size() && info.changed_pos + info.changed_neg == got.size());
            for (size_t i = 1; i < got.size(); ++i) EXPECT(got[i - 1].index < got[i].index);
            std::printf("reference %d: %u points, %u unsurveyed, %u unchanged, %u changed+, %u changed-, peaks %lld %lld\n", ref, info.n_points,
                        info.unsurveyed, info.unchanged, info.changed_pos, info.changed_neg, (long long)info.peak_pos, (long long)info.peak_neg);
            EXPECT(info.changed_pos > 1000 && info.unchanged > 5000 && info.unsurveyed > 500 && info.peak_pos > 0);
            // the frame path needs a frame again (the stage calls took slot 0)
            proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        }
        // the map was not changed
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&back[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        EXPECT(proc.wallMapInfo().frames == 0);
        cp.threshold = 9.0;
        refused = false;
        try { proc.checkWallMap(pose, cp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_check_test ok\n");
    return 0;
}
