// gm_wall_add_checked_test -- the host mirror's checked add: an 80 x 90 wall map is filled with deterministic raw cells
// through gm_wall_map_add_raw, a synthetic tunnel frame with a displaced strip goes through processFrame and
// Processor::checkWallMap, and Processor::addToWallMapChecked is compared, byte for byte in the raw cells and in the totals,
// with gm_wall_map_add_points of the frame's /choppedCloud less the points a scalar C++ restatement of the row rule of
// include/gm_hip.h selects, and with the stage call gm_wall_map_add_points_checked on the same cloud and rows.  Prints
// "gm_wall_add_checked_test ok" on success.
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
// (int64) rint(e 2^20): one fp32 product, rounded to nearest even (every value here is far inside the int32 range)
static int64_t fix(float e)
{
    volatile float p = e * 1048576.0f;
    return (int64_t)std::nearbyint((double)p);
}

static const unsigned kN = 80, kNs = 90;

static std::vector<gm_wall_raw_cell> raw_of(gm_wall_map *m)
{
    std::vector<gm_wall_raw_cell> c(kN * kNs);
    uint64_t nc = 0;
    EXPECT(gm_wall_map_read_raw(m, 0, kN, &c[0], c.size(), &nc) == GM_OK && nc == c.size());
    return c;
}
static bool same_map(gm_wall_map *a, gm_wall_map *b)
{
    const std::vector<gm_wall_raw_cell> ca = raw_of(a), cb = raw_of(b);
    gm_wall_info ia, ib;
    EXPECT(gm_wall_map_info(a, &ia) == GM_OK && gm_wall_map_info(b, &ib) == GM_OK);
    return std::memcmp(&ca[0], &cb[0], ca.size() * sizeof(gm_wall_raw_cell)) == 0 && ia.mapped == ib.mapped && ia.outside == ib.outside &&
           ia.beyond_gate == ib.beyond_gate && ia.plane == ib.plane && ia.cells_hit == ib.cells_hit && ia.frames == ib.frames;
}

int main()
{
    try {
        gm_wall_add_checked_params ap;
        gm_wall_add_checked_default_params(&ap);
        EXPECT(ap.struct_size == sizeof(gm_wall_add_checked_params) && ap.skip == (GM_WALL_SKIP_NEG | GM_WALL_SKIP_POS) && ap.min_delta == 0.0);
        EXPECT(sizeof(gm_wall_add_checked_params) == 16 && sizeof(gm_wall_add_checked_info) == 64);
        EXPECT(gm_wall_add_checked_check_params(&ap) == GM_OK);
        ap.skip = 0;
        EXPECT(gm_wall_add_checked_check_params(&ap) == GM_ERR_INVALID_ARG);
        ap.skip = 3;
        ap.min_delta = 8.5;
        EXPECT(gm_wall_add_checked_check_params(&ap) == GM_ERR_INVALID_ARG);
        ap.min_delta = 0.10;

        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        cp.min_count = 4;
        cp.threshold = 0.04;
        cp.gate = 0.5;
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = -10.0;
        const double pose[12] = {1, 0, 0, 0.125, 0, 1, 0, 0.0625, 0, 0, 1, -0.03125};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
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
        gm_wall_map *plain = 0, *staged = 0;   // the same survey twice more: the filtered plain add, the stage call
        EXPECT(gm_wall_map_create(proc.ctx(), &prm, &plain) == GM_OK && gm_wall_map_create(proc.ctx(), &prm, &staged) == GM_OK);
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK && gm_wall_map_add_raw(plain, 0, kN, &raw[0]) == GM_OK &&
               gm_wall_map_add_raw(staged, 0, kN, &raw[0]) == GM_OK);

        // the frame: a tunnel of radius 2 along the design axis, 1 cm of noise, a strip of the ring (16 %) moved out by 10 cm:
        // with a 4 cm threshold the strip is changed+, and about half of its rows reach min_delta = 10 cm
        const unsigned n = 20000;
        std::vector<float> rows(4 * n);
        for (unsigned i = 0; i < n; ++i) {
            const double t = -4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
            const double r = 2.0 + 0.02 * (uni(seed) - 0.5) + (phi < 1.0 ? 0.1 : 0.0);
            rows[4 * i] = (float)(t - pose[3]); rows[4 * i + 1] = (float)(r * std::cos(phi) - pose[7]);
            rows[4 * i + 2] = (float)(r * std::sin(phi) - pose[11]);
            rows[4 * i + 3] = 0.0f;
        }
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no check of this frame yet
        const std::vector<gm_wall_check_point> changed = proc.checkWallMap(pose, cp);
        gm_wall_add_checked_info info;
        const gm_wall_add_info add = proc.addToWallMapChecked(pose, ap, &info);
        EXPECT(add.struct_size == sizeof(gm_wall_add_info) && add.gate == (float)prm.gate);
        // the check is still readable, with the same rows
        uint32_t count = 0;
        std::vector<gm_wall_check_point> again(changed.size() ? changed.size() : 1);
        EXPECT(gm_wall_map_get_check(proc.wallMap(), 0, 0, &again[0], (uint32_t)changed.size(), &count) == GM_OK && count == changed.size());
        EXPECT(changed.empty() || std::memcmp(&again[0], &changed[0], changed.size() * sizeof(gm_wall_check_point)) == 0);

        // the rule, one row at a time
        const PointCloud cloud = proc.choppedCloud();
        EXPECT(cloud.size() == fr.n_valid);
        const int64_t S = (int64_t)std::nearbyint(ap.min_delta * 1048576.0);
        std::vector<char> skip(cloud.size(), 0);
        gm_wall_add_checked_info want;
        std::memset(&want, 0, sizeof(want));
        for (size_t i = 0; i < changed.size(); ++i) {
            const int64_t dq = fix(changed[i].delta);
            if (dq == 0 || !std::isfinite(changed[i].delta) || changed[i].index >= cloud.size()) { ++want.rows_rejected; continue; }
            const bool sel = dq < 0 ? ((ap.skip & GM_WALL_SKIP_NEG) && -dq >= S) : ((ap.skip & GM_WALL_SKIP_POS) && dq >= S);
            if (!sel) { ++want.rows_kept; continue; }
            ++(dq < 0 ? want.rows_neg : want.rows_pos);
            skip[changed[i].index] = 1;
        }
        std::vector<float> xyz, all(3 * cloud.size());
        for (size_t i = 0; i < cloud.size(); ++i) {
            all[3 * i] = cloud[i].x; all[3 * i + 1] = cloud[i].y; all[3 * i + 2] = cloud[i].z;
            if (skip[i]) { ++want.skipped; continue; }
            xyz.push_back(cloud[i].x); xyz.push_back(cloud[i].y); xyz.push_back(cloud[i].z);
        }
        std::printf("%u points, %u rows: %u neg, %u pos, %u kept, %u rejected; %u skipped, %u mapped\n", info.n_points, info.n_rows,
                    info.rows_neg, info.rows_pos, info.rows_kept, info.rows_rejected, info.skipped, info.mapped);
        EXPECT(info.struct_size == sizeof(info) && info.min_delta_q == S && info.reserved == 0);
        EXPECT(info.n_points == cloud.size() && info.n_rows == changed.size());
        EXPECT(info.rows_neg == want.rows_neg && info.rows_pos == want.rows_pos && info.rows_kept == want.rows_kept &&
               info.rows_rejected == want.rows_rejected && info.skipped == want.skipped);
        EXPECT(info.rows_neg + info.rows_pos + info.rows_kept + info.rows_rejected == info.n_rows);
        EXPECT(info.skipped + info.plane + info.beyond_gate + info.outside + info.mapped == info.n_points);
        EXPECT(info.rows_pos > 100 && info.rows_kept > 100 && info.skipped == info.rows_neg + info.rows_pos);

        // the filtered plain add, and the stage call on the whole cloud and the rows
        EXPECT(gm_wall_map_add_points(plain, xyz.empty() ? 0 : &xyz[0], (uint32_t)(xyz.size() / 3), 0, pose, 0, 0, 0) == GM_OK);
        EXPECT(same_map(proc.wallMap(), plain));
        gm_wall_add_checked_info info2;
        std::vector<float> e(cloud.size());
        std::vector<int32_t> cell(cloud.size());
        EXPECT(gm_wall_map_add_points_checked(staged, &all[0], (uint32_t)cloud.size(), 0, pose, &ap, changed.empty() ? 0 : &changed[0],
                                              (uint32_t)changed.size(), 0, &info2, &e[0], &cell[0]) == GM_OK);
        EXPECT(std::memcmp(&info, &info2, sizeof(info)) == 0);
        EXPECT(same_map(proc.wallMap(), staged));
        for (size_t i = 0; i < cloud.size(); ++i)
            if (skip[i]) EXPECT(cell[i] == -1 && std::isfinite(e[i]));
        EXPECT(proc.wallMapInfo().frames == 1);

        // the stage call took slot 0: the frame is gone, and so is the check that belonged to it
        refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e2) { refused = e2.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e2) { refused = e2.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // a new frame, the old check
        proc.checkWallMap(pose, cp);
        ap.skip = 4;
        refused = false;
        try { proc.addToWallMapChecked(pose, ap); } catch (const Error &e2) { refused = e2.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        gm_wall_map_destroy(plain);
        gm_wall_map_destroy(staged);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_add_checked_test ok\n");
    return 0;
}
