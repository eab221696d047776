// gm_wall_align_test -- the host mirror's wall-map align: a synthetic tunnel frame on a textured wall goes through
// processFrame; Processor::alignWallMap, handed a pose that is 2 stations and 1 sector short of the true one, is compared,
// byte for byte, with a direct gm_wall_map_align_frame / gm_wall_map_get_align call and with the stage call
// gm_wall_map_align_points on the frame's /choppedCloud, against a survey of the same wall (other noise) added at the true
// pose; the host-only gm_wall_align_select on the returned table must reproduce the selection and the pose.  The shift
// found must be (2, 1) with the flags clear and the aligned pose within half a cell of the true one, laterally unchanged.
// Prints "gm_wall_align_test ok" on success.
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

// the wall in map coordinates: radius 2, bumps of a few centimetres that repeat neither within the station search
// (periods of 3.0 m and 1.9 m) nor within the sector search (120 and 72 degrees), 5 mm of noise
static void wall_point(unsigned long long &seed, double out[3])
{
    const double t = -4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
    const double r = 2.0 + 0.03 * std::sin(2.1 * t) * std::cos(3.0 * phi) + 0.02 * std::cos(3.3 * t + 1.0) * std::sin(5.0 * phi) +
                     0.01 * (uni(seed) - 0.5);
    out[0] = t; out[1] = r * std::cos(phi); out[2] = r * std::sin(phi);
}

static bool same(const gm_wall_align_info &a, const gm_wall_align_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
static bool same(const std::vector<gm_wall_align_score> &a, const std::vector<gm_wall_align_score> &b)
{
    return a.size() == b.size() && std::memcmp(&a[0], &b[0], a.size() * sizeof(a[0])) == 0;
}

int main()
{
    try {
        EXPECT(sizeof(gm_wall_align_params) == 56 && sizeof(gm_wall_align_score) == 24 && sizeof(gm_wall_align_info) == 224);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = 80;
        prm.n_sectors = 32;
        prm.t_min = -10.0;
        gm_wall_align_params ap;
        gm_wall_align_default_params(&ap);
        EXPECT(ap.struct_size == sizeof(ap) && ap.half_patch_stations == 20 && ap.max_station_shift == 8 && ap.max_sector_shift == 4 &&
               ap.min_count == 8 && ap.min_frame_count == 4 && ap.min_overlap == 64 && ap.reserved == 0 && ap.gate == 0.25 &&
               ap.clip == 0.05 && ap.min_distinction == 1.5 && gm_wall_align_check_params(&ap, prm.n_sectors) == GM_OK);
        ap.half_patch_stations = 16;
        ap.max_station_shift = 4;
        EXPECT(gm_wall_align_check_params(&ap, prm.n_sectors) == GM_OK && gm_wall_align_check_params(&ap, 8) == GM_ERR_INVALID_ARG);
        // the true pose: the sensor 12.5 cm along, 6 cm and -3 cm off the axis, no rotation.  The caller's: 2 stations and
        // 1 sector short of it (turned about the axis through the origin, then moved back along it).
        const double ds = prm.station_length, dth = 6.283185307179586 / prm.n_sectors;
        const double truth[12] = {1, 0, 0, 0.125, 0, 1, 0, 0.0625, 0, 0, 1, -0.03125};
        const double c = std::cos(-dth), s = std::sin(-dth);
        const double pose[12] = {1, 0, 0, truth[3] - 2 * ds, 0, c, -s, c * truth[7] - s * truth[11], 0, s, c, s * truth[7] + c * truth[11]};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.alignWallMap(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.alignWallMap(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no frame yet

        // the survey: the wall seen from the true pose, added there
        unsigned long long seed = 4711;
        const unsigned n = 20000;
        std::vector<float> survey(3 * (size_t)(2 * n));
        for (unsigned i = 0; i < 2 * n; ++i) {
            double w[3];
            wall_point(seed, w);
            for (int k = 0; k < 3; ++k) survey[3 * i + k] = (float)(w[k] - truth[4 * k + 3]);
        }
        EXPECT(gm_wall_map_add_points(proc.wallMap(), &survey[0], 2 * n, 0, truth, 0, 0, 0) == GM_OK);
        // the frame: other points of the same wall, in the coordinates of the true sensor
        std::vector<float> rows(4 * (size_t)n);
        for (unsigned i = 0; i < n; ++i) {
            double w[3];
            wall_point(seed, w);
            for (int k = 0; k < 3; ++k) rows[4 * i + k] = (float)(w[k] - truth[4 * k + 3]);
            rows[4 * i + 3] = 0.0f;
        }
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        const PointCloud cloud = proc.choppedCloud();
        std::vector<float> xyz(3 * cloud.size());
        for (size_t i = 0; i < cloud.size(); ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
        const gm_wall_info before = proc.wallMapInfo();

        std::vector<gm_wall_align_score> table, direct_table, staged_table;
        const gm_wall_align_info got = proc.alignWallMap(pose, ap, &table);
        const uint32_t shifts = (2 * ap.max_station_shift + 1) * (2 * ap.max_sector_shift + 1);
        EXPECT(table.size() == shifts);
        gm_wall_align_info direct, staged, selected;
        gm_wall_add_info add;
        uint32_t n_out = 0;
        EXPECT(gm_wall_map_align_frame(proc.wallMap(), proc.ctx(), 0, pose, &ap, &add) == GM_OK);
        EXPECT(gm_wall_map_get_align(proc.wallMap(), 0, 0, 0, 0, &n_out) == GM_OK && n_out == shifts);
        direct_table.resize(n_out);
        EXPECT(gm_wall_map_get_align(proc.wallMap(), 0, &direct, &direct_table[0], n_out, &n_out) == GM_OK);
        EXPECT(same(got, direct) && same(table, direct_table) && add.anchor_station == got.anchor_station && add.gate == 0.25f);
        EXPECT(gm_wall_map_get_align(proc.wallMap(), 0, &direct, &direct_table[0], n_out - 1, &n_out) == GM_ERR_CAPACITY);
        std::vector<float> res(cloud.size());
        std::vector<int32_t> cell(cloud.size());
        staged_table.resize(shifts);
        EXPECT(gm_wall_map_align_points(proc.wallMap(), &xyz[0], (uint32_t)cloud.size(), 0, pose, &ap, 0, &staged, &staged_table[0],
                                        shifts, &n_out, &res[0], &cell[0]) == GM_OK);
        EXPECT(same(got, staged) && same(table, staged_table) && n_out == shifts);
        unsigned binned = 0;
        for (size_t i = 0; i < cloud.size(); ++i) {
            binned += cell[i] >= 0;
            EXPECT(cell[i] < (int32_t)(2 * ap.half_patch_stations * prm.n_sectors) && res[i] == res[i]);   // (no plane points here)
        }
        EXPECT(got.struct_size == sizeof(got) && got.n_points == cloud.size() && binned == got.binned && got.plane == 0 &&
               got.plane + got.beyond_gate + got.outside_patch + got.binned == got.n_points);
        EXPECT(got.half_patch_stations == 16 && got.max_station_shift == 4 && got.max_sector_shift == 4);
        // the host-only selection on the table: the same result but for the device's counts
        EXPECT(gm_wall_align_select(&prm, &ap, pose, &table[0], shifts, &selected) == GM_OK);
        EXPECT(selected.n_points == 0 && selected.binned == 0 && selected.patch_cells_usable == 0);
        selected.n_points = got.n_points; selected.plane = got.plane; selected.beyond_gate = got.beyond_gate;
        selected.outside_patch = got.outside_patch; selected.binned = got.binned; selected.patch_cells_usable = got.patch_cells_usable;
        EXPECT(same(got, selected));
        EXPECT(gm_wall_align_select(&prm, &ap, pose, &table[0], shifts - 1, &selected) == GM_ERR_INVALID_ARG);
        // the shift, and the aligned pose against the true one
        const double along = (got.pose[3] - truth[3]) / ds;
        const double turn = std::atan2(got.pose[9], got.pose[5]) / dth;   // Rm' = Rx(turn): the true one is the identity
        const double dy = got.pose[7] - truth[7], dz = got.pose[11] - truth[11];
        std::printf("best (%d, %d) + (%.3f, %.3f), overlap %u, distinction %.2f, rms %.4f / %.4f, pose off by %.3f stations, %.3f sectors\n",
                    got.best_station, got.best_sector, got.frac_station, got.frac_sector, got.overlap, got.distinction, got.rms_best,
                    got.rms_runner, along, turn);
        EXPECT(got.status == GM_ALIGN_OK && got.best_station == 2 && got.best_sector == 1 && got.overlap >= ap.min_overlap);
        EXPECT(std::fabs(along) < 0.5 && std::fabs(turn) < 0.5 && std::sqrt(dy * dy + dz * dz) < 0.5 * dth * 0.07);
        EXPECT(got.distinction >= ap.min_distinction && got.rms_best < got.rms_runner);
        // the map was not changed
        const gm_wall_info after = proc.wallMapInfo();
        EXPECT(std::memcmp(&before, &after, sizeof(before)) == 0 && after.frames == 1);
        proc.processFrame(&rows[0], n, 16, 0, 4, 8);   // the stage call took slot 0: the frame path needs a frame again
        ap.clip = 9.0;
        refused = false;
        try { proc.alignWallMap(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_align_test ok\n");
    return 0;
}
