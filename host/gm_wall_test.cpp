// gm_wall_test -- the host mirror's persistent wall map: a Processor drives through a synthetic straight tunnel whose
// wall is pushed out by 0.15 m over a world-fixed patch, adding every frame under its pose with Processor::addToWallMap
// (blocking frames first, then the same frames submitted without blocking with the add right behind each submit), and
// reads the map with readWallMap.  Checks the totals, the patch, the undisturbed wall, the overlap of neighbouring
// frames, that chainages nobody saw stay empty, that both passes give the same cells, and the refusals.
// Prints "gm_wall_test ok" on success.  Usage: gm_wall_test [n_points_per_frame]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gm_tunnel_processing.hpp"

using namespace gm_host;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
    } while (0)

// deterministic uniform [0, 1) (64-bit LCG, top 53 bits)
static double uni(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
}

static const double kPi = 3.14159265358979323846, kR = 2.0, kDr = 0.15;
static const int kFrames = 6;

// frame f: sensor at chainage 6 + 3 f, 0.1 m off the axis, yawed by +-3 degrees; the wall within 6 m of it in SENSOR
// coordinates.  World-fixed patch: t in [10, 11), phi in [20, 44) degrees (u = +z, v = -y), pushed out by kDr.
static void make_frame(int f, unsigned n, PointCloud &cloud, double pose[12])
{
    const double s0 = 6.0 + 3.0 * f, yaw = (f % 2 ? 3.0 : -3.0) * kPi / 180.0, c = std::cos(yaw), s = std::sin(yaw);
    const double Rm[3][3] = {{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}}, tr[3] = {s0, 0.1, -0.1};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) pose[4 * r + k] = Rm[r][k];
        pose[4 * r + 3] = tr[r];
    }
    cloud.resize(n);
    unsigned long long seed = 4242 + 977 * (unsigned long long)f;
    for (unsigned i = 0; i < n; ++i) {
        const double t = s0 - 6.0 + 12.0 * uni(seed), phi = 2.0 * kPi * uni(seed), deg = phi * 180.0 / kPi;
        double r = kR + 0.02 * (uni(seed) - 0.5);
        if (t >= 10.0 && t < 11.0 && deg >= 20.0 && deg < 44.0) r += kDr;
        const double w[3] = {t - tr[0], -r * std::sin(phi) - tr[1], r * std::cos(phi) - tr[2]};
        cloud[i].x = (float)(Rm[0][0] * w[0] + Rm[1][0] * w[1] + Rm[2][0] * w[2]);   // Rm^T (p - tr)
        cloud[i].y = (float)(Rm[0][1] * w[0] + Rm[1][1] * w[1] + Rm[2][1] * w[2]);
        cloud[i].z = (float)(Rm[0][2] * w[0] + Rm[1][2] * w[1] + Rm[2][2] * w[2]);
        cloud[i].pad = 0.f;
    }
}

int main(int argc, char **argv)
{
    const unsigned n = argc > 1 ? (unsigned)std::atoi(argv[1]) : 200000u;
    try {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = 160;   // 40 m
        prm.radius = kR;
        std::vector<PointCloud> clouds(kFrames);
        double poses[kFrames][12];
        for (int f = 0; f < kFrames; ++f) make_frame(f, n, clouds[f], poses[f]);

        // blocking frames
        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.addToWallMap(poses[0]); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.addToWallMap(poses[0]); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no frame yet
        unsigned long long n_valid = 0;
        for (int f = 0; f < kFrames; ++f) {
            const gm_frame_result res = proc.processFrame(&clouds[f][0], n, 16, 0, 4, 8);
            n_valid += res.n_valid;
            const gm_wall_add_info ai = proc.addToWallMap(poses[f]);
            EXPECT(ai.struct_size == sizeof(gm_wall_add_info) && ai.anchor_station == (int64_t)std::floor((6.0 + 3.0 * f) / 0.25));
            EXPECT(ai.a[0] > 0.99f && std::fabs(ai.R - 2.0f) == 0.0f);
        }
        const gm_wall_info info = proc.wallMapInfo();
        EXPECT(info.struct_size == sizeof(gm_wall_info) && info.status == GM_SURF_OK);
        EXPECT(info.frames == (uint64_t)kFrames && info.n_stations == 160 && info.n_sectors == 90);
        EXPECT(info.mapped + info.outside + info.beyond_gate + info.plane == n_valid);
        EXPECT(info.mapped > n_valid * 9 / 10 && info.plane == 0);
        std::vector<gm_surface_cell> cells;
        proc.readWallMap(0, 160, cells);
        EXPECT(cells.size() == 160u * 90u);
        unsigned long long total = 0, hit = 0;
        for (size_t c = 0; c < cells.size(); ++c) {
            total += cells[c].count;
            hit += cells[c].count ? 1u : 0u;
            if (!cells[c].count) EXPECT(std::isnan(cells[c].mean) && std::isnan(cells[c].min) && std::isnan(cells[c].max));
            else EXPECT(cells[c].min <= cells[c].max && std::fabs(cells[c].mean) <= 0.25f);
        }
        EXPECT(total == info.mapped && hit == info.cells_hit);
        for (unsigned j = 40; j < 44; ++j)          // the patch: t in [10, 11), 20..44 degrees
            for (unsigned k = 5; k < 11; ++k) {
                const gm_surface_cell &c = cells[j * 90 + k];
                EXPECT(c.count > 10 && std::fabs(c.mean - kDr) < 0.01);
            }
        for (unsigned j = 48; j < 80; ++j)          // undisturbed wall, seen by two or three frames
            for (unsigned k = 60; k < 70; ++k) {
                const gm_surface_cell &c = cells[j * 90 + k];
                EXPECT(c.count > 10 && std::fabs(c.mean) < 0.01);
            }
        for (unsigned j = 120; j < 160; ++j)        // beyond the last frame's crop box (21 + 5 m, yawed): nobody saw it
            for (unsigned k = 0; k < 90; ++k) EXPECT(cells[j * 90 + k].count == 0);
        // a window, and a window that leaves the map
        std::vector<gm_surface_cell> win;
        proc.readWallMap(40, 4, win);
        EXPECT(win.size() == 4u * 90u && std::memcmp(&win[0], &cells[40 * 90], win.size() * sizeof(gm_surface_cell)) == 0);
        refused = false;
        try { proc.readWallMap(159, 2, win); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        double bad[12];
        std::memcpy(bad, poses[0], sizeof(bad));
        bad[0] *= 1.01;
        refused = false;
        try { proc.addToWallMap(bad); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);

        // the same frames submitted without blocking, the add right behind each submit: the same cells
        Processor stream(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        stream.createWallMap(prm);
        for (int f = 0; f < kFrames; ++f) {
            stream.submitFrame(&clouds[f][0], n, 16, 0, 4, 8);
            stream.addToWallMap(poses[f]);
            stream.waitFrame();
        }
        std::vector<gm_surface_cell> again;
        stream.readWallMap(0, 160, again);
        EXPECT(again.size() == cells.size() && std::memcmp(&again[0], &cells[0], cells.size() * sizeof(gm_surface_cell)) == 0);
        EXPECT(stream.wallMapInfo().mapped == info.mapped);
        std::printf("map: frames=%llu mapped=%llu outside=%llu beyond_gate=%llu cells_hit=%llu\n",
                    (unsigned long long)info.frames, (unsigned long long)info.mapped, (unsigned long long)info.outside,
                    (unsigned long long)info.beyond_gate, (unsigned long long)info.cells_hit);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_test ok\n");
    return 0;
}
