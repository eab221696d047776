// gm_wall_locate_test -- the host mirror's wall-map locate: a synthetic tunnel frame on the design cylinder, seen from a
// sensor off the axis, goes through processFrame; Processor::locateWallMap, handed a pose that is 3 cm and 6 mrad off,
// is compared, byte for byte, with a direct gm_wall_map_locate_frame / gm_wall_map_get_locate call and with the stage
// call gm_wall_map_locate_points on the frame's /choppedCloud -- for both references, the MAP one against a survey added
// at the true pose -- and pass 0 with a scalar C++ restatement of the rule of include/gm_hip.h in double on the frame the
// pass reported.  The corrected pose must lie within 1 mm and 0.3 mrad of the true one and keep the caller's chainage.
// Prints "gm_wall_locate_test ok" on success.
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

static bool same(const gm_wall_locate_info &a, const gm_wall_locate_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// pass 0 of the DESIGN rule in double on the reported frame: the class counts and the step
static void restate(const PointCloud &cloud, const gm_wall_locate_pass &f, double R, unsigned &used, unsigned &gated, unsigned &near_gate,
                    double x[4])
{
    double A[4][4] = {{0}}, g[4] = {0, 0, 0, 0};
    used = gated = near_gate = 0;
    for (size_t i = 0; i < cloud.size(); ++i) {
        const double q[3] = {cloud[i].x - (double)f.o[0], cloud[i].y - (double)f.o[1], cloud[i].z - (double)f.o[2]};
        const double t = q[0] * f.a[0] + q[1] * f.a[1] + q[2] * f.a[2];
        const double w[3] = {q[0] - t * f.a[0], q[1] - t * f.a[1], q[2] - t * f.a[2]};
        const double rho = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double res = rho - R;
        if (std::fabs(std::fabs(res) - (double)f.gate) < 1e-5) ++near_gate;
        if (!(std::fabs(res) < (double)f.gate) || !(rho > 0.0)) { ++gated; continue; }
        ++used;
        const double a1 = -(w[0] * f.u[0] + w[1] * f.u[1] + w[2] * f.u[2]) / rho;
        const double a2 = -(w[0] * f.v[0] + w[1] * f.v[1] + w[2] * f.v[2]) / rho;
        const double J[4] = {a1, a2, t * a1, t * a2};
        for (int r = 0; r < 4; ++r) {
            for (int c = 0; c < 4; ++c) A[r][c] += J[r] * J[c];
            g[r] += J[r] * res;
        }
    }
    // Cholesky, as the device solves it
    for (int k = 0; k < 4; ++k) {
        double piv = A[k][k];
        for (int j = 0; j < k; ++j) piv -= A[k][j] * A[k][j];
        A[k][k] = std::sqrt(piv);
        for (int i = k + 1; i < 4; ++i) {
            double v = A[i][k];
            for (int j = 0; j < k; ++j) v -= A[i][j] * A[k][j];
            A[i][k] = v / A[k][k];
        }
    }
    double y[4];
    for (int i = 0; i < 4; ++i) {
        double v = -g[i];
        for (int j = 0; j < i; ++j) v -= A[i][j] * y[j];
        y[i] = v / A[i][i];
    }
    for (int i = 3; i >= 0; --i) {
        double v = y[i];
        for (int j = i + 1; j < 4; ++j) v -= A[j][i] * x[j];
        x[i] = v / A[i][i];
    }
}

int main()
{
    try {
        EXPECT(sizeof(gm_wall_locate_params) == 24 && sizeof(gm_wall_locate_pass) == 112 && sizeof(gm_wall_locate_info) == 488);
        gm_wall_locate_params lp;
        gm_wall_locate_default_params(&lp);
        EXPECT(lp.struct_size == sizeof(gm_wall_locate_params) && lp.reference == GM_WALL_LOCATE_DESIGN && lp.min_count == 8 &&
               lp.reserved == 0 && lp.gate == 0.25 && gm_wall_locate_check_params(&lp) == GM_OK);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = 80;
        prm.n_sectors = 90;
        prm.t_min = -10.0;
        // the true pose: the sensor 12.5 cm along, 6 cm and -3 cm off the axis, no rotation; the caller's: 3 cm and 6 mrad off
        const double truth[12] = {1, 0, 0, 0.125, 0, 1, 0, 0.0625, 0, 0, 1, -0.03125};
        const double cy = std::cos(0.006), sy = std::sin(0.006);
        const double pose[12] = {cy, -sy, 0, 0.125, sy, cy, 0, 0.0625 + 0.03, 0, 0, 1, -0.03125 - 0.02};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.locateWallMap(pose, lp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.locateWallMap(pose, lp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no frame yet

        // the frame: a tunnel of radius 2 on the design axis with 1 cm of noise, in the coordinates of the true sensor
        unsigned long long seed = 4711;
        const unsigned n = 20000;
        std::vector<float> rows(4 * n);
        for (unsigned i = 0; i < n; ++i) {
            const double t = -4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
            const double r = 2.0 + 0.02 * (uni(seed) - 0.5);
            rows[4 * i] = (float)(t - truth[3]); rows[4 * i + 1] = (float)(r * std::cos(phi) - truth[7]);
            rows[4 * i + 2] = (float)(r * std::sin(phi) - truth[11]);
            rows[4 * i + 3] = 0.0f;
        }
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        const PointCloud cloud = proc.choppedCloud();
        std::vector<float> xyz(3 * cloud.size());
        for (size_t i = 0; i < cloud.size(); ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
        // the survey: the same wall, added at the true pose (the stage call takes slot 0: the frame again behind it)
        EXPECT(gm_wall_map_add_points(proc.wallMap(), &xyz[0], (uint32_t)cloud.size(), 0, truth, 0, 0, 0) == GM_OK);
        proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        const gm_wall_info before = proc.wallMapInfo();

        for (int ref = 0; ref < 2; ++ref) {
            lp.reference = (uint32_t)ref;
            lp.min_count = 2;
            const gm_wall_locate_info got = proc.locateWallMap(pose, lp);
            gm_wall_locate_info direct, staged;
            EXPECT(gm_wall_map_locate_frame(proc.wallMap(), proc.ctx(), 0, pose, &lp) == GM_OK);
            EXPECT(gm_wall_map_get_locate(proc.wallMap(), 0, &direct) == GM_OK && same(got, direct));
            std::vector<float> res(cloud.size());
            std::vector<int32_t> cell(cloud.size());
            EXPECT(gm_wall_map_locate_points(proc.wallMap(), &xyz[0], (uint32_t)cloud.size(), 0, pose, &lp, &staged, &res[0], &cell[0]) == GM_OK);
            EXPECT(same(got, staged));
            EXPECT(got.struct_size == sizeof(got) && got.status == GM_LOCATE_OK && got.passes == 3 && got.n_points == cloud.size());
            unsigned used = 0, with_cell = 0;
            for (size_t i = 0; i < cloud.size(); ++i) { used += res[i] == res[i]; with_cell += cell[i] >= 0; }
            EXPECT(used == got.pass[2].used && (ref == GM_WALL_LOCATE_MAP ? with_cell > cloud.size() / 2 : with_cell == 0));
            for (int k = 0; k < 3; ++k) {
                const gm_wall_locate_pass &q = got.pass[k];
                EXPECT(q.plane + q.outside + q.unsurveyed + q.gated + q.used == got.n_points && q.gate == (float)(0.25 / (1 << k)));
            }
            // the corrected pose against the true one: lateral offset, axis angle, chainage
            const double dy = got.pose[7] - truth[7], dz = got.pose[11] - truth[11];
            const double ax = got.pose[0], ay = got.pose[1], az = got.pose[2];   // Rm'^T a for a = (1, 0, 0): row 0
            const double ang = std::atan2(std::sqrt(ay * ay + az * az), ax);
            std::printf("reference %d: used %u %u %u, lateral %.2e m, angle %.2e rad, chainage %.1e, lateral (%.4f, %.4f) tilt (%.5f, %.5f)\n",
                        ref, got.pass[0].used, got.pass[1].used, got.pass[2].used, std::sqrt(dy * dy + dz * dz), ang, got.pose[3] - pose[3],
                        got.lateral[0], got.lateral[1], got.tilt[0], got.tilt[1]);
            EXPECT(std::sqrt(dy * dy + dz * dz) < 1e-3 && ang < 3e-4 && std::fabs(got.pose[3] - pose[3]) <= 1e-9);
            if (ref == GM_WALL_LOCATE_DESIGN) {
                unsigned u0 = 0, g0 = 0, near_gate = 0;
                double x[4];
                restate(cloud, got.pass[0], (double)(float)prm.radius, u0, g0, near_gate, x);
                EXPECT(u0 + near_gate >= got.pass[0].used && got.pass[0].used + near_gate >= u0 && g0 + u0 == got.n_points);
                if (near_gate == 0)
                    for (int k = 0; k < 4; ++k) EXPECT(std::fabs(x[k] - got.pass[0].step[k]) <= 1e-6);
            }
            proc.processFrame(&rows[0], n, 16, 0, 4, 8);   // the frame path needs a frame again
        }
        // the map was not changed
        const gm_wall_info after = proc.wallMapInfo();
        EXPECT(std::memcmp(&before, &after, sizeof(before)) == 0 && after.frames == 1);
        lp.gate = 9.0;
        refused = false;
        try { proc.locateWallMap(pose, lp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_locate_test ok\n");
    return 0;
}
