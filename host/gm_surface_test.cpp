// gm_surface_test -- the host mirror's wall deviation map: a Processor created with GM_CFG_SURFACE_MAP processes a
// synthetic tunnel whose wall is pushed out by 0.15 m over a patch of 4 x 6 default cells, then Processor::getSurfaceMap
// reads the map.  Checks the class counts, the cells against the patch and the undisturbed wall, and that
// setSurfaceParams applies to the next frame and refuses a grid above GM_SURF_MAX_CELLS.
// Prints "gm_surface_test ok" on success.  Usage: gm_surface_test [n_points]
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char **argv)
{
    const unsigned n = argc > 1 ? (unsigned)std::atoi(argv[1]) : 200000u;
    const double R = 2.0, pi = 3.14159265358979323846, floor_z = -1.2, dr = 0.15;
    // tunnel along x, 12 m long, +-0.01 m uniform radial noise, floor at z = -1.2; in the map's default frame
    // (u = +z, v = a x u = -y) the wall is pushed out by dr for t in [-2, -1), phi in [20, 44) degrees
    PointCloud cloud(n);
    unsigned long long s = 4242;
    for (unsigned i = 0; i < n; ++i) {
        const double t = -6.0 + 12.0 * uni(s), phi = 2.0 * pi * uni(s);
        double r = R + 0.02 * (uni(s) - 0.5);
        const double deg = phi * 180.0 / pi;
        if (t >= -2.0 && t < -1.0 && deg >= 20.0 && deg < 44.0) r += dr;
        double z = r * std::cos(phi);
        if (z < floor_z) z = floor_z + 0.02 * (uni(s) - 0.5);
        cloud[i].x = (float)t; cloud[i].y = (float)(-r * std::sin(phi)); cloud[i].z = (float)z; cloud[i].pad = 0.f;
    }
    try {
        Processor proc(5.0, 0.5, 0.25, 0.2, 0,
                       GM_CFG_VOXEL_GRID | GM_CFG_RANSAC_PLANE | GM_CFG_RANSAC_CYLINDER | GM_CFG_CYLINDER_FIT | GM_CFG_SURFACE_MAP);
        gm_surface_params prm;
        gm_surface_default_params(&prm);
        proc.setSurfaceParams(prm);
        const gm_frame_result res = proc.processFrame(&cloud[0], n, 16, 0, 4, 8);
        gm_surface_info info;
        std::vector<gm_surface_cell> cells;
        proc.getSurfaceMap(info, cells);
        EXPECT(info.struct_size == sizeof(gm_surface_info));
        EXPECT(info.status == GM_SURF_OK);
        EXPECT(info.n_stations == 40 && info.n_sectors == 90 && cells.size() == 3600);
        EXPECT(info.mapped + info.outside + info.beyond_gate + info.plane == res.n_valid);
        unsigned long long total = 0;
        unsigned hit = 0;
        for (size_t c = 0; c < cells.size(); ++c) {
            total += cells[c].count;
            hit += cells[c].count ? 1u : 0u;
            if (!cells[c].count) EXPECT(std::isnan(cells[c].mean));
            else EXPECT(cells[c].min <= cells[c].mean && cells[c].mean <= cells[c].max);
        }
        EXPECT(total == info.mapped && hit == info.cells_hit);
        EXPECT(info.a[0] > 0.999f && info.u[2] > 0.999f && info.v[1] < -0.999f);
        for (unsigned j = 12; j < 16; ++j)
            for (unsigned k = 5; k < 11; ++k) {
                const gm_surface_cell &c = cells[j * 90 + k];
                EXPECT(c.count > 10 && std::fabs(c.mean - dr) < 0.01);
            }
        for (unsigned j = 25; j < 35; ++j)        // undisturbed upper wall
            for (unsigned k = 80; k < 90; ++k) {
                const gm_surface_cell &c = cells[j * 90 + k];
                EXPECT(c.count > 10 && std::fabs(c.mean) < 0.01);
            }
        // the next frame uses new parameters; a grid above GM_SURF_MAX_CELLS is refused
        gm_surface_params one = prm;
        one.n_stations = 1; one.n_sectors = 1; one.station_length = 10.0;
        proc.setSurfaceParams(one);
        proc.processFrame(&cloud[0], n, 16, 0, 4, 8);
        gm_surface_info info1;
        proc.getSurfaceMap(info1, cells);
        EXPECT(cells.size() == 1 && info1.n_stations == 1 && cells[0].count == info1.mapped && info1.mapped > 0);
        gm_surface_params big = prm;
        big.n_stations = GM_SURF_MAX_CELLS + 1; big.n_sectors = 1;
        bool refused = false;
        try { proc.setSurfaceParams(big); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        std::printf("map: mapped=%u outside=%u beyond_gate=%u plane=%u cells_hit=%u R=%.5f\n", info.mapped, info.outside,
                    info.beyond_gate, info.plane, info.cells_hit, info.R);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_surface_test ok\n");
    return 0;
}
