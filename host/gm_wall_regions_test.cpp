// gm_wall_regions_test -- the host mirror's deviation regions: a Processor drives through a synthetic straight tunnel
// whose wall carries three world-fixed patches (two pushed out by 0.15 m, one pushed in), adds every frame to the wall
// map under its pose, and asks Processor::wallMapRegions for the regions above 0.075 m.  Checks that exactly the three
// patches come back, ascending by label, with their sign, cells, extents and metrics (gm_wall_region_metrics), the
// counts of the call, a sub-window that cuts a patch, and the refusals.
// Prints "gm_wall_regions_test ok" on success.  Usage: gm_wall_regions_test [n_points_per_frame]
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

static const double kPi = 3.14159265358979323846, kR = 2.0;
static const int kFrames = 12;
// world-fixed patches on 0.25 m x 4 degree cells: chainage [t0, t1), angle [p0, p1) degrees (u = +z, v = -y), dr
struct Patch { double t0, t1, p0, p1, dr; unsigned j0, j1, k0, k1; };
static const Patch kPatches[3] = {{10.0, 12.0, 20.0, 44.0, 0.15, 40, 47, 5, 10},
                                  {25.0, 27.0, 316.0, 340.0, -0.15, 100, 107, 79, 84},
                                  {33.0, 34.0, 100.0, 140.0, 0.15, 132, 135, 25, 34}};

// frame f: sensor at chainage 6 + 3 f, 0.1 m off the axis, yawed by +-3 degrees; the wall within 6 m of it
static void make_frame(int f, unsigned n, PointCloud &cloud, double pose[12])
{
    const double s0 = 6.0 + 3.0 * f, yaw = (f % 2 ? 3.0 : -3.0) * kPi / 180.0, c = std::cos(yaw), s = std::sin(yaw);
    const double Rm[3][3] = {{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}}, tr[3] = {s0, 0.1, -0.1};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) pose[4 * r + k] = Rm[r][k];
        pose[4 * r + 3] = tr[r];
    }
    cloud.resize(n);
    unsigned long long seed = 777 + 131 * (unsigned long long)f;
    for (unsigned i = 0; i < n; ++i) {
        const double t = s0 - 6.0 + 12.0 * uni(seed), phi = 2.0 * kPi * uni(seed), deg = phi * 180.0 / kPi;
        double r = kR + 0.02 * (uni(seed) - 0.5);
        for (int p = 0; p < 3; ++p)
            if (t >= kPatches[p].t0 && t < kPatches[p].t1 && deg >= kPatches[p].p0 && deg < kPatches[p].p1) r += kPatches[p].dr;
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
        prm.n_stations = 208;   // 52 m
        prm.radius = kR;
        gm_wall_region_params rp;
        gm_wall_region_default_params(&rp);
        EXPECT(rp.struct_size == sizeof(gm_wall_region_params) && rp.min_count == 8 && rp.min_cells == 4 && rp.connectivity == 8);
        rp.threshold = 0.075;
        rp.min_count = 1;

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.wallMapRegions(0, 208, rp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        EXPECT(proc.wallMapRegions(0, 208, rp).empty());   // an empty map has no regions
        PointCloud cloud;
        double pose[12];
        for (int f = 0; f < kFrames; ++f) {
            make_frame(f, n, cloud, pose);
            proc.processFrame(&cloud[0], n, 16, 0, 4, 8);
            proc.addToWallMap(pose);
        }
        gm_wall_regions_info info;
        const std::vector<gm_wall_region> reg = proc.wallMapRegions(0, 208, rp, &info);
        EXPECT(info.struct_size == sizeof(gm_wall_regions_info) && info.n_stations == 208 && info.n_sectors == 90);
        EXPECT(info.threshold_q == 78643 && info.regions == 3 && info.flagged_pos == 88 && info.flagged_neg == 48);
        EXPECT(reg.size() == 3);
        const double cell_area = 0.25 * kR * 2.0 * kPi / 90.0;
        EXPECT(std::fabs(info.cell_area - cell_area) < 1e-15);
        for (size_t i = 0; i < reg.size() && i < 3; ++i) {
            const gm_wall_region &r = reg[i];
            const Patch &p = kPatches[i];
            const unsigned cells = (p.j1 - p.j0 + 1) * (p.k1 - p.k0 + 1);
            EXPECT(r.label == p.j0 * 90 + p.k0 && r.sign == (p.dr > 0 ? 1 : -1) && r.cells == cells);
            EXPECT(r.station_min == p.j0 && r.station_max == p.j1 && r.sector_min == p.k0 && r.sector_max == p.k1);
            EXPECT(r.points > 10ull * cells);
            struct gm_wall_region_metrics m;
            EXPECT(gm_wall_region_metrics(&prm, &r, &m) == GM_OK);
            EXPECT(std::fabs(m.mean_m - p.dr) < 0.005 && std::fabs(m.peak_m) >= std::fabs(m.mean_m));
            EXPECT(std::fabs(m.area_m2 - cells * cell_area) < 1e-12 && std::fabs(m.volume_m3 - m.mean_m * m.area_m2) < 1e-12);
            EXPECT(m.chainage_from == p.t0 && m.chainage_to == p.t1 && m.angle_from_deg == p.p0 && m.angle_to_deg == p.p1);
            std::printf("region %u: sign %d cells %u stations %u-%u sectors %u-%u mean %.4f m volume %.4f m3\n", r.label, r.sign,
                        r.cells, r.station_min, r.station_max, r.sector_min, r.sector_max, m.mean_m, m.volume_m3);
        }
        // a window that cuts the first patch at station 44 and ends behind the second (stations 44-107): labels and extents
        // stay map-wide
        const std::vector<gm_wall_region> cut = proc.wallMapRegions(44, 64, rp, &info);
        EXPECT(cut.size() == 2 && info.station0 == 44 && info.n_stations == 64);
        if (cut.size() == 2) {
            EXPECT(cut[0].label == 44 * 90 + 5 && cut[0].cells == 24 && cut[0].station_min == 44 && cut[0].station_max == 47);
            EXPECT(cut[1].label == 100 * 90 + 79 && cut[1].cells == 48);
        }
        refused = false;
        try { proc.wallMapRegions(207, 2, rp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        rp.connectivity = 6;
        refused = false;
        try { proc.wallMapRegions(0, 208, rp); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_regions_test ok\n");
    return 0;
}
