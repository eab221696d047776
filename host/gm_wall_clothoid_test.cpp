// gm_wall_clothoid_test -- the host mirror's wall map on a clothoid design axis: Processor::createWallMap(params, NULL,
// clothoid) on a transition from straight to an 80 m radius, then a short drive of three frames on the curved tube
// through the mirror (check, add), each compared byte for byte with the C ABI's stage calls on a second map of the same
// clothoid (gm_wall_map_create_clothoid, gm_wall_map_add_points, gm_wall_map_check_points), one cloud whose points are put
// back through gm_wall_clothoid_project, and the refusals of locateWallMap and alignWallMap.  Prints
// "gm_wall_clothoid_test ok" on success.
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

static const unsigned kN = 160, kNs = 90;

static std::vector<gm_wall_raw_cell> read_all(gm_wall_map *m)
{
    std::vector<gm_wall_raw_cell> raw((size_t)kN * kNs);
    uint64_t nc = 0;
    EXPECT(gm_wall_map_read_raw(m, 0, kN, &raw[0], raw.size(), &nc) == GM_OK && nc == raw.size());
    return raw;
}

// n points of the tube within 4.5 m of chainage s0 in the sensor coordinates of `pose`: rows of x, y, z, 0
static void tube(const gm_wall_params &prm, const gm_wall_clothoid &cl, const double pose[12], double s0, unsigned n, double strip,
                 unsigned long long &seed, std::vector<float> &rows)
{
    rows.assign(4 * (size_t)n, 0.0f);
    for (unsigned i = 0; i < n; ++i) {
        const double s = s0 - 4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
        const double rho = 2.0 + 0.02 * (uni(seed) - 0.5) + (phi < 1.0 ? strip : 0.0);
        double x[3];
        EXPECT(gm_wall_clothoid_point(&prm, &cl, s, phi, rho, x) == GM_OK);
        for (int c = 0; c < 3; ++c)   // Rm^T (x - tr)
            rows[4 * (size_t)i + c] = (float)(pose[c] * (x[0] - pose[3]) + pose[4 + c] * (x[1] - pose[7]) + pose[8 + c] * (x[2] - pose[11]));
    }
}

int main()
{
    try {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;   // 40 m
        prm.n_sectors = kNs;
        gm_wall_clothoid cl;
        std::memset(&cl, 0, sizeof(cl));
        cl.struct_size = sizeof(cl);
        cl.normal[1] = 0.6; cl.normal[2] = 0.8;   // an oblique plane of curvature
        cl.curvature = 0.0;
        cl.rate = 1.0 / (80.0 * 40.0);
        cl.point_chainage = 2.0;
        EXPECT(sizeof(gm_wall_clothoid) == 56 && sizeof(gm_wall_clothoid_add_info) == 128);
        EXPECT(gm_wall_clothoid_check_params(&prm, &cl) == GM_OK);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        gm_wall_clothoid flat = cl;
        flat.rate = 1.0e-9;
        try { proc.createWallMap(prm, 0, &flat); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused && !proc.wallMap());
        proc.createWallMap(prm, 0, &cl);
        gm_wall_clothoid got;
        gm_wall_arc got_arc;
        EXPECT(gm_wall_map_get_clothoid(proc.wallMap(), &got) == GM_OK && std::memcmp(&got, &cl, sizeof(cl)) == 0);
        EXPECT(gm_wall_map_get_arc(proc.wallMap(), &got_arc) == GM_OK && got_arc.curvature[1] == 0.0 && got_arc.curvature[2] == 0.0);
        gm_wall_map *abi = 0, *straight = 0;
        EXPECT(gm_wall_map_create_clothoid(proc.ctx(), &prm, &cl, &abi) == GM_OK && abi);
        EXPECT(gm_wall_map_create(proc.ctx(), &prm, &straight) == GM_OK);
        EXPECT(gm_wall_map_get_clothoid(straight, &got) == GM_OK && got.struct_size == 0 && got.rate == 0.0 && got.normal[1] == 0.0);

        const unsigned n = 20000;
        unsigned long long seed = 4711;
        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        cp.min_count = 2;
        cp.threshold = 0.04;
        double o[3], a[3], u[3], v[3], kappa, pose[12];
        std::vector<float> rows, survey4, survey;
        for (int f = 0; f < 3; ++f) {
            // the pose rides the axis at chainage 24.1 + 4 f: the section there as a sensor frame, 15 cm off
            const double s0 = 24.1 + 4.0 * f;
            EXPECT(gm_wall_clothoid_frame(&prm, &cl, s0, o, a, u, v, &kappa, 0) == GM_OK);
            EXPECT(std::fabs(kappa - cl.rate * (s0 - 2.0)) < 1e-15);
            for (int r = 0; r < 3; ++r) {
                pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
                pose[4 * r + 3] = o[r] + 0.15 * u[r] - 0.1 * v[r];
            }
            gm_wall_clothoid_add_info af;
            EXPECT(gm_wall_clothoid_add_frame(&prm, &cl, pose, &af) == GM_OK && af.anchor_station == 96 + 16 * f && af.struct_size == sizeof(af));
            EXPECT(std::fabs(af.sensor_chainage - s0) < 1e-9 && af.anchor_chainage == 24.0 + 4.0 * f);
            // the survey all maps start from: the tube without the strip, as a stage call; then the frame with the strip moved out
            tube(prm, cl, pose, s0, n, 0.0, seed, survey4);
            survey.resize(3 * (size_t)n);
            for (unsigned i = 0; i < n; ++i)
                for (int c = 0; c < 3; ++c) survey[3 * (size_t)i + c] = survey4[4 * (size_t)i + c];
            EXPECT(gm_wall_map_add_points(proc.wallMap(), &survey[0], n, 0, pose, 0, 0, 0) == GM_OK);
            EXPECT(gm_wall_map_add_points(abi, &survey[0], n, 0, pose, 0, 0, 0) == GM_OK);
            EXPECT(gm_wall_map_add_points(straight, &survey[0], n, 0, pose, 0, 0, 0) == GM_OK);
            tube(prm, cl, pose, s0, n, 0.1, seed, rows);

            const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
            EXPECT(fr.n_valid > n / 2);
            const PointCloud cloud = proc.choppedCloud();
            EXPECT(cloud.size() == fr.n_valid);
            std::vector<float> xyz(3 * cloud.size());
            for (size_t i = 0; i < cloud.size(); ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
            const uint32_t nv = (uint32_t)cloud.size();

            // one check: the mirror's frame path against the ABI's stage call on the other map (row = index there)
            gm_wall_check_info ci, ci2;
            const std::vector<gm_wall_check_point> rows_got = proc.checkWallMap(pose, cp, &ci);
            std::vector<gm_wall_check_point> staged(nv ? nv : 1);
            uint32_t count = 0;
            EXPECT(gm_wall_map_check_points(abi, &xyz[0], nv, 0, pose, &cp, 0, &ci2, &staged[0], nv, &count, 0, 0, 0, 0) == GM_OK);
            staged.resize(count);
            EXPECT(count == rows_got.size() && std::memcmp(&ci, &ci2, sizeof(ci)) == 0);
            for (size_t i = 0; i < staged.size() && i < rows_got.size(); ++i) {
                EXPECT(staged[i].row == staged[i].index);
                staged[i].row = rows_got[i].row;
            }
            EXPECT(rows_got.empty() || std::memcmp(&rows_got[0], &staged[0], rows_got.size() * sizeof(gm_wall_check_point)) == 0);
            std::printf("frame %d check: %u points, %u unchanged, %u changed+, %u changed-\n", f, ci.n_points, ci.unchanged, ci.changed_pos,
                        ci.changed_neg);
            EXPECT(ci.changed_pos > 1000 && ci.unchanged > 5000);

            // one add: the mirror's frame path against the ABI's stage call (the stage call above took slot 0: the frame again)
            EXPECT(proc.processFrame(&rows[0], n, 16, 0, 4, 8).n_valid == nv);
            const gm_wall_add_info ai = proc.addToWallMap(pose);
            gm_wall_add_info ai2;
            std::vector<float> e(nv ? nv : 1);
            EXPECT(gm_wall_map_add_points(abi, &xyz[0], nv, 0, pose, &ai2, &e[0], 0) == GM_OK);
            EXPECT(std::memcmp(&ai, &ai2, sizeof(ai)) == 0 && ai.anchor_station == af.anchor_station);
            EXPECT(std::memcmp(ai.o, af.o, 12) == 0 && std::memcmp(ai.a, af.a, 12) == 0);
            const std::vector<gm_wall_raw_cell> ra = read_all(proc.wallMap()), rb = read_all(abi);
            EXPECT(std::memcmp(&ra[0], &rb[0], ra.size() * sizeof(gm_wall_raw_cell)) == 0);
            float worst = 0.0f;
            for (uint32_t i = 0; i < nv; ++i) worst = std::fabs(e[i]) > worst ? std::fabs(e[i]) : worst;
            EXPECT(worst < 0.12f);   // every point lies within the strip's 10 cm + 1 cm of the design tube
        }
        EXPECT(proc.wallMapInfo().frames == 6);
        gm_wall_info wi, si;
        EXPECT(gm_wall_map_info(abi, &wi) == GM_OK && gm_wall_map_info(straight, &si) == GM_OK);
        std::printf("survey: clothoid map mapped %llu, straight map mapped %llu\n", (unsigned long long)wi.mapped,
                    (unsigned long long)si.mapped);
        EXPECT(si.mapped < wi.mapped / 2);   // (at 30 m the transition has left its tangent by rate t^3 / 6 = 1.1 m)

        // one cloud: the mirror against the ABI, and every point back through the clothoid's own projection
        gm_wall_cloud_params cc;
        gm_wall_cloud_default_params(&cc);
        cc.block_stations = 2; cc.block_sectors = 3; cc.min_count = 4;
        for (int c = 0; c < 3; ++c) cc.anchor[c] = o[c];
        gm_wall_cloud_info li, li2;
        const std::vector<gm_wall_cloud_point> pts = proc.wallMapCloud(80, 60, cc, &li);
        uint64_t np = 0;
        EXPECT(gm_wall_map_cloud(abi, 80, 60, &cc, &li2, 0, 0, &np) == GM_OK && np == pts.size());
        std::vector<gm_wall_cloud_point> direct(np ? np : 1);
        EXPECT(gm_wall_map_cloud(abi, 80, 60, &cc, &li2, &direct[0], np, &np) == GM_OK);
        EXPECT(std::memcmp(&li, &li2, sizeof(li)) == 0 && pts.size() > 500);
        EXPECT(pts.empty() || std::memcmp(&pts[0], &direct[0], pts.size() * sizeof(gm_wall_cloud_point)) == 0);
        double worst_s = 0.0, worst_e = 0.0;
        for (size_t i = 0; i < pts.size(); ++i) {
            const double x[3] = {pts[i].x + cc.anchor[0], pts[i].y + cc.anchor[1], pts[i].z + cc.anchor[2]};
            double s, phi, ee;
            EXPECT(gm_wall_clothoid_project(&prm, &cl, x, &s, &phi, &ee) == GM_OK);
            const unsigned J = pts[i].block / li.blocks_sectors;
            const double tc = prm.t_min + (80 + 2 * J + 1) * prm.station_length;   // whole blocks of 2 stations
            worst_s = std::fabs(s - tc) > worst_s ? std::fabs(s - tc) : worst_s;
            worst_e = std::fabs(ee - pts[i].mean) > worst_e ? std::fabs(ee - pts[i].mean) : worst_e;
        }
        std::printf("cloud: %zu points, worst |s - tc| %.2e m, worst |e - mean| %.2e m\n", pts.size(), worst_s, worst_e);
        EXPECT(worst_s <= 2e-6 && worst_e <= 2e-6);   // (fp32 coordinates of up to 10 m: half an ulp is 5e-7 m per axis)

        // locate and align are not available on a clothoid map
        gm_wall_locate_params lp;
        gm_wall_locate_default_params(&lp);
        gm_wall_align_params ap;
        gm_wall_align_default_params(&ap);
        proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        int unsupported = 0;
        try { proc.locateWallMap(pose, lp); } catch (const Error &e) { unsupported += e.status == GM_ERR_UNSUPPORTED; }
        try { proc.alignWallMap(pose, ap); } catch (const Error &e) { unsupported += e.status == GM_ERR_UNSUPPORTED; }
        EXPECT(unsupported == 2);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_clothoid_test ok\n");
    return 0;
}
