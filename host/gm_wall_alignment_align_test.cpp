// gm_wall_alignment_align_test -- the host mirror's align on a wall alignment: Processor::createWallAlignment on
// straight - clothoid - arc, a survey of a bumpy wall around the clothoid -> arc joint, then frames 1 m before and after
// the joint through the mirror (processFrame, alignWallAlignment) under a pose two stations short.  The info and the score
// table are compared byte for byte with the C ABI's stage call (gm_wall_alignment_align_points) on the frame's valid cloud
// against a second alignment that holds the same survey, and the shift must be the two stations.  Prints
// "gm_wall_alignment_align_test ok" on success.
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

static gm_wall_element element(uint32_t kind, uint32_t n, double curvature, double rate)
{
    gm_wall_element e;
    std::memset(&e, 0, sizeof(e));
    e.struct_size = sizeof(e);
    e.kind = kind;
    e.n_stations = n;
    e.turn[1] = -1.0;
    e.curvature = curvature;
    e.rate = rate;
    return e;
}

// the wall's relief at (chainage, angle): bumps of a few centimetres that no two stations share
static double relief(double s, double phi)
{
    return 0.03 * std::sin(2.3 * s + 0.7 * std::sin(1.1 * s)) * std::cos(3.0 * phi + 0.9 * s) + 0.02 * std::sin(5.1 * s) * std::sin(2.0 * phi);
}

// the pose of a sensor at chainage s_pose (0.15 m up, 0.1 m aside) and n points of the wall around s_wall in the
// coordinates of a sensor at s_wall
static void frame(const gm_wall_params &prm, const std::vector<gm_wall_element> &el, double s_wall, double s_pose, unsigned n,
                  unsigned long long &seed, double pose[12], std::vector<float> &rows)
{
    const uint32_t ne = (uint32_t)el.size();
    double at[2][12];
    for (int q = 0; q < 2; ++q) {
        const double s0 = q ? s_pose : s_wall;
        double P[3], pu[3], pv[3], u[3], v[3], a[3];
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 0.0, P) == GM_OK);
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 1.0, pu) == GM_OK);
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 1.5707963267948966, 1.0, pv) == GM_OK);
        for (int c = 0; c < 3; ++c) { u[c] = pu[c] - P[c]; v[c] = pv[c] - P[c]; }
        a[0] = u[1] * v[2] - u[2] * v[1]; a[1] = u[2] * v[0] - u[0] * v[2]; a[2] = u[0] * v[1] - u[1] * v[0];
        for (int r = 0; r < 3; ++r) {
            at[q][4 * r] = a[r]; at[q][4 * r + 1] = -v[r]; at[q][4 * r + 2] = u[r];
            at[q][4 * r + 3] = P[r] + 0.15 * u[r] - 0.1 * v[r];
        }
    }
    std::memcpy(pose, at[1], sizeof(at[1]));
    const double *t = at[0];
    rows.assign(4 * (size_t)n, 0.0f);
    for (unsigned i = 0; i < n; ++i) {
        const double s = s_wall - 4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
        const double rho = 2.0 + relief(s, phi) + 0.004 * (uni(seed) - 0.5);
        double x[3];
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, phi, rho, x) == GM_OK);
        for (int c = 0; c < 3; ++c)   // Rm^T (x - tr) of the sensor at s_wall
            rows[4 * (size_t)i + c] = (float)(t[c] * (x[0] - t[3]) + t[4 + c] * (x[1] - t[7]) + t[8 + c] * (x[2] - t[11]));
    }
}

int main()
{
    try {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        const double K = 1.0 / 80.0;
        std::vector<gm_wall_element> el;
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, 0.0, K / 20.0));
        el.push_back(element(GM_WALL_ELEMENT_ARC, 80, K, 0.0));
        const uint32_t ne = (uint32_t)el.size();
        EXPECT(sizeof(gm_wall_alignment_align_info) == 472 && sizeof(gm_wall_alignment_align_plan_info) == 336);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        gm_wall_align_params ap;
        gm_wall_align_default_params(&ap);
        ap.half_patch_stations = 18;
        ap.min_count = 2;
        ap.min_frame_count = 1;
        EXPECT(gm_wall_align_check_params(&ap, prm.n_sectors) == GM_OK);
        double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        bool refused = false;
        try { proc.alignWallAlignment(eye, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.createWallAlignment(prm, el);
        refused = false;
        try { proc.alignWallAlignment(eye, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no frame yet
        gm_wall_alignment *abi = 0;
        EXPECT(gm_wall_alignment_create(proc.ctx(), &prm, &el[0], ne, &abi) == GM_OK && abi);

        const unsigned n = 8000;
        unsigned long long seed = 7;
        double pose[12];
        std::vector<float> rows;
        // the survey: the wall around the joint at 40 m, into both alignments
        for (int f = 0; f < 9; ++f) {
            const double s = 36.0 + 1.0 * f;
            frame(prm, el, s, s, n, seed, pose, rows);
            std::vector<float> xyz(3 * (size_t)n);
            for (size_t i = 0; i < n; ++i) { xyz[3 * i] = rows[4 * i]; xyz[3 * i + 1] = rows[4 * i + 1]; xyz[3 * i + 2] = rows[4 * i + 2]; }
            EXPECT(gm_wall_alignment_add_points(proc.wallAlignment(), &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
            EXPECT(gm_wall_alignment_add_points(abi, &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
        }
        const uint32_t nsh = (2u * ap.max_station_shift + 1u) * (2u * ap.max_sector_shift + 1u);
        for (int f = 0; f < 2; ++f) {
            const double s = f ? 41.0 : 39.0;
            frame(prm, el, s, s - 2.0 * prm.station_length, n, seed, pose, rows);   // the caller's pose is two stations short
            const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
            EXPECT(fr.n_valid > n / 2);
            const PointCloud cloud = proc.choppedCloud();
            const uint32_t nv = (uint32_t)cloud.size();
            std::vector<float> xyz(3 * (size_t)nv);
            for (size_t i = 0; i < nv; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
            // (the frame's align first: the stage call below takes the context's slot 0 for its own cloud)
            std::vector<gm_wall_align_score> got;
            gm_wall_alignment_align_plan_info plan;
            const gm_wall_alignment_align_info gi = proc.alignWallAlignment(pose, ap, &got, &plan);
            gm_wall_alignment_align_info wi;
            gm_wall_alignment_align_plan_info wplan;
            std::vector<gm_wall_align_score> want(nsh);
            uint32_t nw = 0;
            EXPECT(gm_wall_alignment_align_points(abi, &xyz[0], nv, 0, pose, &ap, &wplan, &wi, &want[0], nsh, &nw, 0, 0, 0) == GM_OK);
            EXPECT(nw == nsh && got.size() == nsh && std::memcmp(&got[0], &want[0], nsh * sizeof(want[0])) == 0);
            EXPECT(gi.struct_size == sizeof(gi) && std::memcmp(&gi, &wi, sizeof(gi)) == 0);
            EXPECT(std::memcmp(&plan, &wplan, sizeof(plan)) == 0 && plan.add.n_sides == 2 && plan.own == 0 && plan.n_pieces >= 2);
            EXPECT(plan.add.side_element[0] == 1 && plan.add.side_element[1] == 2 && gi.n_sides == 2 && gi.n_points == nv);
            EXPECT(gi.side_class[0][3] > 100 && gi.side_class[1][3] > 100 && gi.binned == gi.side_class[0][3] + gi.side_class[1][3]);
            EXPECT(!(gi.status & GM_ALIGN_FAILED_MASK) && gi.best_station == 2 && gi.best_sector == 0);
            // the aligned pose is the pose at s: two stations further along the curve
            double truth[12];
            std::vector<float> none;
            unsigned long long s2 = 1;
            frame(prm, el, s, s, 0, s2, truth, none);
            double worst = 0.0;
            for (int k = 0; k < 12; ++k) worst = std::fmax(worst, std::fabs(gi.pose[k] - truth[k]));
            EXPECT(worst < 0.5 * prm.station_length);   // (half a station: the fraction's own error is far below)
            std::printf("frame %d: %u valid, binned %u + %u, best (%d, %d) + (%.3f, %.3f), distinction %.2f, |pose - truth| %.4f\n", f, nv,
                        gi.side_class[0][3], gi.side_class[1][3], gi.best_station, gi.best_sector, gi.frac_station, gi.frac_sector,
                        gi.distinction, worst);
        }
        gm_wall_alignment_destroy(abi);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_align_test ok\n");
    return 0;
}
