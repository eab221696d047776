// gm_wall_alignment_check_test -- the host mirror's check and checked add on a wall alignment: Processor::createWallAlignment
// on straight - clothoid - arc, a survey of the alignment's own tube around the clothoid -> arc joint, then frames 1 m before
// and after the joint, a strip of the wall moved 0.3 m inward, through the mirror (processFrame, checkWallAlignment,
// addToWallAlignmentChecked).  The check's info and rows are compared byte for byte with the C ABI's stage call
// (gm_wall_alignment_check_points) on the frame's valid cloud, and the element maps after the checked add with those of a
// second alignment fed gm_wall_alignment_add_points_checked.  Prints "gm_wall_alignment_check_test ok" on success.
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

// the pose of a sensor at chainage s0 (0.15 m up, 0.1 m aside) and n points of the tube around it, in sensor coordinates;
// with `moved`, the strip of the wall at angles 1.0 .. 1.4 rad lies 0.3 m inside the tube over the whole frame (a patch,
// not single points: a lone point has no neighbours and does not reach the valid cloud) and moved[i] says so of point i
static void frame(const gm_wall_params &prm, const std::vector<gm_wall_element> &el, double s0, unsigned n, std::vector<unsigned char> *moved,
                  unsigned long long &seed, double pose[12], std::vector<float> &rows)
{
    const uint32_t ne = (uint32_t)el.size();
    double P[3], pu[3], pv[3], u[3], v[3], a[3];
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 0.0, P) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 1.0, pu) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 1.5707963267948966, 1.0, pv) == GM_OK);
    for (int c = 0; c < 3; ++c) { u[c] = pu[c] - P[c]; v[c] = pv[c] - P[c]; }
    a[0] = u[1] * v[2] - u[2] * v[1]; a[1] = u[2] * v[0] - u[0] * v[2]; a[2] = u[0] * v[1] - u[1] * v[0];
    for (int r = 0; r < 3; ++r) {
        pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
        pose[4 * r + 3] = P[r] + 0.15 * u[r] - 0.1 * v[r];
    }
    rows.assign(4 * (size_t)n, 0.0f);
    if (moved) moved->assign(n, 0);
    for (unsigned i = 0; i < n; ++i) {
        const double s = s0 - 4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
        const bool in = moved && phi >= 1.0 && phi < 1.4;
        if (in) (*moved)[i] = 1;
        const double rho = 2.0 + 0.01 * (uni(seed) - 0.5) - (in ? 0.3 : 0.0);
        double x[3];
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, phi, rho, x) == GM_OK);
        for (int c = 0; c < 3; ++c)   // Rm^T (x - tr)
            rows[4 * (size_t)i + c] = (float)(pose[c] * (x[0] - pose[3]) + pose[4 + c] * (x[1] - pose[7]) + pose[8 + c] * (x[2] - pose[11]));
    }
}

static bool same_maps(gm_wall_alignment *p, gm_wall_alignment *q, uint32_t ne, const gm_wall_params &prm, const std::vector<gm_wall_element> &el)
{
    bool same = gm_wall_alignment_sync(p) == GM_OK && gm_wall_alignment_sync(q) == GM_OK;
    for (uint32_t i = 0; i < ne && same; ++i) {
        gm_wall_map *mp = 0, *mq = 0;
        same = gm_wall_alignment_map(p, i, &mp) == GM_OK && gm_wall_alignment_map(q, i, &mq) == GM_OK;
        const size_t cells = (size_t)el[i].n_stations * prm.n_sectors;
        std::vector<gm_wall_raw_cell> a(cells), b(cells);
        same = same && gm_wall_map_read_raw(mp, 0, el[i].n_stations, &a[0], cells, 0) == GM_OK &&
               gm_wall_map_read_raw(mq, 0, el[i].n_stations, &b[0], cells, 0) == GM_OK && std::memcmp(&a[0], &b[0], cells * sizeof(a[0])) == 0;
        gm_wall_info ia, ib;
        same = same && gm_wall_map_info(mp, &ia) == GM_OK && gm_wall_map_info(mq, &ib) == GM_OK && ia.mapped == ib.mapped &&
               ia.outside == ib.outside && ia.beyond_gate == ib.beyond_gate && ia.plane == ib.plane && ia.frames == ib.frames;
    }
    return same;
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
        EXPECT(sizeof(gm_wall_alignment_check_info) == 184);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        cp.min_count = 2;
        gm_wall_add_checked_params ap;
        gm_wall_add_checked_default_params(&ap);
        double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        bool refused = false;
        try { proc.checkWallAlignment(eye, cp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        refused = false;
        try { proc.addToWallAlignmentChecked(eye, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.createWallAlignment(prm, el);
        gm_wall_alignment *abi = 0;
        EXPECT(gm_wall_alignment_create(proc.ctx(), &prm, &el[0], ne, &abi) == GM_OK && abi);

        const unsigned n = 4000;
        unsigned long long seed = 7;
        double pose[12];
        std::vector<float> rows;
        // the survey: the tube around the joint at 40 m, into both alignments
        for (int f = 0; f < 4; ++f) {
            frame(prm, el, 37.0 + 2.0 * f, n, 0, seed, pose, rows);
            std::vector<float> xyz(3 * (size_t)n);
            for (size_t i = 0; i < n; ++i) { xyz[3 * i] = rows[4 * i]; xyz[3 * i + 1] = rows[4 * i + 1]; xyz[3 * i + 2] = rows[4 * i + 2]; }
            EXPECT(gm_wall_alignment_add_points(proc.wallAlignment(), &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
            EXPECT(gm_wall_alignment_add_points(abi, &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
        }
        for (int f = 0; f < 2; ++f) {
            std::vector<unsigned char> moved;
            frame(prm, el, f ? 41.0 : 39.0, n, &moved, seed, pose, rows);
            const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
            EXPECT(fr.n_valid > n / 2);
            const PointCloud cloud = proc.choppedCloud();
            const uint32_t nv = (uint32_t)cloud.size();
            std::vector<float> xyz(3 * (size_t)nv);
            for (size_t i = 0; i < nv; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
            // (the frame's check and checked add first: the stage calls below take the context's slot 0 for their own cloud)
            refused = false;
            try { proc.addToWallAlignmentChecked(pose, ap); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
            EXPECT(refused);   // no check of this frame yet
            gm_wall_alignment_check_info ci;
            gm_wall_alignment_add_info plan;
            const std::vector<gm_wall_check_point> got = proc.checkWallAlignment(pose, cp, &ci, &plan);
            gm_wall_add_checked_info ai;
            const gm_wall_alignment_add_info aplan = proc.addToWallAlignmentChecked(pose, ap, &ai);
            EXPECT(std::memcmp(&plan, &aplan, sizeof(plan)) == 0 && plan.n_sides == 2 && plan.side_element[0] == 1 && plan.side_element[1] == 2);

            gm_wall_alignment_check_info cj;
            std::vector<gm_wall_check_point> want(nv ? nv : 1);
            uint32_t nw = 0;
            std::vector<float> res(nv ? nv : 1);
            EXPECT(gm_wall_alignment_check_points(abi, &xyz[0], nv, 0, pose, &cp, 0, &cj, &want[0], nv, &nw, &res[0], 0, 0, 0, 0) == GM_OK);
            uint32_t moved_valid = 0;   // the strip's points that reached the valid cloud (the wall's own noise is 5 mm)
            for (size_t i = 0; i < nv; ++i) moved_valid += res[i] < -0.2f ? 1u : 0u;
            EXPECT(ci.struct_size == sizeof(ci) && std::memcmp(&ci, &cj, sizeof(ci)) == 0);
            EXPECT(nw == got.size() && ci.n_points == nv && ci.n_sides == 2);
            uint32_t per_side[2] = {0, 0};
            for (size_t i = 0; i < got.size() && i < nw; ++i) {
                gm_wall_check_point a = got[i], b = want[i];
                a.row = b.row = 0;   // (the frame's rows carry the input row, the stage call's the index)
                EXPECT(std::memcmp(&a, &b, sizeof(a)) == 0);
                EXPECT(got[i].row < n && moved[got[i].row] && GM_WALL_ROW_SIDE(got[i].cell) < 2 && GM_WALL_ROW_CELL(got[i].cell) < 80u * prm.n_sectors);
                ++per_side[GM_WALL_ROW_SIDE(got[i].cell) & 1u];
            }
            // every changed point lies in the strip; the strip's points are changed unless their cell holds fewer than two
            // survey points (16 000 survey points over some 5 400 cells: about one cell in five)
            EXPECT(ci.changed_pos == 0 && ci.changed_neg == got.size() && got.size() <= moved_valid && 2 * got.size() > moved_valid);
            EXPECT(moved_valid > 100 && per_side[0] > 10 && per_side[1] > 10);
            EXPECT(ci.side_class[0][GM_WALL_CHECK_CLS_CHANGED_NEG] == per_side[0] && ci.side_class[1][GM_WALL_CHECK_CLS_CHANGED_NEG] == per_side[1]);
            EXPECT(ai.struct_size == sizeof(ai) && ai.skipped == got.size() && ai.n_rows == got.size() && ai.n_points == nv);
            gm_wall_add_checked_info aj;
            EXPECT(gm_wall_alignment_add_points_checked(abi, &xyz[0], nv, 0, pose, &ap, got.empty() ? 0 : &got[0], (uint32_t)got.size(), 0, &aj, 0,
                                                        0, 0) == GM_OK);
            EXPECT(std::memcmp(&ai, &aj, sizeof(ai)) == 0);
            EXPECT(same_maps(proc.wallAlignment(), abi, ne, prm, el));
            std::printf("frame %d: %u valid, %u of them moved, %zu changed (%u + %u), skipped %u\n", f, nv, moved_valid, got.size(), per_side[0],
                        per_side[1], ai.skipped);
        }
        gm_wall_alignment_destroy(abi);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_check_test ok\n");
    return 0;
}
