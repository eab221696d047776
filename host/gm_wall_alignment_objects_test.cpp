// gm_wall_alignment_objects_test -- the host mirror's check objects on a wall alignment: Processor::createWallAlignment on
// straight - clothoid - arc, a survey of the alignment's own tube around the clothoid -> arc joint at 40 m, then a frame 1 m
// before the joint in which a strip of the wall lies 0.3 m inside the tube, through the mirror (processFrame,
// checkWallAlignment, wallAlignmentCheckObjects).  The strip runs through the joint plane and must come out as ONE object
// whose global station extents hold the joint; the info and the records are compared byte for byte with the C ABI's stage
// call (gm_wall_alignment_check_objects_rows) on the check's rows and plan, and the window with the host-only
// gm_wall_alignment_object_window.  Prints "gm_wall_alignment_objects_test ok" on success.
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
        EXPECT(sizeof(gm_wall_alignment_objects_info) == 136 && sizeof(struct gm_wall_alignment_object_metrics) == 112);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        cp.min_count = 2;
        gm_wall_object_params op;
        gm_wall_object_default_params(&op);
        op.block_stations = 3;   // (the joint at global station 160 lies inside a block row)
        op.block_sectors = 2;
        bool refused = false;
        try { proc.wallAlignmentCheckObjects(op); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.createWallAlignment(prm, el);
        refused = false;
        try { proc.wallAlignmentCheckObjects(op); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no check yet

        const unsigned n = 4000;
        unsigned long long seed = 11;
        double pose[12];
        std::vector<float> rows;
        for (int f = 0; f < 4; ++f) {   // the survey: the tube around the joint at 40 m
            frame(prm, el, 37.0 + 2.0 * f, n, 0, seed, pose, rows);
            std::vector<float> xyz(3 * (size_t)n);
            for (size_t i = 0; i < n; ++i) { xyz[3 * i] = rows[4 * i]; xyz[3 * i + 1] = rows[4 * i + 1]; xyz[3 * i + 2] = rows[4 * i + 2]; }
            EXPECT(gm_wall_alignment_add_points(proc.wallAlignment(), &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
        }
        std::vector<unsigned char> moved;
        frame(prm, el, 39.0, n, &moved, seed, pose, rows);
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        gm_wall_alignment_check_info ci;
        gm_wall_alignment_add_info plan;
        const std::vector<gm_wall_check_point> got = proc.checkWallAlignment(pose, cp, &ci, &plan);
        EXPECT(plan.n_sides == 2 && plan.side_element[0] == 1 && plan.side_element[1] == 2 && got.size() > 50);
        gm_wall_alignment_objects_info oi;
        const std::vector<gm_wall_object> objects = proc.wallAlignmentCheckObjects(op, &oi);
        EXPECT(oi.struct_size == sizeof(oi) && oi.n_rows == got.size() && oi.objects == objects.size() && oi.rejected == 0);
        EXPECT(oi.n_sides == 2 && oi.element == plan.element && oi.total == 240 && oi.side_first[0] == 80 && oi.side_first[1] == 160);
        EXPECT(oi.side_rows[0] == ci.side_class[0][GM_WALL_CHECK_CLS_CHANGED_NEG] + ci.side_class[0][GM_WALL_CHECK_CLS_CHANGED_POS]);
        EXPECT(oi.side_rows[1] == ci.side_class[1][GM_WALL_CHECK_CLS_CHANGED_NEG] + ci.side_class[1][GM_WALL_CHECK_CLS_CHANGED_POS]);
        EXPECT(oi.side_rows[0] > 10 && oi.side_rows[1] > 10 && oi.side_rows[0] + oi.side_rows[1] == got.size());
        EXPECT(oi.rejected + oi.outside_window + oi.sparse + oi.small + oi.in_object == oi.n_rows);

        // the stage call on the check's rows and plan, and the host-only window
        gm_wall_alignment_objects_info oj, ow;
        std::vector<gm_wall_object> want(objects.size() ? objects.size() : 1);
        std::vector<int32_t> of_row(got.size() ? got.size() : 1);
        uint32_t nw = 0;
        EXPECT(gm_wall_alignment_check_objects_rows(proc.wallAlignment(), &got[0], (uint32_t)got.size(), &plan, &op, &oj, &want[0],
                                                    (uint32_t)want.size(), &nw, &of_row[0]) == GM_OK);
        EXPECT(nw == objects.size() && std::memcmp(&oi, &oj, sizeof(oi)) == 0);
        EXPECT(objects.empty() || std::memcmp(&objects[0], &want[0], objects.size() * sizeof(gm_wall_object)) == 0);
        EXPECT(gm_wall_alignment_object_window(&prm, &el[0], ne, &plan, &op, &ow) == GM_OK);
        EXPECT(ow.station0 == oi.station0 && ow.n_stations == oi.n_stations && ow.blocks_stations == oi.blocks_stations &&
               ow.blocks_sectors == oi.blocks_sectors && ow.anchor_global == oi.anchor_global && ow.total == oi.total &&
               std::memcmp(ow.side_first, oi.side_first, sizeof(ow.side_first)) == 0 && ow.in_object == 0);

        // the strip is one object through the joint plane: the largest record holds most of the rows and station 160
        size_t big = 0;
        for (size_t i = 1; i < objects.size(); ++i)
            if (objects[i].points > objects[big].points) big = i;
        EXPECT(!objects.empty() && objects[big].sign == -1 && 2 * objects[big].points > got.size());
        EXPECT(!objects.empty() && objects[big].station_min < 160 && objects[big].station_max >= 160);
        uint32_t in_big = 0;
        for (size_t i = 0; i < got.size(); ++i) in_big += of_row[i] == (int32_t)big ? 1u : 0u;
        EXPECT(!objects.empty() && in_big == objects[big].points);
        if (!objects.empty()) {
            struct gm_wall_alignment_object_metrics m;
            EXPECT(gm_wall_alignment_object_metrics(&prm, &el[0], ne, &op, &objects[big], &m) == GM_OK);
            EXPECT(m.element_from == 1 && m.element_to == 2 && m.station_from == objects[big].station_min - 80 &&
                   m.station_to == objects[big].station_max - 160);
            EXPECT(m.chainage_from < 40.0 && m.chainage_to > 40.0 && m.mean_m < -0.2 && m.mean_m > -0.4);
            EXPECT(m.angle_from_deg >= 50.0 && m.angle_to_deg <= 90.0);   // the strip: 1.0 .. 1.4 rad
            std::printf("%zu rows (%u + %u), %zu objects; the strip: %llu points, stations %u .. %u, chainage %.2f .. %.2f, %.0f .. %.0f deg, mean %.3f m\n",
                        got.size(), oi.side_rows[0], oi.side_rows[1], objects.size(), (unsigned long long)objects[big].points,
                        objects[big].station_min, objects[big].station_max, m.chainage_from, m.chainage_to, m.angle_from_deg, m.angle_to_deg,
                        m.mean_m);
        }
        // a repeat with other parameters works on the same rows
        op.min_points = 1u << 20;
        EXPECT(proc.wallAlignmentCheckObjects(op, &oi).empty() && oi.small + oi.sparse + oi.outside_window == got.size());
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_objects_test ok\n");
    return 0;
}
