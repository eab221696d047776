// gm_wall_alignment_host_test -- the device-free calls of the wall alignment (gm_wall_alignment_check, _element_params,
// _project, _point, _window, _add_plan, _object_window, _object_metrics) as a stand-alone program: linked with gm_wall_host.hip and
// gm_wall_alignment_host.hip alone and built with AddressSanitizer and UBSan by tests/test_host_wall_alignment.py.
// Prints "gm_wall_alignment_host_test ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/gm_hip.h"

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
    } while (0)

static gm_wall_element element(uint32_t kind, uint32_t n, double curvature, double rate)
{
    gm_wall_element e;
    std::memset(&e, 0, sizeof(e));
    e.struct_size = sizeof(e);
    e.kind = kind;
    e.n_stations = n;
    e.turn[1] = -2.0;   // +y under the default up; normalised by the library
    e.curvature = curvature;
    e.rate = rate;
    return e;
}

int main()
{
    gm_wall_params prm;
    gm_wall_default_params(&prm);
    prm.n_stations = 0;   // not read
    const double K = 1.0 / 80.0, Lc = 12.0;
    std::vector<gm_wall_element> el;
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 40, 0.0, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 48, 0.0, K / Lc));
    el.push_back(element(GM_WALL_ELEMENT_ARC, 40, K, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 48, K, -K / Lc));
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 40, 0.0, 0.0));
    const uint32_t n = (uint32_t)el.size();
    EXPECT(sizeof(gm_wall_element) == 48 && sizeof(gm_wall_alignment_add_info) == 160 && sizeof(gm_wall_alignment_totals) == 72);
    EXPECT(gm_wall_alignment_check(&prm, &el[0], n) == GM_OK);
    EXPECT(gm_wall_alignment_check(&prm, &el[0], 0) == GM_ERR_INVALID_ARG && gm_wall_alignment_check(0, &el[0], n) == GM_ERR_INVALID_ARG);
    std::vector<gm_wall_element> many(GM_WALL_ALIGNMENT_MAX_ELEMENTS + 1, el[0]);
    EXPECT(gm_wall_alignment_check(&prm, &many[0], GM_WALL_ALIGNMENT_MAX_ELEMENTS) == GM_OK);
    EXPECT(gm_wall_alignment_check(&prm, &many[0], GM_WALL_ALIGNMENT_MAX_ELEMENTS + 1) == GM_ERR_INVALID_ARG);
    gm_wall_element bad = el[2];
    bad.kind = 3;
    EXPECT(gm_wall_alignment_check(&prm, &bad, 1) == GM_ERR_INVALID_ARG);

    // the derived structs: element i + 1 starts at element i's end frame
    for (uint32_t i = 0; i < n; ++i) {
        gm_wall_params p;
        gm_wall_arc arc;
        gm_wall_clothoid cl;
        EXPECT(gm_wall_alignment_element_params(&prm, &el[0], n, i, &p, &arc, &cl) == GM_OK);
        EXPECT(p.n_stations == el[i].n_stations && (arc.struct_size != 0) == (el[i].kind == GM_WALL_ELEMENT_ARC) &&
               (cl.struct_size != 0) == (el[i].kind == GM_WALL_ELEMENT_CLOTHOID));
        if (i + 1 < n && el[i].kind != GM_WALL_ELEMENT_STRAIGHT) {
            gm_wall_params q;
            EXPECT(gm_wall_alignment_element_params(&prm, &el[0], n, i + 1, &q, 0, 0) == GM_OK);
            double o[3], a[3], u[3], v[3], kappa;
            const double s_end = p.t_min + p.n_stations * p.station_length;
            if (el[i].kind == GM_WALL_ELEMENT_ARC) EXPECT(gm_wall_arc_frame(&p, &arc, s_end, o, a, u, v) == GM_OK);
            else EXPECT(gm_wall_clothoid_frame(&p, &cl, s_end, o, a, u, v, &kappa, 0) == GM_OK);
            EXPECT(std::memcmp(q.point, o, 24) == 0 && std::memcmp(q.direction, a, 24) == 0 && std::memcmp(q.up, u, 24) == 0);
        }
    }
    EXPECT(gm_wall_alignment_element_params(&prm, &el[0], n, n, &prm, 0, 0) == GM_ERR_INVALID_ARG);

    // project(point) across every joint
    double worst = 0.0;
    unsigned seen[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 2000; ++k) {
        const double s = 0.01 + 53.98 * k / 1999.0, phi = 6.28 * ((k * 37) % 100) / 100.0, rho = 2.0 + 0.1 * std::sin(0.3 * k);
        double x[3], s2, phi2, e2;
        uint32_t who = 99;
        EXPECT(gm_wall_alignment_point(&prm, &el[0], n, s, phi, rho, x) == GM_OK);
        EXPECT(gm_wall_alignment_project(&prm, &el[0], n, x, &who, &s2, &phi2, &e2) == GM_OK && who < n);
        if (who < n) ++seen[who];
        double dphi = std::fabs(phi2 - phi);
        dphi = dphi > 3.14159 ? 6.283185307179586 - dphi : dphi;
        worst = std::fmax(worst, std::fmax(std::fabs(s2 - s), std::fmax(std::fabs(e2 - (rho - 2.0)), dphi * rho)));
    }
    std::printf("round trip: worst %.2e\n", worst);
    EXPECT(worst <= 1e-9 && seen[0] > 100 && seen[1] > 100 && seen[2] > 100 && seen[3] > 100 && seen[4] > 100);

    // the window: pieces, the count query, capacity
    gm_wall_alignment_piece pc[8];
    uint32_t got = 0;
    EXPECT(gm_wall_alignment_window(&prm, &el[0], n, 8.1, 33.3, 0, 0, &got) == GM_ERR_CAPACITY && got == 4);
    EXPECT(gm_wall_alignment_window(&prm, &el[0], n, 8.1, 33.3, pc, 2, &got) == GM_ERR_CAPACITY && got == 4);
    EXPECT(gm_wall_alignment_window(&prm, &el[0], n, 8.1, 33.3, pc, 8, &got) == GM_OK && got == 4);
    EXPECT(pc[0].element == 0 && pc[0].station0 == 32 && pc[0].n_stations == 8 && pc[3].element == 3 && pc[3].station0 == 0 &&
           pc[3].n_stations == 6 && pc[1].n_stations == 48 && pc[2].n_stations == 40);
    EXPECT(gm_wall_alignment_window(&prm, &el[0], n, 2.0, 1.0, pc, 8, &got) == GM_ERR_INVALID_ARG);

    // the plan of an add 1 m before the first joint, and a reach that meets every element
    double pose[12] = {1, 0, 0, 9.0, 0, 1, 0, 0.1, 0, 0, 1, -0.1};
    gm_wall_alignment_add_info info;
    EXPECT(gm_wall_alignment_add_plan(&prm, &el[0], n, pose, 1.0, &info) == GM_OK);
    EXPECT(info.struct_size == sizeof(info) && info.element == 0 && info.n_sides == 2 && info.side_element[1] == 1 &&
           info.side_anchor[0] == 36 && info.side_anchor[1] == -4 && std::fabs(info.chainage - 9.0) < 1e-12);
    EXPECT(info.joint_o[0][0] == 1.0f && info.joint_o[0][1] == -0.1f && info.joint_a[0][0] == 1.0f);
    EXPECT(gm_wall_alignment_add_plan(&prm, &el[0], n, pose, 5.0, &info) == GM_OK && info.n_sides == 3);
    pose[3] = 27.0;
    EXPECT(gm_wall_alignment_add_plan(&prm, &el[0], n, pose, 9.0, &info) == GM_ERR_UNSUPPORTED);
    pose[0] = 2.0;
    EXPECT(gm_wall_alignment_add_plan(&prm, &el[0], n, pose, 5.0, &info) == GM_ERR_INVALID_ARG);
    // the object window and metrics on the global station grid (bases 0, 40, 88, 128, 176; total 216), anchors at the
    // ends of int64 included
    pose[0] = 1.0; pose[3] = 9.0;
    EXPECT(gm_wall_alignment_add_plan(&prm, &el[0], n, pose, 1.0, &info) == GM_OK && info.n_sides == 2);
    gm_wall_object_params op;
    gm_wall_object_default_params(&op);
    op.block_stations = 3;
    op.half_window_stations = 10;
    gm_wall_alignment_objects_info oi;
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, &info, &op, &oi) == GM_OK);
    EXPECT(oi.struct_size == sizeof(oi) && oi.anchor_global == 36 && oi.total == 216 && oi.side_first[0] == 0 && oi.side_first[1] == 40 &&
           oi.station0 == 24 && oi.n_stations == 24 && oi.blocks_stations == 8 && oi.n_sides == 2 && oi.in_object == 0);
    gm_wall_alignment_add_info far = info;
    far.element = 1;
    far.side_anchor[1] = INT64_MAX;
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, &far, &op, &oi) == GM_OK && oi.blocks_stations == 0 && oi.anchor_global == INT64_MAX);
    far.side_anchor[1] = INT64_MIN;
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, &far, &op, &oi) == GM_OK && oi.blocks_stations == 0);
    far.side_anchor[1] = 175;   // G_f = 215, the last station
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, &far, &op, &oi) == GM_OK && oi.station0 + oi.n_stations == 216);
    far.side_element[1] = 2;
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, &far, &op, &oi) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_object_window(&prm, &el[0], n, 0, &op, &oi) == GM_ERR_INVALID_ARG);
    gm_wall_object rec;
    std::memset(&rec, 0, sizeof(rec));
    rec.points = 3; rec.station_min = 39; rec.station_max = 88; rec.sector_max = 2; rec.sector_max_turned = prm.n_sectors / 2 + 2;
    rec.sector_min_turned = prm.n_sectors / 2;
    struct gm_wall_alignment_object_metrics om;
    EXPECT(gm_wall_alignment_object_metrics(&prm, &el[0], n, &op, &rec, &om) == GM_OK);
    EXPECT(om.element_from == 0 && om.station_from == 39 && om.element_to == 2 && om.station_to == 0 &&
           om.chainage_from == prm.t_min + 39.0 * prm.station_length && om.chainage_to == prm.t_min + 89.0 * prm.station_length);
    rec.station_max = 216;
    EXPECT(gm_wall_alignment_object_metrics(&prm, &el[0], n, &op, &rec, &om) == GM_ERR_INVALID_ARG);
    // an alignment that turns 143 degrees: a point beyond the arc lies behind the first joint's plane and is element 2's
    std::vector<gm_wall_element> turn;
    turn.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    turn.push_back(element(GM_WALL_ELEMENT_ARC, 800, K, 0.0));
    turn.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 400, 0.0, 0.0));
    EXPECT(gm_wall_alignment_check(&prm, &turn[0], 3) == GM_OK);
    double xt[3], st, pt, et;
    uint32_t wt = 99;
    EXPECT(gm_wall_alignment_point(&prm, &turn[0], 3, 310.0, 1.0, 2.1, xt) == GM_OK);
    EXPECT(gm_wall_alignment_project(&prm, &turn[0], 3, xt, &wt, &st, &pt, &et) == GM_OK);
    EXPECT(wt == 2 && std::fabs(st - 310.0) < 1e-9 && std::fabs(et - 0.1) < 1e-9 && std::fabs(pt - 1.0) < 1e-9);
    double pose2[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    EXPECT(gm_wall_alignment_point(&prm, &turn[0], 3, 310.0, 0.0, 0.0, xt) == GM_OK);
    pose2[3] = xt[0]; pose2[7] = xt[1]; pose2[11] = xt[2];
    EXPECT(gm_wall_alignment_add_plan(&prm, &turn[0], 3, pose2, 5.0, &info) == GM_OK);
    EXPECT(info.element == 2 && info.n_sides == 1 && info.side_element[0] == 2 && std::fabs(info.chainage - 310.0) < 1e-9);
    if (fails) return 1;
    std::printf("gm_wall_alignment_host_test ok\n");
    return 0;
}
