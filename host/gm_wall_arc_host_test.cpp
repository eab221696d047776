// gm_wall_arc_host_test -- the device-free entries of the wall map on a circular-arc design axis (gm_wall_arc_*,
// csrc/gm_wall_host.hip) as a stand-alone program: linked with that one source file, it initialises no device, so it can
// run under the host sanitizers (tests/test_host_wall_arc_pure.py builds it that way).  The frame at a chainage is
// orthonormal and lies on the axis, point and project are inverse to 1e-9 m, the per-add frame anchors at the sensor's
// station, and every refusal of the rule is refused.  Prints "gm_wall_arc_host_test ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/gm_hip.h"

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
    } while (0)

static double dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

static gm_wall_arc arc_of(double cx, double cy, double cz, double s0)
{
    gm_wall_arc a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.curvature[0] = cx; a.curvature[1] = cy; a.curvature[2] = cz;
    a.point_chainage = s0;
    return a;
}

int main()
{
    gm_wall_params p;
    gm_wall_default_params(&p);
    p.n_stations = 480;
    p.t_min = -20.0;
    p.point[0] = 3.0; p.point[1] = -2.0; p.point[2] = 1.0;
    p.direction[0] = 1.0; p.direction[1] = 0.05; p.direction[2] = 0.02;
    const gm_wall_arc arc = arc_of(0.004, 0.006, 0.008, 12.5);   // its component along the axis is dropped
    EXPECT(gm_wall_arc_check_params(&p, &arc) == GM_OK);

    double o[3], a[3], u[3], v[3];
    for (int k = 0; k <= 10; ++k) {
        const double s = p.t_min + 0.1 * k * p.n_stations * p.station_length;
        EXPECT(gm_wall_arc_frame(&p, &arc, s, o, a, u, v) == GM_OK);
        EXPECT(std::fabs(dot(a, a) - 1.0) < 1e-14 && std::fabs(dot(u, u) - 1.0) < 1e-14 && std::fabs(dot(v, v) - 1.0) < 1e-14);
        EXPECT(std::fabs(dot(a, u)) < 1e-14 && std::fabs(dot(a, v)) < 1e-14 && std::fabs(dot(u, v)) < 1e-14);
        double sp, phi, e;
        EXPECT(gm_wall_arc_project(&p, &arc, o, &sp, &phi, &e) == GM_OK && std::fabs(sp - s) < 1e-9 && std::fabs(e + p.radius) < 1e-9);
        // point and project are inverse
        for (int j = 0; j < 16; ++j) {
            const double ang = 0.39 * j + 0.01, rho = p.radius + 0.02 * (j - 8);
            double x[3];
            EXPECT(gm_wall_arc_point(&p, &arc, s, ang, rho, x) == GM_OK);
            EXPECT(gm_wall_arc_project(&p, &arc, x, &sp, &phi, &e) == GM_OK);
            EXPECT(std::fabs(sp - s) < 1e-9 && std::fabs(e - (rho - p.radius)) < 1e-9 && std::fabs(phi - ang) * rho < 1e-9);
        }
        // the per-add frame of a sensor riding the axis there
        double pose[12];
        for (int r = 0; r < 3; ++r) {
            pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
            pose[4 * r + 3] = o[r] + 0.2 * u[r] - 0.1 * v[r];
        }
        if (k == 10) continue;   // (the map's far end: the sensor's station is n_stations)
        gm_wall_arc_add_info f;
        EXPECT(gm_wall_arc_add_frame(&p, &arc, pose, &f) == GM_OK && f.struct_size == sizeof(f) && f.reserved == 0);
        EXPECT(std::fabs(f.sensor_chainage - s) < 1e-9 && f.anchor_chainage <= f.sensor_chainage + 1e-9 &&
               f.sensor_chainage < f.anchor_chainage + p.station_length + 1e-9);
        EXPECT(f.anchor_chainage == p.t_min + (double)f.anchor_station * p.station_length);
        // in sensor coordinates the section at the anchor is the sensor's own frame up to the turn within one station
        EXPECT(std::fabs(f.a[0] - 1.0f) < 1e-4f && std::fabs(f.a[1]) < 1e-2f && std::fabs(f.a[2]) < 1e-2f);
        EXPECT(std::fabs(f.o[0]) <= (float)p.station_length + 1e-3f && std::fabs(f.o[1] + 0.1f) < 1e-3f && std::fabs(f.o[2] + 0.2f) < 1e-3f);
        EXPECT(std::fabs(f.kappa - 0.01f) < 5e-4f && std::fabs(f.un * f.un + f.ub * f.ub - 1.0f) < 1e-6f);
    }

    // refusals
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    gm_wall_params q;
    gm_wall_default_params(&q);
    q.n_stations = 40;
    gm_wall_arc t = arc_of(0.0, 1.0 / 80.0, 0.0, 0.0);
    EXPECT(gm_wall_arc_check_params(&q, &t) == GM_OK);
    t = arc_of(0.0, 1.0 / 1.1e6, 0.0, 0.0);  EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = arc_of(0.0, 1.0 / 4.4, 0.0, 0.0);    EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = arc_of(0.0, 1.0 / 3.0, 0.0, 0.0);    EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);   // 10 m of map: psi > 3
    t = arc_of(0.0, nan, 0.0, 0.0);          EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = arc_of(0.0, 0.01, 0.0, inf);         EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = arc_of(0.5, 0.0, 0.0, 0.0);          EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = arc_of(0.0, 1.0 / 80.0, 0.0, 0.0);
    t.struct_size = 32;
    EXPECT(gm_wall_arc_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t.struct_size = sizeof(t);
    EXPECT(gm_wall_arc_check_params(0, &t) == GM_ERR_INVALID_ARG && gm_wall_arc_check_params(&q, 0) == GM_ERR_INVALID_ARG);
    double x[3] = {0.0, 0.0, 2.0}, sp, phi, e;
    EXPECT(gm_wall_arc_frame(&q, &t, nan, o, a, u, v) == GM_ERR_INVALID_ARG && gm_wall_arc_frame(&q, &t, 1.0, 0, a, u, v) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_arc_project(&q, &t, 0, &sp, &phi, &e) == GM_ERR_INVALID_ARG && gm_wall_arc_project(&q, &t, x, 0, &phi, &e) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_arc_point(&q, &t, 1.0, inf, 2.0, x) == GM_ERR_INVALID_ARG && gm_wall_arc_point(&q, &t, 1.0, 0.0, 2.0, 0) == GM_ERR_INVALID_ARG);
    gm_wall_arc_add_info f;
    double bad[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0};   // a reflection
    EXPECT(gm_wall_arc_add_frame(&q, &t, bad, &f) == GM_ERR_INVALID_ARG && gm_wall_arc_add_frame(&q, &t, 0, &f) == GM_ERR_INVALID_ARG);
    bad[10] = 1.0;
    EXPECT(gm_wall_arc_add_frame(&q, &t, bad, &f) == GM_OK && f.anchor_station == 0 && gm_wall_arc_add_frame(&q, &t, bad, 0) == GM_ERR_INVALID_ARG);
    bad[3] = nan;
    EXPECT(gm_wall_arc_add_frame(&q, &t, bad, &f) == GM_ERR_INVALID_ARG);

    if (fails) return 1;
    std::printf("gm_wall_arc_host_test ok\n");
    return 0;
}
