// gm_wall_clothoid_host_test -- the device-free entries of the wall map on a clothoid design axis (gm_wall_clothoid_*,
// csrc/gm_wall_host.hip) as a stand-alone program: linked with that one source file, it initialises no device, so it can
// run under the host sanitizers (tests/test_wall_clothoid_np.py builds it that way).  The frame at a chainage is
// orthonormal, lies on the axis and carries the linear curvature, the axis agrees with a quadrature of its own, point and
// project are inverse to 1e-9 m, the per-add frame anchors at the sensor's station, and every refusal of the rule is
// refused.  Prints "gm_wall_clothoid_host_test ok" on success.
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

static gm_wall_clothoid clothoid_of(double nx, double ny, double nz, double k0, double rate, double s0)
{
    gm_wall_clothoid c;
    std::memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.normal[0] = nx; c.normal[1] = ny; c.normal[2] = nz;
    c.curvature = k0;
    c.rate = rate;
    c.point_chainage = s0;
    return c;
}

int main()
{
    gm_wall_params p;
    gm_wall_default_params(&p);
    p.n_stations = 480;
    p.t_min = 4980.0;
    p.point[0] = 3.0; p.point[1] = -2.0; p.point[2] = 1.0;
    p.direction[0] = 1.0; p.direction[1] = 0.05; p.direction[2] = 0.02;
    // an S-transition at chainage 5 km; the normal's component along the axis is dropped
    const gm_wall_clothoid cl = clothoid_of(0.3, 0.6, 0.8, -1.0 / 120.0, 1.0 / 7000.0, 5012.5);
    EXPECT(gm_wall_clothoid_check_params(&p, &cl) == GM_OK);

    double o[3], a[3], u[3], v[3], n[3], kappa;
    for (int k = 0; k <= 10; ++k) {
        const double s = p.t_min + 0.1 * k * p.n_stations * p.station_length;
        EXPECT(gm_wall_clothoid_frame(&p, &cl, s, o, a, u, v, &kappa, n) == GM_OK);
        EXPECT(std::fabs(dot(a, a) - 1.0) < 1e-14 && std::fabs(dot(u, u) - 1.0) < 1e-14 && std::fabs(dot(v, v) - 1.0) < 1e-14);
        EXPECT(std::fabs(dot(a, u)) < 1e-14 && std::fabs(dot(a, v)) < 1e-14 && std::fabs(dot(u, v)) < 1e-14);
        EXPECT(std::fabs(dot(n, n) - 1.0) < 1e-14 && std::fabs(dot(a, n)) < 1e-14);
        EXPECT(std::fabs(kappa - (cl.curvature + cl.rate * (s - cl.point_chainage))) < 1e-15);
        EXPECT(gm_wall_clothoid_frame(&p, &cl, s, o, a, u, v, &kappa, 0) == GM_OK);   // n is optional
        // the axis moves along its own tangent: a central difference over 2 mm
        double o0[3], o1[3], t0[3], t1[3], t2[3], k1;
        EXPECT(gm_wall_clothoid_frame(&p, &cl, s - 1e-3, o0, t0, t1, t2, &k1, 0) == GM_OK);
        EXPECT(gm_wall_clothoid_frame(&p, &cl, s + 1e-3, o1, t0, t1, t2, &k1, 0) == GM_OK);
        for (int c = 0; c < 3; ++c) EXPECT(std::fabs((o1[c] - o0[c]) / 2e-3 - a[c]) < 1e-8);
        double sp, phi, e;
        EXPECT(gm_wall_clothoid_project(&p, &cl, o, &sp, &phi, &e) == GM_OK && std::fabs(sp - s) < 1e-9 &&
               std::fabs(e + p.radius) < 1e-9);
        // point and project are inverse
        for (int j = 0; j < 16; ++j) {
            const double ang = 0.39 * j + 0.01, rho = p.radius + 0.02 * (j - 8);
            double x[3];
            EXPECT(gm_wall_clothoid_point(&p, &cl, s, ang, rho, x) == GM_OK);
            EXPECT(gm_wall_clothoid_project(&p, &cl, x, &sp, &phi, &e) == GM_OK);
            EXPECT(std::fabs(sp - s) < 1e-9 && std::fabs(e - (rho - p.radius)) < 1e-9 && std::fabs(phi - ang) * rho < 1e-9);
        }
        // the per-add frame of a sensor riding the axis there
        double pose[12];
        for (int r = 0; r < 3; ++r) {
            pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
            pose[4 * r + 3] = o[r] + 0.2 * u[r] - 0.1 * v[r];
        }
        if (k == 10) continue;   // (the map's far end: the sensor's station is n_stations)
        gm_wall_clothoid_add_info f;
        EXPECT(gm_wall_clothoid_add_frame(&p, &cl, pose, &f) == GM_OK && f.struct_size == sizeof(f) && f.reserved[0] == 0 &&
               f.reserved[1] == 0);
        EXPECT(std::fabs(f.sensor_chainage - s) < 1e-9 && f.anchor_chainage <= f.sensor_chainage + 1e-9 &&
               f.sensor_chainage < f.anchor_chainage + p.station_length + 1e-9);
        EXPECT(f.anchor_chainage == p.t_min + (double)f.anchor_station * p.station_length);
        EXPECT(std::fabs(f.a[0] - 1.0f) < 1e-4f && std::fabs(f.a[1]) < 1e-2f && std::fabs(f.a[2]) < 1e-2f);
        EXPECT(std::fabs(f.o[0]) <= (float)p.station_length + 1e-3f && std::fabs(f.o[1] + 0.1f) < 1e-3f && std::fabs(f.o[2] + 0.2f) < 1e-3f);
        EXPECT(std::fabs(f.kappa - (float)(cl.curvature + cl.rate * (f.anchor_chainage - cl.point_chainage))) < 1e-8f);
        EXPECT(f.rate == (float)cl.rate && std::fabs(f.un * f.un + f.ub * f.ub - 1.0f) < 1e-6f);
    }

    // the axis against a midpoint rule of its own, in the (a, n) plane of params.point
    {
        double a0[3], n0[3], o0[3], k0;
        EXPECT(gm_wall_clothoid_frame(&p, &cl, cl.point_chainage, o0, a0, u, v, &k0, n0) == GM_OK);
        for (int c = 0; c < 3; ++c) EXPECT(std::fabs(o0[c] - p.point[c]) < 1e-12);
        const double L = 80.0;
        const int N = 400000;
        double X = 0.0, Y = 0.0;
        for (int i = 0; i < N; ++i) {
            const double t = (i + 0.5) * L / N, psi = cl.curvature * t + 0.5 * cl.rate * t * t;
            X += std::cos(psi) * L / N;
            Y += std::sin(psi) * L / N;
        }
        EXPECT(gm_wall_clothoid_frame(&p, &cl, cl.point_chainage + L, o, a, u, v, &kappa, n) == GM_OK);
        for (int c = 0; c < 3; ++c) EXPECT(std::fabs(o[c] - (p.point[c] + X * a0[c] + Y * n0[c])) < 1e-9);
    }

    // refusals
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    gm_wall_params q;
    gm_wall_default_params(&q);
    q.n_stations = 400;   // 100 m
    gm_wall_clothoid t = clothoid_of(0.0, 1.0, 0.0, 0.0, 1.0 / 8000.0, 0.0);
    EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_OK);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, 0.9e-8, 0.0);        EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, 0.0, 0.0);           EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, 1.0 / 400.0, 0.0);   EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);   // (R + gate) kappa
    t = clothoid_of(0.0, 1.0, 0.0, 0.1, -1.0 / 1000.0, 0.0); EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);   // psi = 5 where kappa = 0
    t = clothoid_of(0.0, nan, 0.0, 0.0, 1e-4, 0.0);          EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, inf, 1e-4, 0.0);          EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, nan, 0.0);           EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, 1e-4, inf);          EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.5, 0.0, 0.0, 0.0, 1e-4, 0.0);          EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 0.0, 0.0, 0.0, 1e-4, 0.0);          EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t = clothoid_of(0.0, 1.0, 0.0, 0.0, 1e-4, 0.0);
    t.struct_size = 48;
    EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t.struct_size = sizeof(t);
    t.reserved = 7;
    EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_ERR_INVALID_ARG);
    t.reserved = 0;
    EXPECT(gm_wall_clothoid_check_params(&q, &t) == GM_OK);
    EXPECT(gm_wall_clothoid_check_params(0, &t) == GM_ERR_INVALID_ARG && gm_wall_clothoid_check_params(&q, 0) == GM_ERR_INVALID_ARG);
    double x[3] = {0.0, 0.0, 2.0}, sp, phi, e;
    EXPECT(gm_wall_clothoid_frame(&q, &t, nan, o, a, u, v, &kappa, n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_clothoid_frame(&q, &t, 1.0, 0, a, u, v, &kappa, n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_clothoid_frame(&q, &t, 1.0, o, a, u, v, 0, n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_clothoid_project(&q, &t, 0, &sp, &phi, &e) == GM_ERR_INVALID_ARG &&
           gm_wall_clothoid_project(&q, &t, x, 0, &phi, &e) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_clothoid_point(&q, &t, 1.0, inf, 2.0, x) == GM_ERR_INVALID_ARG &&
           gm_wall_clothoid_point(&q, &t, 1.0, 0.0, 2.0, 0) == GM_ERR_INVALID_ARG);
    gm_wall_clothoid_add_info f;
    double bad[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0};   // a reflection
    EXPECT(gm_wall_clothoid_add_frame(&q, &t, bad, &f) == GM_ERR_INVALID_ARG && gm_wall_clothoid_add_frame(&q, &t, 0, &f) == GM_ERR_INVALID_ARG);
    bad[10] = 1.0;
    EXPECT(gm_wall_clothoid_add_frame(&q, &t, bad, &f) == GM_OK && f.anchor_station == 0 &&
           gm_wall_clothoid_add_frame(&q, &t, bad, 0) == GM_ERR_INVALID_ARG);
    bad[3] = 1.0e300;   // far past the map's end: the anchor is out of range
    EXPECT(gm_wall_clothoid_add_frame(&q, &t, bad, &f) == GM_ERR_INVALID_ARG);
    // a sensor on the axis 10 m past the map's end: accepted, anchored beyond the last station (its points class outside)
    EXPECT(gm_wall_clothoid_frame(&q, &t, 110.0, o, a, u, v, &kappa, n) == GM_OK);
    double past[12];
    for (int r = 0; r < 3; ++r) { past[4 * r] = a[r]; past[4 * r + 1] = -v[r]; past[4 * r + 2] = u[r]; past[4 * r + 3] = o[r]; }
    EXPECT(gm_wall_clothoid_add_frame(&q, &t, past, &f) == GM_OK && f.anchor_station >= 439 && f.anchor_station <= 440 &&
           std::fabs(f.sensor_chainage - 110.0) < 1e-9);
    bad[3] = nan;
    EXPECT(gm_wall_clothoid_add_frame(&q, &t, bad, &f) == GM_ERR_INVALID_ARG);

    if (fails) return 1;
    std::printf("gm_wall_clothoid_host_test ok\n");
    return 0;
}
