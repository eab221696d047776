// gm_wall_axis_dump -- every device-free entry of the arc, the clothoid and the alignment rules (gm_wall_arc_*,
// gm_wall_clothoid_*, gm_wall_alignment_*) over a fixed set of accepted and refused inputs, each status and each output
// printed in hex.  A stand-alone program over the C ABI, linked with gm_wall_host.hip and gm_wall_alignment_host.hip
// alone (hipcc --offload-host-only, as the host tests): two builds of those files compute the same results exactly when
// their outputs are the same text.  The inputs hold chainages near 1e5, a kappa = 0 crossing inside a clothoid, and poses
// at an element's first and last station.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/gm_hip.h"

static void dump(const char *what, int status, const void *p, size_t n)
{
    std::printf("%s st=%d ", what, status);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char *)p)[i]);
    std::printf("\n");
}

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double unit()   // [0, 1)
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg_state >> 11) / 9007199254740992.0;
}

// a rotation about a seeded axis by a seeded angle (Rodrigues), with the translation tr
static void pose_of(const double tr[3], double pose[12])
{
    double k[3] = {unit() - 0.5, unit() - 0.5, unit() - 0.5};
    const double l = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]) + 1e-300;
    for (int i = 0; i < 3; ++i) k[i] /= l;
    const double th = 6.0 * (unit() - 0.5), c = std::cos(th), s = std::sin(th);
    const double K[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) pose[4 * r + q] = (r == q ? c : 0.0) + s * K[r][q] + (1.0 - c) * k[r] * k[q];
        pose[4 * r + 3] = tr[r];
    }
}

static gm_wall_params params_of(double t_min, uint32_t n_stations)
{
    gm_wall_params p;
    gm_wall_default_params(&p);
    p.n_stations = n_stations;
    p.t_min = t_min;
    p.direction[0] = 0.9; p.direction[1] = 0.3; p.direction[2] = 0.1;
    p.point[0] = 5.0; p.point[1] = -3.0; p.point[2] = 2.0;
    return p;
}

static gm_wall_arc arc_of(double cy, double cz, double s0)
{
    gm_wall_arc a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.curvature[1] = cy; a.curvature[2] = cz;
    a.point_chainage = s0;
    return a;
}

static gm_wall_clothoid clothoid_of(double ny, double nz, double k0, double rate, double s0)
{
    gm_wall_clothoid c;
    std::memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.normal[1] = ny; c.normal[2] = nz;
    c.curvature = k0; c.rate = rate; c.point_chainage = s0;
    return c;
}

static gm_wall_element element(uint32_t kind, uint32_t n, double curvature, double rate)
{
    gm_wall_element e;
    std::memset(&e, 0, sizeof(e));
    e.struct_size = sizeof(e);
    e.kind = kind;
    e.n_stations = n;
    e.turn[0] = 0.6; e.turn[1] = -0.8;
    e.curvature = curvature;
    e.rate = rate;
    return e;
}

// the sample chainages of [s0, s1]: both ends (the first and the last station), one station inside each, seeded ones
static std::vector<double> chainages(double s0, double s1, double ds, int seeded)
{
    std::vector<double> s = {s0, s0 + 0.5 * ds, s1 - 0.5 * ds, s1, s0 - 1.5 * ds, s1 + 1.5 * ds};
    for (int i = 0; i < seeded; ++i) s.push_back(s0 + (s1 - s0) * unit());
    return s;
}

// one arc (cl NULL) or clothoid map: check, frame, point, project, add_frame
static void dump_map(const char *tag, const gm_wall_params &p, const gm_wall_arc *arc, const gm_wall_clothoid *cl)
{
    char w[96];
    std::snprintf(w, sizeof(w), "%s check", tag);
    dump(w, arc ? gm_wall_arc_check_params(&p, arc) : gm_wall_clothoid_check_params(&p, cl), "", 0);
    const double s0 = p.t_min, s1 = p.t_min + p.n_stations * p.station_length;
    const std::vector<double> ss = chainages(s0, s1, p.station_length, 12);
    for (size_t i = 0; i < ss.size(); ++i) {
        double f[16];
        std::memset(f, 0, sizeof(f));
        const int st = arc ? gm_wall_arc_frame(&p, arc, ss[i], f, f + 3, f + 6, f + 9)
                           : gm_wall_clothoid_frame(&p, cl, ss[i], f, f + 3, f + 6, f + 9, f + 12, f + 13);
        std::snprintf(w, sizeof(w), "%s frame %zu", tag, i);
        dump(w, st, f, sizeof(f));
        for (int q = 0; q < 6; ++q) {
            const double ang = q == 0 ? 0.0 : 6.283185307179586 * unit(), rho = q == 1 ? p.radius : 1.7 + 0.6 * unit();
            double x[3] = {0.0, 0.0, 0.0}, out[3] = {0.0, 0.0, 0.0};
            int sp = arc ? gm_wall_arc_point(&p, arc, ss[i], ang, rho, x) : gm_wall_clothoid_point(&p, cl, ss[i], ang, rho, x);
            std::snprintf(w, sizeof(w), "%s point %zu.%d", tag, i, q);
            dump(w, sp, x, sizeof(x));
            sp = arc ? gm_wall_arc_project(&p, arc, x, out, out + 1, out + 2) : gm_wall_clothoid_project(&p, cl, x, out, out + 1, out + 2);
            std::snprintf(w, sizeof(w), "%s project %zu.%d", tag, i, q);
            dump(w, sp, out, sizeof(out));
            if (q < 3) {   // a sensor near that point's section, any attitude
                double tr[3], pose[12];
                const int sq = arc ? gm_wall_arc_point(&p, arc, ss[i], ang, 0.4 * q, tr) : gm_wall_clothoid_point(&p, cl, ss[i], ang, 0.4 * q, tr);
                pose_of(tr, pose);
                std::snprintf(w, sizeof(w), "%s add_frame %zu.%d (%d)", tag, i, q, sq);
                if (arc) {
                    gm_wall_arc_add_info ai;
                    std::memset(&ai, 0, sizeof(ai));
                    dump(w, gm_wall_arc_add_frame(&p, arc, pose, &ai), &ai, sizeof(ai));
                } else {
                    gm_wall_clothoid_add_info ai;
                    std::memset(&ai, 0, sizeof(ai));
                    dump(w, gm_wall_clothoid_add_frame(&p, cl, pose, &ai), &ai, sizeof(ai));
                }
            }
        }
    }
}

static void dump_alignment(const char *tag, const gm_wall_params &prm, const std::vector<gm_wall_element> &el)
{
    char w[96];
    const uint32_t n = (uint32_t)el.size();
    std::snprintf(w, sizeof(w), "%s check", tag);
    dump(w, gm_wall_alignment_check(&prm, &el[0], n), "", 0);
    double s = prm.t_min;
    for (uint32_t i = 0; i < n; ++i) {
        struct { gm_wall_params p; gm_wall_arc arc; gm_wall_clothoid cl; } e;
        std::memset(&e, 0, sizeof(e));
        std::snprintf(w, sizeof(w), "%s element_params %u", tag, i);
        dump(w, gm_wall_alignment_element_params(&prm, &el[0], n, i, &e.p, &e.arc, &e.cl), &e, sizeof(e));
        const double s1 = s + el[i].n_stations * prm.station_length;
        const std::vector<double> ss = chainages(s, s1, prm.station_length, 6);
        for (size_t k = 0; k < ss.size(); ++k)
            for (int q = 0; q < 4; ++q) {
                const double ang = 6.283185307179586 * unit(), rho = q == 0 ? 0.3 : 1.7 + 0.6 * unit();
                double x[3] = {0.0, 0.0, 0.0};
                struct { uint32_t el, pad; double out[3]; } pr;
                std::memset(&pr, 0, sizeof(pr));
                std::snprintf(w, sizeof(w), "%s point %u.%zu.%d", tag, i, k, q);
                dump(w, gm_wall_alignment_point(&prm, &el[0], n, ss[k], ang, rho, x), x, sizeof(x));
                std::snprintf(w, sizeof(w), "%s project %u.%zu.%d", tag, i, k, q);
                dump(w, gm_wall_alignment_project(&prm, &el[0], n, x, &pr.el, pr.out, pr.out + 1, pr.out + 2), &pr, sizeof(pr));
                if (q > 1) continue;
                double pose[12];
                pose_of(x, pose);   // q = 0: a sensor 0.3 m off the axis
                for (double bound : {2.0, 5.0, 30.0}) {
                    gm_wall_alignment_add_info ai;
                    std::memset(&ai, 0, sizeof(ai));
                    std::snprintf(w, sizeof(w), "%s add_plan %u.%zu.%d B=%g", tag, i, k, q, bound);
                    dump(w, gm_wall_alignment_add_plan(&prm, &el[0], n, pose, bound, &ai), &ai, sizeof(ai));
                    gm_wall_alignment_locate_start ls;
                    std::memset(&ls, 0, sizeof(ls));
                    std::snprintf(w, sizeof(w), "%s locate_plan %u.%zu.%d B=%g", tag, i, k, q, bound);
                    dump(w, gm_wall_alignment_locate_plan(&prm, &el[0], n, pose, bound, &ls), &ls, sizeof(ls));
                }
            }
        for (int k = 0; k < 4; ++k) {
            const double a = s - 3.0 + 20.0 * unit(), b = a + 40.0 * unit();
            gm_wall_alignment_piece pc[8];
            std::memset(pc, 0, sizeof(pc));
            uint32_t got = 0;
            std::snprintf(w, sizeof(w), "%s window %u.%d", tag, i, k);
            const int st = gm_wall_alignment_window(&prm, &el[0], n, a, b, pc, k == 3 ? 1u : 8u, &got);
            std::printf("n=%u ", got);
            dump(w, st, pc, sizeof(pc));
        }
        s = s1;
    }
}

static void dump_refusals()
{
    const double nan = std::nan(""), inf = INFINITY;
    gm_wall_params p = params_of(3.0, 100);
    gm_wall_arc a = arc_of(0.01, 0.0, 3.0);
    gm_wall_clothoid c = clothoid_of(1.0, 0.0, 0.01, 4e-4, 3.0);
    double pose[12] = {1, 0, 0, 5, 0, 1, 0, -3, 0, 0, 1, 2}, x[3] = {5.0, -3.0, 2.0}, o[16];
    gm_wall_arc_add_info ai;
    gm_wall_clothoid_add_info ci;
    int r[64], k = 0;
    gm_wall_arc t = a;
    t = arc_of(1e-7, 0.0, 3.0);   r[k++] = gm_wall_arc_check_params(&p, &t);
    t = arc_of(0.3, 0.0, 3.0);    r[k++] = gm_wall_arc_check_params(&p, &t);
    t = arc_of(0.2, 0.0, 3.0);    r[k++] = gm_wall_arc_check_params(&p, &t);   // psi > 3
    t = arc_of(nan, 0.0, 3.0);    r[k++] = gm_wall_arc_check_params(&p, &t);
    t = arc_of(0.01, 0.0, inf);   r[k++] = gm_wall_arc_check_params(&p, &t);
    t = a; t.struct_size = 8;     r[k++] = gm_wall_arc_check_params(&p, &t);
    r[k++] = gm_wall_arc_check_params(0, &a);
    r[k++] = gm_wall_arc_check_params(&p, 0);
    gm_wall_params q = p; q.gate = 9.0;   r[k++] = gm_wall_arc_check_params(&q, &a);
    gm_wall_clothoid u = c;
    u = clothoid_of(1.0, 0.0, 0.01, 1e-9, 3.0);    r[k++] = gm_wall_clothoid_check_params(&p, &u);
    u = clothoid_of(0.0, 0.0, 0.01, 4e-4, 3.0);    r[k++] = gm_wall_clothoid_check_params(&p, &u);
    u = clothoid_of(1.0, 0.0, 0.3, 4e-4, 3.0);     r[k++] = gm_wall_clothoid_check_params(&p, &u);
    u = clothoid_of(1.0, 0.0, 0.1, 1e-2, 3.0);     r[k++] = gm_wall_clothoid_check_params(&p, &u);
    u = clothoid_of(1.0, 0.0, nan, 4e-4, 3.0);     r[k++] = gm_wall_clothoid_check_params(&p, &u);
    u = c; u.reserved = 1;                         r[k++] = gm_wall_clothoid_check_params(&p, &u);
    r[k++] = gm_wall_clothoid_check_params(&p, 0);
    r[k++] = gm_wall_clothoid_check_params(&q, &c);
    // the entries' own refusals
    double bad[12];
    std::memcpy(bad, pose, sizeof(bad)); bad[3] = nan;
    r[k++] = gm_wall_arc_add_frame(&p, &a, bad, &ai);
    r[k++] = gm_wall_clothoid_add_frame(&p, &c, bad, &ci);
    std::memcpy(bad, pose, sizeof(bad)); bad[0] = 1.001;
    r[k++] = gm_wall_arc_add_frame(&p, &a, bad, &ai);
    r[k++] = gm_wall_clothoid_add_frame(&p, &c, bad, &ci);
    std::memcpy(bad, pose, sizeof(bad)); bad[0] = -1.0;   // a reflection
    r[k++] = gm_wall_arc_add_frame(&p, &a, bad, &ai);
    r[k++] = gm_wall_arc_add_frame(&p, &a, 0, &ai);
    r[k++] = gm_wall_clothoid_add_frame(&p, &c, pose, 0);
    r[k++] = gm_wall_arc_frame(&p, &a, nan, o, o + 3, o + 6, o + 9);
    r[k++] = gm_wall_arc_frame(&p, &a, 3.0, 0, o + 3, o + 6, o + 9);
    r[k++] = gm_wall_clothoid_frame(&p, &c, inf, o, o + 3, o + 6, o + 9, o + 12, 0);
    r[k++] = gm_wall_clothoid_frame(&p, &c, 3.0, o, o + 3, o + 6, o + 9, 0, 0);
    double xb[3] = {nan, 0.0, 0.0};
    r[k++] = gm_wall_arc_project(&p, &a, xb, o, o + 1, o + 2);
    r[k++] = gm_wall_clothoid_project(&p, &c, xb, o, o + 1, o + 2);
    r[k++] = gm_wall_arc_project(&p, &a, x, 0, o + 1, o + 2);
    r[k++] = gm_wall_arc_point(&p, &a, 3.0, nan, 2.0, o);
    r[k++] = gm_wall_clothoid_point(&p, &c, 3.0, 0.0, inf, o);
    r[k++] = gm_wall_clothoid_point(&p, &c, 3.0, 0.0, 2.0, 0);
    // the alignment's
    std::vector<gm_wall_element> el = {element(GM_WALL_ELEMENT_ARC, 100, 0.01, 0.0), element(GM_WALL_ELEMENT_CLOTHOID, 100, 0.01, 4e-4)};
    std::vector<gm_wall_element> e2 = el;
    r[k++] = gm_wall_alignment_check(&p, &el[0], 0);
    r[k++] = gm_wall_alignment_check(0, &el[0], 2);
    e2[1].kind = 3;                              r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[0].turn[0] = e2[0].turn[1] = 0;  r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[0].curvature = -0.01;            r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[1].rate = 0.0;                   r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[1].n_stations = 0;               r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[0].reserved = 1;                 r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    e2 = el; e2[0].curvature = 0.3;              r[k++] = gm_wall_alignment_check(&p, &e2[0], 2);
    gm_wall_params ep;
    r[k++] = gm_wall_alignment_element_params(&p, &el[0], 2, 2, &ep, 0, 0);
    r[k++] = gm_wall_alignment_element_params(&p, &el[0], 2, 0, 0, 0, 0);
    uint32_t owner = 0, got = 0;
    r[k++] = gm_wall_alignment_project(&p, &el[0], 2, xb, &owner, o, o + 1, o + 2);
    r[k++] = gm_wall_alignment_point(&p, &el[0], 2, nan, 0.0, 2.0, o);
    gm_wall_alignment_add_info pl;
    gm_wall_alignment_locate_start ls;
    r[k++] = gm_wall_alignment_add_plan(&p, &el[0], 2, pose, 0.0, &pl);
    r[k++] = gm_wall_alignment_add_plan(&p, &el[0], 2, bad, 5.0, &pl);
    r[k++] = gm_wall_alignment_add_plan(&p, &el[0], 2, pose, 5.0, 0);
    r[k++] = gm_wall_alignment_locate_plan(&p, &el[0], 2, pose, nan, &ls);
    r[k++] = gm_wall_alignment_locate_plan(&p, &el[0], 2, pose, 5.0, 0);
    std::vector<gm_wall_element> many(6, element(GM_WALL_ELEMENT_ARC, 4, 0.01, 0.0));
    r[k++] = gm_wall_alignment_add_plan(&p, &many[0], 6, pose, 5.0, &pl);   // too many sides
    r[k++] = gm_wall_alignment_window(&p, &el[0], 2, 10.0, 5.0, 0, 0, &got);
    r[k++] = gm_wall_alignment_window(&p, &el[0], 2, 5.0, 40.0, 0, 0, &got);
    r[k++] = gm_wall_alignment_window(&p, &el[0], 2, 5.0, 40.0, 0, 0, 0);
    for (int i = 0; i < k; ++i) std::printf("refusal %d st=%d\n", i, r[i]);
}

int main()
{
    {   // arc maps: a lateral and an oblique curve; chainages near 1e5
        gm_wall_params p = params_of(3.0, 100);
        gm_wall_arc a = arc_of(0.01, 0.0, 3.0), b = arc_of(-0.012, 0.016, 10.0);
        dump_map("arc", p, &a, 0);
        dump_map("arc_oblique", p, &b, 0);
        gm_wall_params f = params_of(1.0e5 - 7.0, 160);
        gm_wall_arc c = arc_of(0.0, 0.02, 1.0e5);
        dump_map("arc_far", f, &c, 0);
    }
    {   // clothoid maps: growing, a kappa = 0 crossing inside, chainages near 1e5
        gm_wall_params p = params_of(3.0, 100);
        gm_wall_clothoid a = clothoid_of(1.0, 0.0, 0.01, 4e-4, 3.0), b = clothoid_of(-0.6, 0.8, -0.005, 4e-4, 3.0);
        dump_map("clothoid", p, 0, &a);
        dump_map("clothoid_s", p, 0, &b);
        gm_wall_params f = params_of(1.0e5 - 7.0, 160);
        gm_wall_clothoid c = clothoid_of(0.0, 2.0, -0.008, 4e-4, 1.0e5);
        dump_map("clothoid_far", f, 0, &c);
    }
    {
        std::vector<gm_wall_element> el;
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 40, 0.0, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 48, 0.0, 0.0125 / 12.0));
        el.push_back(element(GM_WALL_ELEMENT_ARC, 40, 0.0125, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 96, 0.0125, -0.0125 / 12.0));   // through kappa = 0 to -0.0125
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 40, 0.0, 0.0));
        dump_alignment("alignment", params_of(3.0, 0), el);
        dump_alignment("alignment_far", params_of(1.0e5, 0), el);
        gm_wall_params odd = params_of(1.0e5 + 0.1, 0);   // no chainage of it is a short binary fraction
        odd.station_length = 0.3;
        dump_alignment("alignment_odd", odd, el);
        odd.n_stations = 90;
        gm_wall_arc a = arc_of(0.01, 0.003, 1.0e5 - 2.7);
        gm_wall_clothoid c = clothoid_of(0.3, 1.0, -0.004, 4e-4, 1.0e5 - 2.7);
        dump_map("arc_odd", odd, &a, 0);
        dump_map("clothoid_odd", odd, 0, &c);
        std::vector<gm_wall_element> one(1, element(GM_WALL_ELEMENT_CLOTHOID, 100, 0.01, 4e-4));
        dump_alignment("alignment_one", params_of(3.0, 0), one);
    }
    dump_refusals();
    return 0;
}
