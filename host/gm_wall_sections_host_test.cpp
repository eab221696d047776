// gm_wall_sections_host_test -- the device-free part of gm_wall_map_sections (csrc/gm_wall_host.hip: the defaults, the
// parameter check, the basis table, the solve, the metrics) as a stand-alone program: it links that one source file and
// nothing else of the library, initialises no device and calls no HIP function, so it runs under the host sanitizers.
// Every buffer is sized exactly, on the heap: an overrun is a report.  Prints "gm_wall_sections_host_test ok".
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

// the sums of a ring of ns sectors whose columns `sel` hold the model of cq, on the library's table
static gm_wall_section_sums ring_sums(unsigned ns, unsigned H, const int64_t *cq, const std::vector<int> &sel, std::vector<int64_t> *values = 0)
{
    const unsigned P = 1 + 2 * H;
    std::vector<int32_t> B((size_t)ns * P);
    uint32_t got = 0;
    EXPECT(gm_wall_section_basis(ns, H, &B[0], (uint32_t)B.size(), &got) == GM_OK && got == B.size());
    gm_wall_section_sums s;
    std::memset(&s, 0, sizeof(s));
    for (unsigned k = 0; k < ns; ++k) {
        int64_t acc = 1 << 19;
        for (unsigned p = 0; p < P; ++p) acc += (int64_t)B[(size_t)k * P + p] * cq[p];
        const int64_t m = values ? (*values)[k] : acc >> 20;
        if (!sel[k]) continue;
        ++s.fitted;
        s.points += 10;
        unsigned idx = 0;
        for (unsigned p = 0; p < P; ++p) {
            for (unsigned q = p; q < P; ++q) s.N[idx++] += (int64_t)B[(size_t)k * P + p] * B[(size_t)k * P + q];
            s.r[p] += (int64_t)B[(size_t)k * P + p] * m;
        }
    }
    return s;
}

int main()
{
    // defaults and the parameter check
    gm_wall_section_params sp;
    gm_wall_section_default_params(&sp);
    gm_wall_section_default_params(0);
    EXPECT(sp.struct_size == 40 && sp.section_stations == 4 && sp.harmonics == 2 && sp.passes == 3 && sp.min_count == 8 &&
           sp.min_columns == 24 && sp.max_gap_deg == 90.0 && sp.reject == 0.05);
    EXPECT(gm_wall_section_check_params(&sp) == GM_OK && gm_wall_section_check_params(0) == GM_ERR_INVALID_ARG);
    {
        gm_wall_section_params q = sp;
        q.harmonics = 5;
        EXPECT(gm_wall_section_check_params(&q) == GM_ERR_INVALID_ARG);
        q = sp; q.passes = 0;
        EXPECT(gm_wall_section_check_params(&q) == GM_ERR_INVALID_ARG);
        q = sp; q.reject = std::nan("");
        EXPECT(gm_wall_section_check_params(&q) == GM_ERR_INVALID_ARG);
        q = sp; q.reject = 1e-9;   // Tr rounds to 0
        EXPECT(gm_wall_section_check_params(&q) == GM_ERR_INVALID_ARG);
        q = sp; q.max_gap_deg = 360.5;
        EXPECT(gm_wall_section_check_params(&q) == GM_ERR_INVALID_ARG);
        q = sp; q.section_stations = 0xFFFFFFFFu; q.harmonics = 4; q.passes = 4; q.reject = 8.0; q.max_gap_deg = 0.0;
        EXPECT(gm_wall_section_check_params(&q) == GM_OK);
    }

    // the basis: the count query, the capacity, exactly sized buffers, the table's own identities
    const unsigned sizes[] = {1, 2, 9, 63, 64, 65, 90, 360, 4096};
    for (unsigned si = 0; si < sizeof(sizes) / sizeof(sizes[0]); ++si)
        for (unsigned H = 0; H <= 4; ++H) {
            const unsigned ns = sizes[si], P = 1 + 2 * H;
            uint32_t got = 0;
            EXPECT(gm_wall_section_basis(ns, H, 0, 0, &got) == GM_OK && got == ns * P);
            std::vector<int32_t> B((size_t)ns * P, -7);
            EXPECT(gm_wall_section_basis(ns, H, &B[0], ns * P - 1, &got) == GM_ERR_CAPACITY && got == ns * P && B[0] == -7);
            EXPECT(gm_wall_section_basis(ns, H, &B[0], ns * P, 0) == GM_OK);
            for (unsigned k = 0; k < ns; ++k) {
                EXPECT(B[(size_t)k * P] == 1 << 20);
                for (unsigned h = 1; h <= H; ++h) {
                    const double c = B[(size_t)k * P + 2 * h - 1] / 1048576.0, s = B[(size_t)k * P + 2 * h] / 1048576.0;
                    EXPECT(std::fabs(c * c + s * s - 1.0) < 4e-6);
                    // the mirror sector: cos is even, sin odd about phi = pi
                    const unsigned km = ns - 1 - k;
                    EXPECT(std::abs(B[(size_t)km * P + 2 * h - 1] - B[(size_t)k * P + 2 * h - 1]) <= 1);
                    EXPECT(std::abs(B[(size_t)km * P + 2 * h] + B[(size_t)k * P + 2 * h]) <= 1);
                }
            }
        }
    EXPECT(gm_wall_section_basis(0, 2, 0, 0, 0) == GM_ERR_INVALID_ARG && gm_wall_section_basis(4097, 2, 0, 0, 0) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_section_basis(8, 5, 0, 0, 0) == GM_ERR_INVALID_ARG && gm_wall_section_basis(8, 1, 0, 3, 0) == GM_ERR_INVALID_ARG);

    // the solve: a series on a full ring comes back exactly
    const int64_t truth[9] = {-8389, 31457, -20972, 4194, 12583, -7340, 2097, -1049, 5243};
    for (unsigned si = 2; si < sizeof(sizes) / sizeof(sizes[0]); ++si)
        for (unsigned H = 0; H <= 4; ++H) {
            const unsigned ns = sizes[si], P = 1 + 2 * H;
            const gm_wall_section_sums s = ring_sums(ns, H, truth, std::vector<int>(ns, 1));
            int64_t *cq = new int64_t[9];   // exactly nine entries
            uint32_t status = 99;
            EXPECT(gm_wall_section_solve(&s, H, 9, cq, &status) == GM_OK && status == GM_SECTION_OK);
            for (unsigned p = 0; p < 9; ++p) EXPECT(cq[p] == (p < P ? truth[p] : 0));
            EXPECT(gm_wall_section_solve(&s, H, ns + 1, cq, &status) == GM_OK && status == GM_SECTION_TOO_FEW && cq[0] == 0);
            delete[] cq;
        }
    {
        int64_t cq[9];
        uint32_t status = 0;
        // identical columns: singular; the same sums with H = 0 are a mean
        std::vector<int> one(90, 0);
        one[7] = 1;
        gm_wall_section_sums s = ring_sums(90, 4, truth, one);
        for (int i = 0; i < 45; ++i) s.N[i] *= 30;
        for (int i = 0; i < 9; ++i) s.r[i] *= 30;
        s.fitted = 30;
        EXPECT(gm_wall_section_solve(&s, 4, 9, cq, &status) == GM_OK && status == GM_SECTION_SINGULAR && cq[0] == 0 && cq[8] == 0);
        // a short arc: the section fails, by its pivots or by its coefficients
        std::vector<int> arc(360, 0);
        for (int k = 0; k < 12; ++k) arc[(350 + k) % 360] = 1;
        std::vector<int64_t> ramp(360);
        for (int k = 0; k < 360; ++k) ramp[k] = k;
        s = ring_sums(360, 4, truth, arc, &ramp);
        EXPECT(gm_wall_section_solve(&s, 4, 9, cq, &status) == GM_OK && (status == GM_SECTION_SINGULAR || status == GM_SECTION_UNBOUNDED));
        for (int p = 0; p < 9; ++p) EXPECT(cq[p] == 0);
        // a coefficient beyond 2^24, and one exactly on it
        std::vector<int64_t> far(90, (1 << 24) + 1), edge(90, 1 << 24);
        s = ring_sums(90, 1, truth, std::vector<int>(90, 1), &far);
        EXPECT(gm_wall_section_solve(&s, 1, 9, cq, &status) == GM_OK && status == GM_SECTION_UNBOUNDED && cq[0] == 0);
        s = ring_sums(90, 1, truth, std::vector<int>(90, 1), &edge);
        EXPECT(gm_wall_section_solve(&s, 1, 9, cq, &status) == GM_OK && status == GM_SECTION_OK && cq[0] == 1 << 24 && cq[1] == 0);
        // all zero sums
        std::memset(&s, 0, sizeof(s));
        s.fitted = 100;
        EXPECT(gm_wall_section_solve(&s, 2, 9, cq, &status) == GM_OK && status == GM_SECTION_SINGULAR);
        EXPECT(gm_wall_section_solve(0, 2, 9, cq, &status) == GM_ERR_INVALID_ARG && gm_wall_section_solve(&s, 2, 9, 0, &status) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_section_solve(&s, 2, 9, cq, 0) == GM_ERR_INVALID_ARG && gm_wall_section_solve(&s, 5, 9, cq, &status) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_section_solve(&s, 2, 0, cq, &status) == GM_ERR_INVALID_ARG);
    }

    // the metrics
    {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.t_min = 100.0;
        gm_wall_section r;
        std::memset(&r, 0, sizeof(r));
        r.station_from = 20;
        r.stations = 4;
        r.accepted = 45;
        r.rss = 45ull << 40;   // 1 m rms
        r.coef_q[0] = -(1 << 13);                 // 2^-7 m of convergence
        r.coef_q[1] = 1 << 12; r.coef_q[2] = -(1 << 11);
        r.coef_q[3] = 0; r.coef_q[4] = 1 << 14;   // oval at 45 degrees
        struct gm_wall_section_metrics *m = new struct gm_wall_section_metrics;
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, m) == GM_OK);
        EXPECT(m->chainage_from == 105.0 && m->chainage_to == 106.0 && m->radial_m == -0.0078125 && m->radius_m == 2.0 - 0.0078125);
        EXPECT(m->centre_u == 0.00390625 && m->centre_v == -0.001953125 && m->oval_m == 0.015625);
        EXPECT(std::fabs(m->oval_angle_deg - 45.0) < 1e-12 && m->rms_m == 1.0 && m->coverage == 0.5);
        EXPECT(m->diameter_max == 2.0 * (m->radius_m + 0.015625) && m->diameter_min == 2.0 * (m->radius_m - 0.015625));
        // u = z, v = a x u = -y for the default design (axis x, up z)
        EXPECT(m->centre[0] == 105.5 && std::fabs(m->centre[1] - 0.001953125) < 1e-15 && std::fabs(m->centre[2] - 0.00390625) < 1e-15);
        const double pi = 3.14159265358979323846;
        const double area = pi * m->radius_m * m->radius_m + 0.5 * pi * (m->centre_u * m->centre_u + m->centre_v * m->centre_v + 0.015625 * 0.015625);
        EXPECT(std::fabs(m->area_m2 - area) < 1e-12);
        EXPECT(gm_wall_section_metrics(&prm, &r, 0, m) == GM_OK && m->oval_m == 0.0 && m->centre_u == 0.0 && m->oval_angle_deg == 0.0);
        r.status = GM_SECTION_TOO_FEW | GM_SECTION_OPEN_ARC;
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, m) == GM_OK && m->radius_m == 0.0 && m->chainage_to == 106.0 && m->area_m2 == 0.0);
        r.status = GM_SECTION_OPEN_ARC;   // kept
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, m) == GM_OK && m->radius_m != 0.0);
        r.stations = 0;
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, m) == GM_ERR_INVALID_ARG);
        r.stations = 4;
        EXPECT(gm_wall_section_metrics(0, &r, 2, m) == GM_ERR_INVALID_ARG && gm_wall_section_metrics(&prm, 0, 2, m) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, 0) == GM_ERR_INVALID_ARG && gm_wall_section_metrics(&prm, &r, 5, m) == GM_ERR_INVALID_ARG);
        prm.n_sectors = 0;
        EXPECT(gm_wall_section_metrics(&prm, &r, 2, m) == GM_ERR_INVALID_ARG);
        delete m;
    }
    if (fails) return 1;
    std::printf("gm_wall_sections_host_test ok\n");
    return 0;
}
