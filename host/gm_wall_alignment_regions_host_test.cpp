// gm_wall_alignment_regions_host_test -- the two device-free calls of the alignment's regions
// (gm_wall_alignment_region_window, gm_wall_alignment_region_metrics), linked with gm_wall_host.hip and
// gm_wall_alignment_host.hip alone, so that it also runs under the host sanitizers (tests/test_host_wall_alignment_regions.py).
// Windows at element starts and ends, one station wide, the whole alignment, 256 elements of one station, out of range and
// both arms of the size rule; metrics of a region inside one element, across one joint and across two, the peak's design
// position against gm_wall_alignment_point bit for bit, and every refusal.  Prints
// "gm_wall_alignment_regions_host_test ok" on success.
#include <cmath>
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
    e.turn[1] = -1.0;
    e.curvature = curvature;
    e.rate = rate;
    return e;
}

static gm_wall_region region(uint32_t nsec, uint32_t smin, uint32_t smax, uint32_t kmin, uint32_t kmax, uint32_t peak_station,
                             uint32_t peak_sector, int64_t peak)
{
    gm_wall_region r;
    std::memset(&r, 0, sizeof(r));
    const uint32_t half = nsec / 2u;
    r.label = smin * nsec + kmin;
    r.sign = peak > 0 ? 1 : -1;
    r.cells = (smax - smin + 1u) * (kmax - kmin + 1u);
    r.station_min = smin; r.station_max = smax;
    r.sector_min = kmin; r.sector_max = kmax;
    r.sector_min_turned = kmin + half; r.sector_max_turned = kmax + half;   // (the callers keep kmax + half < nsec)
    r.peak_cell = peak_station * nsec + peak_sector;
    r.peak = peak;
    r.sum_d = peak * (int64_t)r.cells / 2;
    r.points = 10ull * r.cells;
    return r;
}

int main()
{
    EXPECT(sizeof(gm_wall_alignment_regions_info) == 112 && sizeof(struct gm_wall_alignment_region_metrics) == 120);
    gm_wall_params prm;
    gm_wall_default_params(&prm);
    prm.n_sectors = 24;
    prm.t_min = 12.5;
    const double K = 1.0 / 80.0;
    std::vector<gm_wall_element> el;
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 10, 0.0, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 7, 0.0, K / 1.75));
    el.push_back(element(GM_WALL_ELEMENT_ARC, 5, K, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 8, 0.0, 0.0));
    const uint32_t ne = (uint32_t)el.size(), base[5] = {0, 10, 17, 22, 30};

    // ---- the window ----
    gm_wall_alignment_regions_info w;
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 0, 30, &w) == GM_OK);
    EXPECT(w.struct_size == sizeof(w) && w.station0 == 0 && w.n_stations == 30 && w.n_sectors == 24 && w.total == 30 && w.n_pieces == 4);
    EXPECT(w.element_from == 0 && w.element_to == 3 && w.station_from == 0 && w.station_to == 7 && w.regions == 0 && w.threshold_q == 0);
    EXPECT(w.cell_area == prm.station_length * prm.radius * 6.283185307179586476925286766559 / 24.0);
    for (uint32_t i = 0; i < ne; ++i) {   // element i alone; its first and its last station; across the joint behind it
        const uint32_t ni = base[i + 1] - base[i];
        EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, base[i], ni, &w) == GM_OK);
        EXPECT(w.n_pieces == 1 && w.element_from == i && w.element_to == i && w.station_from == 0 && w.station_to == ni - 1);
        EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, base[i], 1, &w) == GM_OK);
        EXPECT(w.n_pieces == 1 && w.element_from == i && w.station_from == 0 && w.station_to == 0);
        EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, base[i + 1] - 1, 1, &w) == GM_OK);
        EXPECT(w.n_pieces == 1 && w.element_to == i && w.station_from == ni - 1 && w.station_to == ni - 1);
        if (i + 1 < ne) {
            EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, base[i + 1] - 1, 2, &w) == GM_OK);
            EXPECT(w.n_pieces == 2 && w.element_from == i && w.element_to == i + 1 && w.station_from == ni - 1 && w.station_to == 0);
        }
    }
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 12, 9, &w) == GM_OK);   // mid-element to mid-element
    EXPECT(w.n_pieces == 2 && w.element_from == 1 && w.element_to == 2 && w.station_from == 2 && w.station_to == 3);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 30, 0, &w) == GM_OK && w.n_pieces == 0 && w.total == 30);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 5, 0, &w) == GM_OK && w.n_pieces == 0 && w.station0 == 5);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 30, 1, &w) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 0, 31, &w) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 0xFFFFFFFFu, 2, &w) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, 0, 30, 0) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_region_window(&prm, &el[0], 0, 0, 30, &w) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_region_window(0, &el[0], ne, 0, 30, &w) == GM_ERR_INVALID_ARG);
    {   // 256 elements of one station each
        std::vector<gm_wall_element> one(256, element(GM_WALL_ELEMENT_STRAIGHT, 1, 0.0, 0.0));
        for (uint32_t i = 0; i < 256; i += 3) one[i] = element(GM_WALL_ELEMENT_ARC, 1, K, 0.0);
        EXPECT(gm_wall_alignment_region_window(&prm, &one[0], 256, 0, 256, &w) == GM_OK);
        EXPECT(w.n_pieces == 256 && w.element_from == 0 && w.element_to == 255 && w.station_from == 0 && w.station_to == 0 && w.total == 256);
        EXPECT(gm_wall_alignment_region_window(&prm, &one[0], 256, 100, 57, &w) == GM_OK);
        EXPECT(w.n_pieces == 57 && w.element_from == 100 && w.element_to == 156);
    }
    {   // the size rule: 2^31 cells in the alignment; a window above 2^26 cells
        gm_wall_params big = prm;
        big.n_sectors = 4096;
        std::vector<gm_wall_element> many(128, element(GM_WALL_ELEMENT_STRAIGHT, 4096, 0.0, 0.0));   // 2^19 stations: 2^31 cells
        EXPECT(gm_wall_alignment_region_window(&big, &many[0], 128, 0, 1, &w) == GM_ERR_UNSUPPORTED);
        EXPECT(gm_wall_alignment_region_window(&big, &many[0], 127, 0, 1, &w) == GM_OK && w.total == 127 * 4096);
        EXPECT(gm_wall_alignment_region_window(&big, &many[0], 127, 0, 16384, &w) == GM_OK && w.n_pieces == 4);   // 2^26 cells
        EXPECT(gm_wall_alignment_region_window(&big, &many[0], 127, 0, 16385, &w) == GM_ERR_UNSUPPORTED);
        EXPECT(gm_wall_alignment_region_window(&big, &many[0], 127, 127 * 4096, 1, &w) == GM_ERR_INVALID_ARG);
    }

    // ---- the metrics ----
    const gm_wall_region in_one = region(24, 11, 14, 2, 5, 12, 3, 400000);    // inside the clothoid
    const gm_wall_region joint1 = region(24, 8, 12, 0, 4, 10, 0, -250000);    // across the straight -> clothoid joint
    const gm_wall_region joint2 = region(24, 15, 23, 7, 9, 19, 8, 123457);    // clothoid -> arc -> straight
    const gm_wall_region *rs[3] = {&in_one, &joint1, &joint2};
    const uint32_t want[3][7] = {{1, 1, 1, 4, 1, 2, 3}, {0, 1, 8, 2, 1, 0, 0}, {1, 3, 5, 1, 2, 2, 8}};
    for (int i = 0; i < 3; ++i) {
        struct gm_wall_alignment_region_metrics m;
        struct gm_wall_region_metrics head;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, rs[i], &m) == GM_OK);
        EXPECT(gm_wall_region_metrics(&prm, rs[i], &head) == GM_OK && std::memcmp(&m, &head, sizeof(head)) == 0);
        EXPECT(m.element_from == want[i][0] && m.element_to == want[i][1] && m.station_from == want[i][2] && m.station_to == want[i][3]);
        EXPECT(m.peak_element == want[i][4] && m.peak_station == want[i][5] && m.peak_sector == want[i][6] && m.reserved == 0);
        const uint32_t G = rs[i]->peak_cell / 24u, k = rs[i]->peak_cell % 24u;
        const volatile double gc = (double)G + 0.5, along = gc * prm.station_length, chainage = prm.t_min + along;
        const volatile double kc = (double)k + 0.5, turn = 6.283185307179586476925286766559 * kc, angle = turn / 24.0;
        const volatile double peak_m = (double)rs[i]->peak * 0x1p-20, rho = prm.radius + peak_m;
        double x[3];
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, chainage, angle, rho, x) == GM_OK);
        EXPECT(std::memcmp(x, m.peak_point, sizeof(x)) == 0);
        EXPECT(m.chainage_from == prm.t_min + (double)rs[i]->station_min * prm.station_length);
    }
    {   // the refusals
        struct gm_wall_alignment_region_metrics m;
        gm_wall_region r = in_one;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, 0, &m) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, 0) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_alignment_region_metrics(0, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_alignment_region_metrics(&prm, 0, ne, &r, &m) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], 0, &r, &m) == GM_ERR_INVALID_ARG);
        r.cells = 0;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        r = in_one; r.sector_max = 24;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        r = in_one; r.station_min = 15;   // min > max
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        r = in_one; r.station_max = 30;   // outside [0, total)
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        r = in_one; r.peak_cell = 30u * 24u;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_ERR_INVALID_ARG);
        r = in_one; r.peak_cell = 30u * 24u - 1u; r.station_max = 29;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, &r, &m) == GM_OK && m.peak_element == 3 && m.peak_station == 7 &&
               m.peak_sector == 23 && m.element_to == 3 && m.station_to == 7);
        gm_wall_element bad = el[1];
        bad.kind = 9;
        std::vector<gm_wall_element> el2 = el;
        el2[1] = bad;
        EXPECT(gm_wall_alignment_region_metrics(&prm, &el2[0], ne, &in_one, &m) == GM_ERR_INVALID_ARG);
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_regions_host_test ok\n");
    return 0;
}
