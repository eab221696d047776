// gm_wall_host_test.cpp -- the device-free part of the wall map's C ABI (csrc/gm_wall_host.hip) on the CPU.  It is linked
// with that one file and nothing else of the library: no device, no HIP runtime call, no context, no map.  Built with
// -fsanitize=address,undefined by tests/test_host_wall_pure.py: an index past a caller's table, a vector read past its
// end or an overflowing signed product ends the program.  Statuses and a handful of exact outputs are asserted; the
// numeric agreement with the twins is the ABI tests' business.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/gm_hip.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static gm_wall_params wall(uint32_t n_sectors)
{
    gm_wall_params p;
    gm_wall_default_params(&p);
    p.n_sectors = n_sectors;
    return p;
}

static int gauge()
{
    const double tri[6] = {2, -1, 0, 2, -2, -1};                // the axis at its centroid
    const double dart[8] = {3, 0, -2, 2, -1, 0, -2, -2};        // not convex at (-1, 0)
    const uint32_t sectors[4] = {1u, 2u, 3u, GM_WALL_MAX_SECTORS};
    for (int s = 0; s < 4; ++s) {
        const uint32_t ns = sectors[s];
        const gm_wall_params p = wall(ns);
        for (int shape = 0; shape < 2; ++shape) {
            const double *uv = shape ? dart : tri;
            const uint32_t nv = shape ? 4u : 3u;
            std::vector<int32_t> q(ns);                         // exactly ns entries: one more written is a finding
            uint32_t n = 77;
            REQUIRE(gm_wall_gauge_from_polygon(&p, uv, nv, nullptr, q.data(), ns, &n) == GM_OK && n == ns);
            for (uint32_t k = 0; k < ns; ++k) REQUIRE(q[k] > 0);
            if (ns == 1u) REQUIRE(q[0] == (int32_t)std::ceil((shape ? 3.0 : std::sqrt(5.0)) * 1048576.0));   // the farthest vertex
            std::vector<int32_t> small(ns - 1u, -5);            // one short: refused, nothing written
            n = 77;
            REQUIRE(gm_wall_gauge_from_polygon(&p, uv, nv, nullptr, small.data(), ns - 1u, &n) == GM_ERR_CAPACITY && n == ns);
            for (uint32_t k = 0; k + 1u < ns; ++k) REQUIRE(small[k] == -5);
            REQUIRE(gm_wall_gauge_from_polygon(&p, uv, nv, nullptr, nullptr, 0, &n) == GM_ERR_CAPACITY && n == ns);   // a count query
        }
    }
    const gm_wall_params p = wall(7);
    int32_t q[7];
    uint32_t n = 77;
    const double off[2] = {0.25, -0.25};                        // the offset moves the polygon, not the axis
    REQUIRE(gm_wall_gauge_from_polygon(&p, tri, 3, off, q, 7, &n) == GM_OK && n == 7u);
    const double on_edge[6] = {-1, 0, 1, 0, 0, 1};
    const double outside[6] = {1, 1, 2, 1, 1, 2};
    // a square with a spur along its lower side: the edge after the spur's tip runs back onto the edge before it.  No edge
    // touches the axis and the winding number is 1, so the fold check itself refuses it -- through the `next` pair (edges
    // 0 and 1) when the tip is vertex 1, through the `prev` pair (edges 0 and nv - 1) when it is vertex 0
    const double folded_next[10] = {-2, -2, 3, -2, 2, -2, 2, 2, -2, 2};
    const double folded_prev[10] = {3, -2, 2, -2, 2, 2, -2, 2, -2, -2};
    double star[10];                                            // {5/2}: the axis inside, every edge crossed by two others
    for (int k = 0; k < 5; ++k) {
        star[2 * k] = std::cos(1.5707963267948966 + 2.5132741228718345 * k);
        star[2 * k + 1] = std::sin(1.5707963267948966 + 2.5132741228718345 * k);
    }
    const double zero_edge[8] = {2, -1, 0, 2, 0, 2, -2, -1};
    REQUIRE(gm_wall_gauge_from_polygon(&p, on_edge, 3, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG && n == 0u);
    REQUIRE(gm_wall_gauge_from_polygon(&p, outside, 3, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    REQUIRE(gm_wall_gauge_from_polygon(&p, folded_next, 5, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    REQUIRE(gm_wall_gauge_from_polygon(&p, folded_prev, 5, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    const double unfolded[10] = {-2, -2, 3, -2, 3, -1, 2, 2, -2, 2};   // (the same outline with the tip's successor off the line)
    REQUIRE(gm_wall_gauge_from_polygon(&p, unfolded, 5, nullptr, q, 7, &n) == GM_OK);
    REQUIRE(gm_wall_gauge_from_polygon(&p, star, 5, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    REQUIRE(gm_wall_gauge_from_polygon(&p, zero_edge, 4, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    const double moved[2] = {5.0, 0.0};                         // (and the offset can move the axis out)
    REQUIRE(gm_wall_gauge_from_polygon(&p, tri, 3, moved, q, 7, &n) == GM_ERR_INVALID_ARG);
    std::vector<double> many(2 * (GM_WALL_GAUGE_MAX_VERTICES + 1u));
    for (uint32_t i = 0; i <= GM_WALL_GAUGE_MAX_VERTICES; ++i) {
        const double phi = 6.283185307179586 * (double)i / (double)(GM_WALL_GAUGE_MAX_VERTICES + 1u);
        many[2 * i] = std::cos(phi);
        many[2 * i + 1] = std::sin(phi);
    }
    REQUIRE(gm_wall_gauge_from_polygon(&p, many.data(), GM_WALL_GAUGE_MAX_VERTICES + 1u, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    REQUIRE(gm_wall_gauge_from_polygon(&p, tri, 2, nullptr, q, 7, &n) == GM_ERR_INVALID_ARG);
    return 0;
}

static std::vector<gm_wall_clearance_station> stations(uint32_t n, const std::vector<uint32_t> &flagged)
{
    std::vector<gm_wall_clearance_station> s(n);
    std::memset(s.data(), 0, n * sizeof(gm_wall_clearance_station));
    for (uint32_t i = 0; i < n; ++i) { s[i].min_clearance = INT64_MAX; s[i].min_sector = UINT32_MAX; }
    for (uint32_t i : flagged) { s[i].tight = 1; s[i].min_clearance = 1000 - (int64_t)i; s[i].min_sector = 2; }
    return s;
}

static int runs()
{
    const gm_wall_params p = wall(8);
    gm_wall_clearance_run r[4];
    uint32_t n = 77;
    REQUIRE(gm_wall_clearance_runs(&p, nullptr, 0, 10, 2, r, 4, &n) == GM_OK && n == 0u);
    std::vector<gm_wall_clearance_station> s = stations(4, {0, 1, 2, 3});   // all flagged: one run
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 4, 10, 0, r, 4, &n) == GM_OK && n == 1u);
    REQUIRE(r[0].station_from == 10u && r[0].station_to == 13u && r[0].tight == 4u && r[0].infringed == 0u);
    REQUIRE(r[0].min_station == 13u && r[0].min_clearance == 997 && r[0].min_sector == 2u && r[0].angle_deg == 112.5);
    REQUIRE(r[0].chainage_from == 2.5 && r[0].chainage_to == 3.5);
    s = stations(4, {});                                                    // none flagged
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 4, 10, 0, r, 4, &n) == GM_OK && n == 0u);
    s = stations(8, {0, 3});                                                // a gap of exactly max_gap joins
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, 0, 2, r, 4, &n) == GM_OK && n == 1u && r[0].station_to == 3u);
    s = stations(8, {0, 4});                                                // one more does not
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, 0, 2, r, 4, &n) == GM_OK && n == 2u);
    REQUIRE(r[0].station_from == 0u && r[0].station_to == 0u && r[1].station_from == 4u && r[1].station_to == 4u);
    n = 77;
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, 0, 2, r, 1, &n) == GM_ERR_CAPACITY && n == 2u);   // one short
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, 0, 2, nullptr, 0, &n) == GM_OK && n == 2u);       // a count query
    s = stations(8, {0, 7});
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, 0, UINT32_MAX, r, 4, &n) == GM_OK && n == 1u && r[0].station_to == 7u);
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, UINT32_MAX - 7u, UINT32_MAX, r, 4, &n) == GM_OK && r[0].station_to == UINT32_MAX);
    REQUIRE(gm_wall_clearance_runs(&p, s.data(), 8, UINT32_MAX - 6u, 0, r, 4, &n) == GM_ERR_INVALID_ARG);
    return 0;
}

static const double kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// a table of (2A + 1)(2B + 1) usable records of cost 100 per cell, but `low` (cost 1) -- an index, or -1
static int select_table(uint32_t A, uint32_t B, int low, gm_wall_align_info *info)
{
    const gm_wall_params p = wall(90);
    gm_wall_align_params ap;
    gm_wall_align_default_params(&ap);
    ap.max_station_shift = A;
    ap.max_sector_shift = B;
    const uint32_t ns = (2u * A + 1u) * (2u * B + 1u);
    std::vector<gm_wall_align_score> t(ns);                     // exactly ns records
    std::memset(t.data(), 0, ns * sizeof(gm_wall_align_score));
    for (uint32_t i = 0; i < ns; ++i) { t[i].n = 100; t[i].ssd = (int)i == low ? 100u : 10000u; }
    REQUIRE(gm_wall_align_select(&p, &ap, kIdentity, t.data(), ns - 1u, info) == GM_ERR_INVALID_ARG || ns == 1u);
    REQUIRE(gm_wall_align_select(&p, &ap, kIdentity, t.data(), ns, info) == GM_OK);
    return 0;
}

static int select()
{
    gm_wall_align_info info;
    REQUIRE(select_table(0, 0, 0, &info) == 0);                 // 1 x 1: no neighbour, no runner-up
    REQUIRE(info.status == GM_ALIGN_OK && info.best_station == 0 && info.best_sector == 0 && info.overlap == 100u);
    REQUIRE(std::isnan(info.rms_runner) && std::isinf(info.distinction) && info.shift_m == 0.0 && info.roll == 0.0);
    REQUIRE(info.pose[0] == 1.0 && info.pose[5] == 1.0 && info.pose[10] == 1.0 && info.pose[3] == 0.0);
    REQUIRE(select_table(0, 1, 1, &info) == 0);                 // 1 x 3
    REQUIRE(info.status == GM_ALIGN_OK && info.best_sector == 0 && info.frac_sector == 0.0);
    REQUIRE(select_table(1, 0, 1, &info) == 0);                 // 3 x 1
    REQUIRE(info.status == GM_ALIGN_OK && info.best_station == 0);
    REQUIRE(select_table(31, 32, 31 * 65 + 32, &info) == 0);    // the largest: 63 x 65 = 4095 of GM_WALL_ALIGN_MAX_SHIFTS
    REQUIRE(info.status == GM_ALIGN_OK && info.best_station == 0 && info.best_sector == 0 && info.distinction == 100.0);
    REQUIRE(select_table(31, 32, 4094, &info) == 0);            // ... its last record: both borders
    REQUIRE(info.status == (GM_ALIGN_OK | GM_ALIGN_AT_BORDER) && info.best_station == 31 && info.best_sector == 32);
    REQUIRE(select_table(64, 15, 64 * 31 + 15, &info) == 0);    // the longest: A = GM_WALL_ALIGN_MAX_SHIFT, 129 x 31
    REQUIRE(info.status == GM_ALIGN_OK && info.best_station == 0 && info.best_sector == 0 && info.distinction == 100.0);
    REQUIRE(select_table(64, 15, 3998, &info) == 0);            // ... its last record: both borders
    REQUIRE(info.status == (GM_ALIGN_OK | GM_ALIGN_AT_BORDER) && info.best_station == 64 && info.best_sector == 15);
    // 3 x 3: the best cell on each border, and off it
    const int at[5] = {1, 7, 3, 5, 4};
    const int sa[5] = {-1, 1, 0, 0, 0}, sb[5] = {0, 0, -1, 1, 0};
    for (int k = 0; k < 5; ++k) {
        REQUIRE(select_table(1, 1, at[k], &info) == 0);
        REQUIRE(info.best_station == sa[k] && info.best_sector == sb[k]);
        REQUIRE(info.status == (k < 4 ? (GM_ALIGN_OK | GM_ALIGN_AT_BORDER) : GM_ALIGN_OK));
    }
    // the exact comparison: (2^63 - 1) / (2^32 - 1) < (2^63 - 2^31) / (2^32 - 2) by 2e-10 of 2^31.  The two are equal as
    // doubles, and the cross products 2^95 - 2^64 - (2^32 - 2) < 2^95 - 2^64 + 2^31 order the other way in their low 64
    // bits (2^64 - 2^32 + 2 > 2^31): the later, smaller record wins only if the products are compared in 128 bits.
    const gm_wall_params p = wall(90);
    gm_wall_align_params ap;
    gm_wall_align_default_params(&ap);
    ap.max_station_shift = 0;
    ap.max_sector_shift = 1;
    gm_wall_align_score t[3];
    std::memset(t, 0, sizeof(t));
    t[0].ssd = (1ull << 63) - (1ull << 31); t[0].n = 0xFFFFFFFEu;
    t[1].ssd = 5; t[1].n = ap.min_overlap - 1u;                 // (not valid)
    t[2].ssd = (1ull << 63) - 1u; t[2].n = 0xFFFFFFFFu;
    t[0].sum_d = INT64_MIN; t[2].sum_d = INT64_MAX;
    REQUIRE(gm_wall_align_select(&p, &ap, kIdentity, t, 3, &info) == GM_OK);
    REQUIRE(info.best_sector == 1 && info.overlap == 0xFFFFFFFFu && (info.status & GM_ALIGN_FAILED_MASK) == 0u);
    // every cell below min_overlap
    for (int i = 0; i < 3; ++i) t[i].n = ap.min_overlap - 1u;
    REQUIRE(gm_wall_align_select(&p, &ap, kIdentity, t, 3, &info) == GM_OK);
    REQUIRE(info.status == GM_ALIGN_NO_OVERLAP && std::isnan(info.pose[0]) && std::isnan(info.roll) && info.overlap == 0u);
    REQUIRE(gm_wall_align_check_params(&ap, 90) == GM_OK && gm_wall_align_check_params(&ap, 2) == GM_ERR_INVALID_ARG);
    REQUIRE(gm_wall_align_check_params(nullptr, 90) == GM_ERR_INVALID_ARG);
    return 0;
}

static int metrics()
{
    gm_wall_region r;
    std::memset(&r, 0, sizeof(r));
    r.cells = 2; r.station_min = 2; r.station_max = 3;
    r.sector_min = 0; r.sector_max = 7;                         // sectors 7 and 0 of 8: across the seam
    r.sector_min_turned = 3; r.sector_max_turned = 4;
    r.peak = -(1 << 19); r.sum_d = -(1 << 20);
    struct gm_wall_region_metrics rm;
    gm_wall_params p = wall(8);
    REQUIRE(gm_wall_region_metrics(&p, &r, &rm) == GM_OK);
    REQUIRE(rm.angle_from_deg == 315.0 && rm.angle_to_deg == 45.0 && rm.chainage_from == 0.5 && rm.chainage_to == 1.0);
    REQUIRE(rm.peak_m == -0.5 && rm.mean_m == -0.5 && rm.area_m2 > 0.0 && rm.volume_m3 == -rm.area_m2 / 2.0);
    gm_wall_object o;
    std::memset(&o, 0, sizeof(o));
    o.points = 4; o.station_min = 2; o.station_max = 3;
    o.sector_min = 0; o.sector_max = 7; o.sector_min_turned = 3; o.sector_max_turned = 4;
    o.sum_x = 4 << 16; o.sum_delta = -(1 << 21); o.peak = -(1 << 20);
    o.box_max[1] = 2.0f;
    struct gm_wall_object_metrics om;
    REQUIRE(gm_wall_object_metrics(&p, nullptr, &o, &om) == GM_OK);
    REQUIRE(om.angle_from_deg == 315.0 && om.angle_to_deg == 45.0 && om.chainage_from == 0.5 && om.chainage_to == 1.0);
    REQUIRE(om.centroid[0] == 1.0 && om.centroid[1] == 0.0 && om.mean_m == -0.5 && om.peak_m == -1.0 && om.size[1] == 2.0);
    r.sector_max = 8;                                           // not a record of this grid
    REQUIRE(gm_wall_region_metrics(&p, &r, &rm) == GM_ERR_INVALID_ARG);
    p = wall(1);                                                // one sector: the whole ring, never turned
    r.sector_max = 0; r.sector_min_turned = 0; r.sector_max_turned = 0;
    o.sector_max = 0; o.sector_min_turned = 0; o.sector_max_turned = 0;
    REQUIRE(gm_wall_region_metrics(&p, &r, &rm) == GM_OK && rm.angle_from_deg == 0.0 && rm.angle_to_deg == 360.0);
    REQUIRE(gm_wall_object_metrics(&p, nullptr, &o, &om) == GM_OK && om.angle_from_deg == 0.0 && om.angle_to_deg == 360.0);
    o.points = 0;
    REQUIRE(gm_wall_object_metrics(&p, nullptr, &o, &om) == GM_ERR_INVALID_ARG);
    return 0;
}

static int directions()
{
    double cs[6];
    uint32_t n = 77;
    gm_wall_params p = wall(1);
    REQUIRE(gm_wall_cloud_directions(&p, nullptr, cs, 1, &n) == GM_OK && n == 1u && cs[0] == -1.0);   // the one sector's centre: pi
    p = wall(5);                                                // blocks of 2: the last one, at the seam, holds one sector
    gm_wall_cloud_params c;
    gm_wall_cloud_default_params(&c);
    c.block_sectors = 2;
    REQUIRE(gm_wall_cloud_directions(&p, &c, cs, 3, &n) == GM_OK && n == 3u);
    REQUIRE(cs[4] == std::cos(6.283185307179586 * 0.9) && cs[5] == std::sin(6.283185307179586 * 0.9));
    double two[4] = {9.0, 9.0, 9.0, 9.0};
    REQUIRE(gm_wall_cloud_directions(&p, &c, two, 2, &n) == GM_ERR_CAPACITY && n == 3u && two[0] == 9.0 && two[3] == 9.0);
    c.block_sectors = 1000;                                     // clamped to the ring
    REQUIRE(gm_wall_cloud_directions(&p, &c, cs, 1, &n) == GM_OK && n == 1u && cs[0] == -1.0);
    c.block_sectors = 0;
    REQUIRE(gm_wall_cloud_directions(&p, &c, cs, 3, &n) == GM_ERR_INVALID_ARG);
    return 0;
}

static int classify()
{
    gm_wall_check_params cp;
    gm_wall_check_default_params(&cp);                          // the mean, min_count 8, threshold 0.05, gate 1
    gm_wall_raw_cell cell;
    std::memset(&cell, 0, sizeof(cell));
    cell.count = 8;
    cell.sum = 8 * (1 << 18);                                   // a mean of 0.25 m
    int64_t d = 77;
    uint32_t cls = 77;
    REQUIRE(gm_wall_check_classify(&cp, &cell, 1.5f, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_BEYOND_GATE && d == 0);
    REQUIRE(gm_wall_check_classify(&cp, &cell, NAN, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_BEYOND_GATE && d == 0);
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.25f, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_UNCHANGED && d == 0);
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.5f, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_CHANGED_POS && d == 1 << 18);
    REQUIRE(gm_wall_check_classify(&cp, &cell, -0.25f, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_CHANGED_NEG && d == -(1 << 19));
    cell.count = 7;
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.5f, &d, &cls) == GM_OK && cls == GM_WALL_CHECK_CLS_UNSURVEYED && d == 0);
    cell.count = 8;
    cell.sum = INT64_MIN;                                       // a merged cell of no survey: the difference wraps, it does not overflow
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.5f, &d, &cls) == GM_OK);
    cp.reference = GM_WALL_CHECK_ENVELOPE;                      // the empty keys decode to something; whatever it is, in bounds
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.5f, &d, &cls) == GM_OK && cls <= GM_WALL_CHECK_CLS_CHANGED_NEG);
    cp.threshold = 1e-9;                                        // rounds to 0
    REQUIRE(gm_wall_check_classify(&cp, &cell, 0.5f, &d, &cls) == GM_ERR_INVALID_ARG);
    return 0;
}

static int params()
{
    gm_wall_locate_params lp;
    gm_wall_locate_default_params(&lp);
    REQUIRE(gm_wall_locate_check_params(&lp) == GM_OK && gm_wall_locate_check_params(nullptr) == GM_ERR_INVALID_ARG);
    lp.gate = NAN;
    REQUIRE(gm_wall_locate_check_params(&lp) == GM_ERR_INVALID_ARG);
    const gm_wall_params p = wall(3);
    const int32_t g[6] = {1, 2, 3, 4, 5, 6};                    // two tables of exactly n_sectors entries
    const uint8_t sg[4] = {0, 1, 1, 0};
    REQUIRE(gm_wall_clearance_check_params(&p, nullptr, g, 2, sg, 4) == GM_OK);
    REQUIRE(gm_wall_clearance_check_params(&p, nullptr, g, 1, sg, 4) == GM_ERR_INVALID_ARG);   // a station names table 1
    REQUIRE(gm_wall_clearance_check_params(&p, nullptr, g, 0, nullptr, 0) == GM_ERR_INVALID_ARG);
    gm_wall_region_params rp;
    gm_wall_object_params op;
    gm_wall_region_default_params(&rp);
    gm_wall_object_default_params(&op);
    gm_wall_object_default_params(nullptr);                     // (a NULL is ignored)
    REQUIRE(rp.struct_size == sizeof(rp) && rp.connectivity == 8u && op.struct_size == sizeof(op) && op.half_window_stations == 128u);
    return 0;
}

int main()
{
    if (gauge() || runs() || select() || metrics() || directions() || classify() || params()) return 1;
    std::printf("gm_wall_host_test ok\n");
    return 0;
}
