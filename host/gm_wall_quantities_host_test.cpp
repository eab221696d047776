// gm_wall_quantities_host_test -- the device-free part of gm_wall_map_quantities (csrc/gm_wall_host.hip: the defaults, the
// parameter check, one column restated, the metrics, the runs) as a stand-alone program: it links that one source file
// and nothing else of the library, initialises no device and calls no HIP function, so it runs under the host
// sanitizers.  Every buffer is sized exactly, on the heap: an overrun is a report.  Prints
// "gm_wall_quantities_host_test ok".
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

static const int32_t kSat = 1 << 24;

static gm_wall_quantity_column_result column(int64_t Rq, uint64_t cn, int64_t sm, int32_t lo, int32_t hi, uint32_t zone = 0,
                                             const uint64_t *bn = 0, int64_t bs = 0, uint32_t min_count = 8)
{
    gm_wall_quantity_column_result c;
    std::memset(&c, 0xAB, sizeof(c));
    EXPECT(gm_wall_quantity_column(Rq, cn, sm, bn ? 1 : 0, bn ? *bn : 0, bs, min_count, lo, hi, zone, &c) == GM_OK);
    return c;
}

int main()
{
    const unsigned ns = 12, n = 10;
    gm_wall_params wp;
    gm_wall_default_params(&wp);
    wp.n_stations = 16;
    wp.n_sectors = ns;
    wp.radius = 2.0;
    wp.station_length = 0.5;
    wp.t_min = 10.0;
    const int64_t Rq = 2 << 20;

    // defaults and the parameter check: the tables are read to their last entry and no further
    gm_wall_quantity_params qp;
    gm_wall_quantity_default_params(&qp);
    gm_wall_quantity_default_params(0);
    EXPECT(qp.struct_size == 16 && qp.section_stations == 4 && qp.min_count == 8 && qp.reserved == 0);
    std::vector<int32_t> lo(2 * ns, -1000), hi(2 * ns, 1000);
    std::vector<uint8_t> prof(3, 1), zone(ns, 0);
    zone[ns - 1] = GM_WALL_QUANTITY_UNMEASURED;
    zone[1] = 2;
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 2, &prof[0], n, &zone[0], 3) == GM_OK);
    EXPECT(gm_wall_quantity_check_params(&wp, 0, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_OK);
    EXPECT(gm_wall_quantity_check_params(0, &qp, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, 0, &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 0, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 257, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 2, 0, n, &zone[0], 2) == GM_ERR_INVALID_ARG);   // zone 2 of 2
    EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 2, 0, n, 0, 9) == GM_ERR_INVALID_ARG);
    {
        gm_wall_quantity_params q = qp;
        q.section_stations = 0;
        EXPECT(gm_wall_quantity_check_params(&wp, &q, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        q = qp; q.min_count = 0;
        EXPECT(gm_wall_quantity_check_params(&wp, &q, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        q = qp; q.struct_size = 8;
        EXPECT(gm_wall_quantity_check_params(&wp, &q, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        std::vector<int32_t> l2 = lo, h2 = hi;
        l2[2 * ns - 1] = -kSat - 1;
        EXPECT(gm_wall_quantity_check_params(&wp, &qp, &l2[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        l2[2 * ns - 1] = -kSat;
        EXPECT(gm_wall_quantity_check_params(&wp, &qp, &l2[0], &hi[0], 2, 0, n, 0, 1) == GM_OK);
        h2[2 * ns - 1] = kSat + 1;
        EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &h2[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        l2 = lo; l2[0] = 1001;
        EXPECT(gm_wall_quantity_check_params(&wp, &qp, &l2[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        std::vector<uint8_t> p2(3, 0);
        p2[2] = 2;
        EXPECT(gm_wall_quantity_check_params(&wp, &qp, &lo[0], &hi[0], 2, &p2[0], n, 0, 1) == GM_ERR_INVALID_ARG);
        gm_wall_params far = wp;
        far.radius = 4096.0 + 1.0 / 1048576.0;
        EXPECT(gm_wall_quantity_check_params(&far, &qp, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_ERR_INVALID_ARG);
        far.radius = 4096.0;
        EXPECT(gm_wall_quantity_check_params(&far, &qp, &lo[0], &hi[0], 2, 0, n, 0, 1) == GM_OK);
    }

    // one column: the classes and their boundaries
    EXPECT(column(Rq, 2, -7, -10, 10, 0, 0, 0, 1).v == -3);             // toward zero
    EXPECT(column(Rq, 8, 8 * 999, 1000, 2000).cls == GM_WALL_QUANTITY_CLASS_UNDER);
    EXPECT(column(Rq, 8, 8 * 1000, 1000, 2000).cls == GM_WALL_QUANTITY_CLASS_WITHIN);
    EXPECT(column(Rq, 8, 8 * 2000, 1000, 2000).cls == GM_WALL_QUANTITY_CLASS_WITHIN);
    EXPECT(column(Rq, 8, 8 * 2001, 1000, 2000).cls == GM_WALL_QUANTITY_CLASS_OVER);
    EXPECT(column(Rq, 7, 7 * 5000, 0, 0).cls == GM_WALL_QUANTITY_CLASS_UNUSABLE && column(Rq, 7, 7 * 5000, 0, 0).v == INT32_MIN);
    EXPECT(column(Rq, 0, 0, 0, 0).cls == GM_WALL_QUANTITY_CLASS_EMPTY && column(Rq, 0, 0, 0, 0, 0xFF).cls == GM_WALL_QUANTITY_CLASS_UNMEASURED);
    EXPECT(column(Rq, 8, (int64_t)8 * (kSat + 77), 0, kSat).v == kSat && column(Rq, 8, -(int64_t)8 * (kSat + 77), -kSat, 0).v == -kSat);
    {
        const gm_wall_quantity_column_result c = column(Rq, 8, 8 * 2001, 1000, 2000);
        EXPECT(c.excess_area == ((int64_t)1 * (2 * Rq + 4001)) >> 20 && c.over_area == ((int64_t)1001 * (2 * Rq + 3001)) >> 20 &&
               c.under_area == 0 && c.over_line == 1001);
        const uint64_t bn = 8;
        // a radius of 0.25 m, the baseline at -2^24 and lo = -2^24: L clamps at 0
        const int64_t small = 1 << 18, x = small + 1000;
        const gm_wall_quantity_column_result d = column(small, 8, 8 * 1000, -kSat, 0, 0, &bn, -(int64_t)8 * kSat);
        EXPECT(d.cls == GM_WALL_QUANTITY_CLASS_OVER && d.v == 1000 + kSat && d.over_area == (x * x) >> 20 && d.excess_area == (x * x) >> 20);
        // the extreme inputs: R_q = 2^32, q = +-2^24 against a baseline at -+2^24, the tables at +-2^24
        const int64_t big = (int64_t)1 << 32;
        const gm_wall_quantity_column_result e = column(big, 8, (int64_t)8 * kSat, -kSat, kSat, 0, &bn, -(int64_t)8 * kSat);
        EXPECT(e.cls == GM_WALL_QUANTITY_CLASS_OVER && e.over_area == ((int64_t)3 * kSat * (2 * big - kSat)) >> 20);
        const gm_wall_quantity_column_result f = column(big, 8, -(int64_t)8 * kSat, kSat, kSat, 0, &bn, (int64_t)8 * kSat);
        EXPECT(f.cls == GM_WALL_QUANTITY_CLASS_UNDER && f.under_area == ((int64_t)3 * kSat * (2 * big + kSat)) >> 20);
        gm_wall_quantity_column_result out;
        EXPECT(gm_wall_quantity_column(0, 8, 0, 0, 0, 0, 8, 0, 0, 0, &out) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_column(Rq, 8, 0, 0, 0, 0, 8, 5, 4, 0, &out) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_column(Rq, 8, 0, 0, 0, 0, 8, 0, 0, 0, 0) == GM_ERR_INVALID_ARG);
    }

    // records of 5 sections x 2 zones, built from the column rule; the metrics and the runs
    const unsigned NS = 5, nz = 2;
    std::vector<gm_wall_quantity> rec(NS * nz);
    std::memset(&rec[0], 0, rec.size() * sizeof(gm_wall_quantity));
    for (unsigned i = 0; i < NS; ++i)
        for (unsigned z = 0; z < nz; ++z) {
            gm_wall_quantity &r = rec[i * nz + z];
            r.station_from = 3 + 2 * i;
            r.stations = i + 1 < NS ? 2 : 1;
            r.zone = z;
            r.peak_under_sector = r.peak_over_sector = UINT32_MAX;
            for (unsigned k = z; k < ns; k += nz) {
                const gm_wall_quantity_column_result c = column(Rq, 8 + k, (int64_t)(8 + k) * ((int64_t)(i * 700 + k * 300) - 2000), -500, 900);
                r.points += 8 + k;
                r.under_area += c.under_area; r.over_area += c.over_area; r.excess_area += c.excess_area;
                if (c.cls == GM_WALL_QUANTITY_CLASS_UNDER) ++r.under;
                else if (c.cls == GM_WALL_QUANTITY_CLASS_OVER) ++r.over;
                else ++r.within;
                if (c.cls == GM_WALL_QUANTITY_CLASS_UNDER && -c.over_line > r.peak_under) { r.peak_under = -c.over_line; r.peak_under_sector = k; }
                if (c.over_line > r.peak_over) { r.peak_over = c.over_line; r.peak_over_sector = k; }
            }
            r.unsurveyed = z;
        }
    struct gm_wall_quantity_metrics mt;
    std::memset(&mt, 0xAB, sizeof(mt));
    EXPECT(gm_wall_quantity_metrics(&wp, &rec[0], &mt) == GM_OK);
    EXPECT(mt.chainage_from == 11.5 && mt.chainage_to == 12.5 && mt.length == 1.0 && mt.coverage == 1.0 && mt.reserved == 0.0);
    EXPECT(mt.under_area_m2 > 0.0 && mt.under_volume_m3 == mt.under_area_m2 && mt.peak_under_angle_deg == 15.0);
    EXPECT(std::fabs(mt.paid_area_m2 - (mt.over_area_m2 - mt.excess_area_m2)) < 1e-12);
    EXPECT(gm_wall_quantity_metrics(&wp, &rec[1], &mt) == GM_OK && mt.coverage == 6.0 / 7.0);
    EXPECT(gm_wall_quantity_metrics(0, &rec[0], &mt) == GM_ERR_INVALID_ARG && gm_wall_quantity_metrics(&wp, 0, &mt) == GM_ERR_INVALID_ARG &&
           gm_wall_quantity_metrics(&wp, &rec[0], 0) == GM_ERR_INVALID_ARG);

    const unsigned run_sections[] = {1, 3, 9};
    for (unsigned t = 0; t < 3; ++t)
        for (unsigned all = 0; all < 2; ++all) {
            const unsigned rs = run_sections[t], NR = (NS + rs - 1) / rs, want = NR * (all ? 1 : nz);
            uint32_t got = 99;
            EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, rs, all, 0, 0, &got) == GM_OK && got == want);
            std::vector<gm_wall_quantity_run> runs(want);
            if (want > 1) {
                std::vector<gm_wall_quantity_run> few(want - 1);
                std::memset(&few[0], 0, few.size() * sizeof(few[0]));
                EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, rs, all, &few[0], want - 1, &got) == GM_ERR_CAPACITY && got == want);
                EXPECT(few[0].sections == 0);   // nothing is written
            }
            EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, rs, all, &runs[0], want, &got) == GM_OK && got == want);
            uint64_t under = 0, stations = 0;
            double vol = 0.0;
            for (unsigned r = 0; r < want; ++r) {
                under += runs[r].under;
                vol += runs[r].over_volume_m3;
                if (all || runs[r].zone == 0) stations += runs[r].stations;
                EXPECT(runs[r].zone == (all ? UINT32_MAX : r % nz) && runs[r].sections >= 1 && runs[r].sections <= rs);
                EXPECT(runs[r].chainage_to == 10.0 + 0.5 * (runs[r].station_from + runs[r].stations));
            }
            uint64_t under_want = 0;
            double vol_want = 0.0;
            for (unsigned i = 0; i < NS * nz; ++i) {
                under_want += rec[i].under;
                EXPECT(gm_wall_quantity_metrics(&wp, &rec[i], &mt) == GM_OK);
                vol_want += mt.over_volume_m3;
            }
            EXPECT(under == under_want && stations == 9 && std::fabs(vol - vol_want) <= 1e-12 * vol_want);
            EXPECT(runs[0].station_from == 3 && runs[want - 1].station_from + runs[want - 1].stations == 12);
        }
    {
        uint32_t got = 99;
        gm_wall_quantity_run one;
        EXPECT(gm_wall_quantity_runs(&wp, 0, 0, nz, 3, 0, &one, 1, &got) == GM_OK && got == 0);
        EXPECT(gm_wall_quantity_runs(&wp, 0, NS, nz, 3, 0, &one, 1, &got) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, 0, 0, &one, 1, &got) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, 9, 3, 0, &one, 1, &got) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, 3, 2, &one, 1, &got) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_quantity_runs(&wp, &rec[0], NS, nz, 3, 0, 0, 1, &got) == GM_ERR_INVALID_ARG);
    }
    if (fails) return 1;
    std::printf("gm_wall_quantities_host_test ok\n");
    return 0;
}
