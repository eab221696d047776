// gm_wall_quantities_test -- the host mirror's quantities: a 30 x 90 wall map (chainage 100 m) is filled through
// gm_wall_map_add_raw with a tube excavated 0.12 m outside the design, an overbreak pocket 0.5 m deep at stations 8 .. 11,
// sectors 88 .. 2 (across the seam), a tight spot 0.05 m inside the design at sectors 40 .. 44 and two thin stations; a
// second map holds the same wall after 0.08 m of lining.  Processor::wallMapQuantities is compared, byte for byte, with a
// direct gm_wall_map_quantities call and with a scalar C++ restatement of the records of include/gm_hip.h on the cells
// read back (each column through gm_wall_quantity_column), through a sub-window, with zones, two profiles and a baseline;
// Processor::wallQuantityMetrics and wallQuantityRuns must name the planted volumes.  Prints "gm_wall_quantities_test ok".
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

static const unsigned kN = 30, kNs = 90;

struct Tables {
    std::vector<int32_t> lo, hi;
    std::vector<uint8_t> profile, zone;
    unsigned n_zones;
};

// the rule, one column at a time
static gm_wall_quantities_info restate(const std::vector<gm_wall_raw_cell> &raw, const std::vector<gm_wall_raw_cell> *base, int64_t Rq,
                                       unsigned station0, unsigned n, const gm_wall_quantity_params &qp, const Tables &t,
                                       std::vector<gm_wall_quantity> &out, std::vector<int32_t> &rows)
{
    const unsigned S = qp.section_stations, NS = n ? (n - 1) / S + 1 : 0, nz = t.n_zones;
    gm_wall_quantities_info info;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    info.station0 = station0; info.n_stations = n; info.n_sectors = kNs;
    info.section_stations = S; info.sections = NS; info.n_zones = nz; info.n_profiles = (uint32_t)(t.lo.size() / kNs);
    info.radius_q = Rq;
    gm_wall_quantity zero;
    std::memset(&zero, 0, sizeof(zero));
    out.assign((size_t)NS * nz, zero);
    rows.assign((size_t)NS * kNs, 0);
    uint64_t *cls[6] = {&info.unmeasured, &info.empty, &info.unusable, &info.under, &info.over, &info.within};
    for (unsigned i = 0; i < NS; ++i) {
        const unsigned from = station0 + i * S, len = n - i * S < S ? n - i * S : S, g = t.profile.empty() ? 0 : t.profile[i];
        for (unsigned z = 0; z < nz; ++z) {
            gm_wall_quantity &r = out[(size_t)i * nz + z];
            r.station_from = from; r.stations = len; r.zone = z; r.profile = g;
            r.peak_under_sector = r.peak_over_sector = UINT32_MAX;
        }
        bool any_under = false, any_over = false;
        for (unsigned k = 0; k < kNs; ++k) {
            uint64_t cn = 0, bn = 0;
            int64_t sm = 0, bs = 0;
            for (unsigned j = from; j < from + len; ++j) {
                const gm_wall_raw_cell &c = raw[j * kNs + k];
                if (c.count) { cn += c.count; sm += c.sum; }
                if (base && (*base)[j * kNs + k].count) { bn += (*base)[j * kNs + k].count; bs += (*base)[j * kNs + k].sum; }
            }
            const unsigned ze = t.zone.empty() ? 0 : t.zone[k];
            gm_wall_quantity_column_result c;
            EXPECT(gm_wall_quantity_column(Rq, cn, sm, base ? 1 : 0, bn, bs, qp.min_count, t.lo[g * kNs + k], t.hi[g * kNs + k], ze, &c) == GM_OK);
            ++*cls[c.cls];
            rows[(size_t)i * kNs + k] = c.v;
            if (c.cls == GM_WALL_QUANTITY_CLASS_UNMEASURED) continue;
            gm_wall_quantity &r = out[(size_t)i * nz + ze];
            if (c.cls == GM_WALL_QUANTITY_CLASS_EMPTY || c.cls == GM_WALL_QUANTITY_CLASS_UNUSABLE) { ++r.unsurveyed; continue; }
            r.points += cn;
            r.under_area += c.under_area; r.over_area += c.over_area; r.excess_area += c.excess_area;
            if (c.cls == GM_WALL_QUANTITY_CLASS_UNDER) {
                ++r.under;
                any_under = true;
                if (-c.over_line > r.peak_under) { r.peak_under = -c.over_line; r.peak_under_sector = k; }
            } else if (c.cls == GM_WALL_QUANTITY_CLASS_OVER) {
                ++r.over;
                any_over = true;
            } else {
                ++r.within;
            }
            if (c.over_line > r.peak_over) { r.peak_over = c.over_line; r.peak_over_sector = k; }
        }
        info.sections_under += any_under;
        info.sections_over += any_over;
    }
    return info;
}

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(T)) == 0);
}
static bool same(const gm_wall_quantities_info &a, const gm_wall_quantities_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static std::vector<gm_wall_raw_cell> tube(double lining)
{
    std::vector<gm_wall_raw_cell> raw(kN * kNs);
    std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
    for (unsigned j = 0; j < kN; ++j)
        for (unsigned k = 0; k < kNs; ++k) {
            gm_wall_raw_cell &c = raw[j * kNs + k];
            c.count = (j == 20 || j == 21) ? (k % 2 ? 3 : 0) : 10;
            if (!c.count) continue;
            double e = 0.12 - lining;
            if (j >= 8 && j <= 11 && (k >= 88 || k <= 2)) e += 0.5;
            if (k >= 40 && k <= 44) e = -0.05 - lining;
            c.sum = (int64_t)c.count * ((int64_t)std::nearbyint(e * 1048576.0) + (int64_t)((j * 7 + k * 3) % 5) - 2);
        }
    return raw;
}

int main()
{
    try {
        EXPECT(sizeof(gm_wall_quantity) == 88 && sizeof(gm_wall_quantities_info) == 96 && sizeof(gm_wall_quantity_params) == 16);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = 100.0;
        prm.station_length = 0.25;
        prm.radius = 2.0;
        const int64_t Rq = 2 << 20;
        gm_wall_quantity_params qp;
        gm_wall_quantity_default_params(&qp);
        EXPECT(qp.struct_size == sizeof(qp) && qp.section_stations == 4 && qp.min_count == 8);

        // the contract: the minimum excavation line 0.10 m and the pay line 0.25 m outside the design; a second profile
        // (a niche section) with both 0.2 m further out; crown, walls and invert, the invert's last sectors under the muck
        Tables t;
        t.lo.assign(2 * kNs, 0); t.hi.assign(2 * kNs, 0);
        for (unsigned k = 0; k < kNs; ++k) {
            t.lo[k] = 104858; t.hi[k] = 262144;
            t.lo[kNs + k] = 104858 + 209715; t.hi[kNs + k] = 262144 + 209715;
        }
        t.zone.assign(kNs, 1);
        for (unsigned k = 0; k < kNs; ++k) t.zone[k] = k < 23 ? 0 : (k < 68 ? 1 : (k < 84 ? 2 : GM_WALL_QUANTITY_UNMEASURED));
        t.n_zones = 3;

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        std::vector<gm_wall_quantity> re, re2, re3;
        std::vector<int32_t> ro, ro2, ro3;
        bool refused = false;
        try { proc.wallMapQuantities(0, kN, t.lo, t.hi, qp, re); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        gm_wall_quantities_info info = proc.wallMapQuantities(0, kN, t.lo, t.hi, qp, re);
        EXPECT(re.size() == 8 && info.empty == (uint64_t)8 * kNs && re[0].unsurveyed == kNs && re[0].peak_over_sector == UINT32_MAX);

        const std::vector<gm_wall_raw_cell> raw = tube(0.0);
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK && nc == back.size());
        // the later epoch: the same wall after 0.08 m of lining, on a second map of the same grid
        gm_wall_map *lined = 0;
        EXPECT(gm_wall_map_create(proc.ctx(), &prm, &lined) == GM_OK);
        const std::vector<gm_wall_raw_cell> raw1 = tube(0.08);
        EXPECT(gm_wall_map_add_raw(lined, 0, kN, &raw1[0]) == GM_OK);

        struct Case { unsigned s0, n, S; bool zones, profiles; };
        const Case cases[] = {{0, kN, 4, true, true}, {0, kN, 4, false, false}, {5, 20, 7, true, false}, {0, kN, 30, true, false},
                              {3, 26, 1, false, true}, {12, 0, 4, true, false}};
        for (size_t ci = 0; ci < sizeof(cases) / sizeof(cases[0]); ++ci) {
            const Case &c = cases[ci];
            qp.section_stations = c.S;
            const unsigned NS = c.n ? (c.n - 1) / c.S + 1 : 0;
            Tables u = t;
            if (!c.zones) { u.zone.clear(); u.n_zones = 1; }
            if (c.profiles) {
                u.profile.assign(NS, 0);
                if (NS > 2) u.profile[2] = 1;
                u.profile[NS - 1] = 1;
            }
            info = proc.wallMapQuantities(c.s0, c.n, u.lo, u.hi, qp, re, 0, u.profile, u.zone, u.n_zones, &ro);
            // the ABI directly
            gm_wall_quantities_info info2;
            uint32_t count = 0;
            const uint8_t *sp = u.profile.empty() ? 0 : &u.profile[0], *zn = u.zone.empty() ? 0 : &u.zone[0];
            EXPECT(gm_wall_map_quantities(proc.wallMap(), 0, c.s0, c.n, &u.lo[0], &u.hi[0], 2, sp, zn, u.n_zones, &qp, &info2, 0, 0, &count, 0) == GM_OK);
            EXPECT(count == re.size() && count == NS * u.n_zones);
            re2.assign(count ? count : 1, gm_wall_quantity());
            ro2.assign(NS ? (size_t)NS * kNs : 1, 0);
            EXPECT(gm_wall_map_quantities(proc.wallMap(), 0, c.s0, c.n, &u.lo[0], &u.hi[0], 2, sp, zn, u.n_zones, &qp, &info2, &re2[0], count,
                                          &count, &ro2[0]) == GM_OK);
            re2.resize(count);
            ro2.resize((size_t)NS * kNs);
            EXPECT(same(re, re2) && same(ro, ro2) && same(info, info2));
            // the rule restated
            const gm_wall_quantities_info info3 = restate(back, 0, Rq, c.s0, c.n, qp, u, re3, ro3);
            EXPECT(same(re, re3) && same(ro, ro3) && same(info, info3));
            EXPECT(info.unmeasured + info.empty + info.unusable + info.under + info.over + info.within == (uint64_t)info.sections * kNs);
            std::printf("case %zu: window %u+%u S %u zones %u -> %llu under, %llu within, %llu over, %llu unusable\n", ci, c.s0, c.n, c.S,
                        u.n_zones, (unsigned long long)info.under, (unsigned long long)info.within, (unsigned long long)info.over,
                        (unsigned long long)info.unusable);
            if (ci == 0) {
                EXPECT(info.sections == 8 && info.radius_q == Rq && info.sections_under == 8 && info.unmeasured == 8 * 6);
                const gm_wall_quantity &pocket = re[2 * 3 + 0];   // section 2 (stations 8 .. 11), the crown: sectors 0 .. 2 of the pocket
                EXPECT(pocket.station_from == 8 && pocket.profile == 1 && pocket.over == 3 && pocket.peak_over_sector <= 2);
                const gm_wall_quantity &tight = re[0 * 3 + 1];    // section 0, the walls: five sectors inside the minimum line
                EXPECT(tight.under == 5 && tight.peak_under_sector >= 40 && tight.peak_under_sector <= 44 && tight.within == 40);
                const struct gm_wall_quantity_metrics mt = Processor::wallQuantityMetrics(prm, tight);
                EXPECT(mt.chainage_from == 100.0 && mt.chainage_to == 101.0 && mt.length == 1.0 && mt.coverage == 1.0);
                EXPECT(std::fabs(mt.peak_under_m - 0.15) < 1e-4);
                // five sectors of a ring between 1.95 m and 2.10 m
                const double want = 3.14159265358979323846 * (2.1 * 2.1 - 1.95 * 1.95) * 5.0 / 90.0;
                EXPECT(std::fabs(mt.under_area_m2 - want) < 1e-4 && std::fabs(mt.under_volume_m3 - want) < 1e-4);
                const std::vector<gm_wall_quantity_run> runs = Processor::wallQuantityRuns(prm, re, 3, 3);
                EXPECT(runs.size() == 9 && runs[0].sections == 3 && runs[6].sections == 2 && runs[6].stations == 6 && runs[6].station_from == 24);
                const std::vector<gm_wall_quantity_run> all = Processor::wallQuantityRuns(prm, re, 3, 100, true);
                EXPECT(all.size() == 1 && all[0].zone == UINT32_MAX && all[0].stations == kN && all[0].chainage_to == 107.5);
                EXPECT(all[0].peak_over_station == 8 && all[0].over >= 3);
            }
            if (ci == 5) EXPECT(re.empty() && ro.empty() && info.sections == 0);
        }
        // the lining: the later epoch against the earlier one, lo = hi = 0; under_area is the lining
        {
            qp.section_stations = 4;
            Tables u;
            u.lo.assign(kNs, 0); u.hi.assign(kNs, 0);
            u.n_zones = 1;
            std::vector<gm_wall_raw_cell> back1(raw1.size());
            EXPECT(gm_wall_map_read_raw(lined, 0, kN, &back1[0], back1.size(), &nc) == GM_OK);
            gm_wall_quantities_info li, li3;
            std::vector<gm_wall_quantity> lr, lr3;
            std::vector<int32_t> lrow, lrow3;
            uint32_t count = 0;
            lr.assign(8, gm_wall_quantity());
            lrow.assign(8 * kNs, 0);
            EXPECT(gm_wall_map_quantities(lined, proc.wallMap(), 0, kN, &u.lo[0], &u.hi[0], 1, 0, 0, 1, &qp, &li, &lr[0], 8, &count, &lrow[0]) == GM_OK);
            li3 = restate(back1, &back, Rq, 0, kN, qp, u, lr3, lrow3);
            EXPECT(count == 8 && same(lr, lr3) && same(lrow, lrow3) && same(li, li3));
            EXPECT(li.under == (uint64_t)8 * kNs && li.over == 0 && lr[0].under == kNs && lrow[0] == -83886);
            const struct gm_wall_quantity_metrics mt = Processor::wallQuantityMetrics(prm, lr[0]);
            EXPECT(std::fabs(mt.peak_under_m - 0.08) < 1e-5 && mt.under_volume_m3 > 0.9 && mt.under_volume_m3 < 1.1);   // ~ 2 pi 2.08 0.08 1 m
            // thin lining: required 0.10 m, so everything is thinner
            for (unsigned k = 0; k < kNs; ++k) u.lo[k] = u.hi[k] = -104858;
            EXPECT(gm_wall_map_quantities(lined, proc.wallMap(), 0, kN, &u.lo[0], &u.hi[0], 1, 0, 0, 1, &qp, &li, &lr[0], 8, &count, 0) == GM_OK);
            EXPECT(li.over == (uint64_t)8 * kNs && li.under == 0);
        }
        // the map was not changed
        std::vector<gm_wall_raw_cell> again(raw.size());
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &again[0], again.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&again[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        refused = false;
        try { proc.wallMapQuantities(29, 2, t.lo, t.hi, qp, re); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        refused = false;
        try { proc.wallMapQuantities(0, kN, t.lo, t.hi, qp, re, proc.wallMap()); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);   // the baseline is the map itself
        qp.min_count = 0;
        refused = false;
        try { proc.wallMapQuantities(0, kN, t.lo, t.hi, qp, re); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        gm_wall_map_destroy(lined);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_quantities_test ok\n");
    return 0;
}
