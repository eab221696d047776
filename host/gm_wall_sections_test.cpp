// gm_wall_sections_test -- the host mirror's sections: a 66 x 90 wall map (chainage 100 m) is filled through
// gm_wall_map_add_raw with a tube that has closed by 8 mm, sits 5 mm off the axis and is 4 mm oval, a niche 0.3 m deep at
// stations 20 .. 23, sectors 86 .. 3 (across the seam) and two thin stations.  Processor::wallMapSections is compared,
// byte for byte, with a direct gm_wall_map_sections call and with a scalar C++ restatement of the rule of
// include/gm_hip.h on the cells read back (the basis and the solve through gm_wall_section_basis and
// gm_wall_section_solve), through a sub-window, with every harmonic count and against a baseline;
// Processor::wallSectionMetrics must name the convergence.  Prints "gm_wall_sections_test ok" on success.
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

static const unsigned kN = 66, kNs = 90;
static const int64_t kSat = 1 << 24;

// the rule, one section at a time
static gm_wall_sections_info restate(const std::vector<gm_wall_raw_cell> &raw, const std::vector<gm_wall_raw_cell> *base, unsigned station0,
                                     unsigned n, const gm_wall_section_params &sp, std::vector<gm_wall_section> &out,
                                     std::vector<gm_wall_section_sums> &sums)
{
    const unsigned S = sp.section_stations, H = sp.harmonics, P = 1 + 2 * H, NS = n ? (n - 1) / S + 1 : 0;
    gm_wall_sections_info info;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    info.station0 = station0; info.n_stations = n; info.n_sectors = kNs;
    info.section_stations = S; info.sections = NS; info.harmonics = H; info.passes = sp.passes;
    info.reject_q = (int64_t)std::nearbyint(sp.reject * 1048576.0);
    info.max_gap_sectors = (uint32_t)std::floor(sp.max_gap_deg * kNs / 360.0);
    std::vector<int32_t> B(kNs * P);
    uint32_t got = 0;
    EXPECT(gm_wall_section_basis(kNs, H, &B[0], (uint32_t)B.size(), &got) == GM_OK && got == B.size());
    out.assign(NS, gm_wall_section());
    sums.assign(NS, gm_wall_section_sums());
    for (unsigned i = 0; i < NS; ++i) {
        gm_wall_section &r = out[i];
        std::memset(&r, 0, sizeof(r));
        r.station_from = station0 + i * S;
        r.stations = n - i * S < S ? n - i * S : S;
        std::vector<int64_t> m(kNs, 0);
        std::vector<uint64_t> cnt(kNs, 0);
        std::vector<int> usable(kNs, 0);
        for (unsigned k = 0; k < kNs; ++k) {
            uint64_t cn = 0, bn = 0;
            int64_t sm = 0, bs = 0;
            for (unsigned j = r.station_from; j < r.station_from + r.stations; ++j) {
                const gm_wall_raw_cell &c = raw[j * kNs + k];
                if (c.count) { cn += c.count; sm += c.sum; }
                if (base && (*base)[j * kNs + k].count) { bn += (*base)[j * kNs + k].count; bs += (*base)[j * kNs + k].sum; }
            }
            cnt[k] = cn;
            if (cn == 0 && bn == 0) { ++info.empty; continue; }
            if (cn < sp.min_count || (base && bn < sp.min_count)) { ++info.unusable; continue; }
            ++info.usable; ++r.usable;
            usable[k] = 1;
            int64_t q = sm / (int64_t)cn;
            if (base) q -= bs / (int64_t)bn;
            m[k] = q > kSat ? kSat : (q < -kSat ? -kSat : q);
        }
        std::vector<int64_t> rho(kNs, 0);
        int64_t cq[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t status = 0;
        for (unsigned pass = 1; pass <= sp.passes + 1 && !status; ++pass) {
            const bool eval = pass == sp.passes + 1;
            const int64_t thr = pass == 1 ? INT64_MAX : (eval ? info.reject_q : info.reject_q << (sp.passes - pass));
            gm_wall_section_sums s;
            std::memset(&s, 0, sizeof(s));
            std::vector<int> sel(kNs, 0);
            uint64_t rss = 0;
            for (unsigned k = 0; k < kNs; ++k) {
                int64_t acc = 1 << 19;
                for (unsigned p = 0; p < P; ++p) acc += (int64_t)B[k * P + p] * cq[p];
                rho[k] = m[k] - (acc >> 20);
                sel[k] = usable[k] && (rho[k] < 0 ? -rho[k] : rho[k]) <= thr;
                if (!sel[k]) continue;
                ++s.fitted;
                s.points += cnt[k];
                rss += (uint64_t)(rho[k] * rho[k]);
                unsigned idx = 0;
                for (unsigned p = 0; p < P; ++p) {
                    for (unsigned q = p; q < P; ++q) s.N[idx++] += (int64_t)B[k * P + p] * B[k * P + q];
                    s.r[p] += (int64_t)B[k * P + p] * m[k];
                }
            }
            unsigned gap = 0;   // the longest cyclic run that is not selected
            if (!s.fitted) gap = kNs;
            else
                for (unsigned k0 = 0; k0 < kNs; ++k0) {
                    unsigned len = 0;
                    while (len < kNs && !sel[(k0 + len) % kNs]) ++len;
                    if (len > gap) gap = len;
                }
            s.largest_gap = gap;
            if (eval) {
                r.accepted = s.fitted;
                r.rejected = r.usable - r.accepted;
                r.points = s.points;
                r.rss = rss;
                r.peak_out_sector = r.peak_in_sector = UINT32_MAX;
                for (unsigned k = 0; k < kNs; ++k) {
                    if (!usable[k]) continue;
                    if (r.peak_out_sector == UINT32_MAX || rho[k] > r.peak_out) { r.peak_out = rho[k]; r.peak_out_sector = k; }
                    if (r.peak_in_sector == UINT32_MAX || rho[k] < r.peak_in) { r.peak_in = rho[k]; r.peak_in_sector = k; }
                }
                break;
            }
            sums[i] = s;
            r.fitted = s.fitted;
            r.largest_gap = gap;
            EXPECT(gm_wall_section_solve(&s, H, sp.min_columns, cq, &status) == GM_OK);
        }
        r.status = status;
        if (status) {
            r.peak_out_sector = r.peak_in_sector = UINT32_MAX;
            ++info.sections_failed;
        } else {
            std::memcpy(r.coef_q, cq, sizeof(cq));
            ++info.sections_ok;
            info.accepted += r.accepted;
            info.rejected += r.rejected;
        }
        if (r.largest_gap > info.max_gap_sectors) { r.status |= GM_SECTION_OPEN_ARC; ++info.sections_open_arc; }
    }
    return info;
}

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(T)) == 0);
}
static bool same(const gm_wall_sections_info &a, const gm_wall_sections_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static std::vector<gm_wall_raw_cell> tube(double c0, double a1, double b1, double a2, double b2, bool niche)
{
    const double pi = 3.14159265358979323846;
    std::vector<gm_wall_raw_cell> raw(kN * kNs);
    std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
    for (unsigned j = 0; j < kN; ++j)
        for (unsigned k = 0; k < kNs; ++k) {
            gm_wall_raw_cell &c = raw[j * kNs + k];
            c.count = (j == 50 || j == 51) ? (k % 2 ? 3 : 0) : 10;
            if (!c.count) continue;
            const double phi = 2.0 * pi * (2.0 * k + 1.0) / (2.0 * kNs);
            double e = c0 + a1 * std::cos(phi) + b1 * std::sin(phi) + a2 * std::cos(2 * phi) + b2 * std::sin(2 * phi);
            if (niche && j >= 20 && j <= 23 && (k >= 86 || k <= 3)) e += 0.3;
            c.sum = (int64_t)c.count * ((int64_t)std::nearbyint(e * 1048576.0) + (int64_t)((j * 7 + k * 3) % 5) - 2);
        }
    return raw;
}

int main()
{
    try {
        EXPECT(sizeof(gm_wall_section) == 144 && sizeof(gm_wall_section_sums) == 448 && sizeof(gm_wall_section_params) == 40);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = 100.0;
        gm_wall_section_params sp;
        gm_wall_section_default_params(&sp);
        EXPECT(sp.struct_size == sizeof(gm_wall_section_params) && sp.section_stations == 4 && sp.harmonics == 2 && sp.passes == 3 &&
               sp.min_count == 8 && sp.min_columns == 24 && sp.max_gap_deg == 90.0 && sp.reject == 0.05);
        EXPECT(gm_wall_section_check_params(&sp) == GM_OK);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        std::vector<gm_wall_section> se, se2, se3;
        std::vector<gm_wall_section_sums> su, su2, su3;
        bool refused = false;
        try { proc.wallMapSections(0, kN, sp, se); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        gm_wall_sections_info info = proc.wallMapSections(0, kN, sp, se);
        EXPECT(se.size() == 17 && info.empty == (uint64_t)17 * kNs && info.sections_failed == 17 && se[0].status == (GM_SECTION_TOO_FEW | GM_SECTION_OPEN_ARC));

        const std::vector<gm_wall_raw_cell> raw = tube(-0.008, 0.003, -0.004, 0.004, 0.0, true);
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK && nc == back.size());
        // the earlier epoch: the design tube, on a second map of the same grid
        gm_wall_map *then = 0;
        EXPECT(gm_wall_map_create(proc.ctx(), &prm, &then) == GM_OK);
        const std::vector<gm_wall_raw_cell> raw0 = tube(0.0, 0.003, -0.004, 0.0, 0.0, false);
        EXPECT(gm_wall_map_add_raw(then, 0, kN, &raw0[0]) == GM_OK);

        struct Case { unsigned s0, n, S, H, passes; bool baseline; };
        const Case cases[] = {{0, kN, 4, 2, 3, false}, {0, kN, 4, 0, 1, false}, {15, 20, 7, 4, 4, false}, {0, kN, 66, 1, 2, false},
                              {3, 60, 1, 3, 3, false}, {0, kN, 4, 2, 3, true}, {30, 0, 4, 2, 3, false}};
        for (size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++t) {
            const Case &c = cases[t];
            sp.section_stations = c.S; sp.harmonics = c.H; sp.passes = c.passes;
            gm_wall_map *base = c.baseline ? then : 0;
            info = proc.wallMapSections(c.s0, c.n, sp, se, base, &su);
            // the ABI directly
            gm_wall_sections_info info2;
            uint32_t count = 0;
            EXPECT(gm_wall_map_sections(proc.wallMap(), base, c.s0, c.n, &sp, &info2, 0, 0, &count, 0) == GM_OK && count == se.size());
            se2.assign(count ? count : 1, gm_wall_section());
            su2.assign(count ? count : 1, gm_wall_section_sums());
            EXPECT(gm_wall_map_sections(proc.wallMap(), base, c.s0, c.n, &sp, &info2, &se2[0], count, &count, &su2[0]) == GM_OK);
            se2.resize(count);
            su2.resize(count);
            EXPECT(same(se, se2) && same(su, su2) && same(info, info2));
            // the rule restated
            const gm_wall_sections_info info3 = restate(back, c.baseline ? &raw0 : 0, c.s0, c.n, sp, se3, su3);
            EXPECT(same(se, se3) && same(su, su3) && same(info, info3));
            EXPECT(info.empty + info.unusable + info.usable == (uint64_t)info.sections * kNs);
            std::printf("case %zu: window %u+%u S %u H %u passes %u -> %u ok, %u failed, %u open arc, %llu accepted, %llu rejected\n", t,
                        c.s0, c.n, c.S, c.H, c.passes, info.sections_ok, info.sections_failed, info.sections_open_arc,
                        (unsigned long long)info.accepted, (unsigned long long)info.rejected);
            if (t == 0) {
                EXPECT(info.sections == 17 && se[5].station_from == 20 && se[5].rejected == 8 && se[5].status == GM_SECTION_OK);
                EXPECT(se[5].peak_out_sector >= 86 || se[5].peak_out_sector <= 3);
                EXPECT(se[16].stations == 2 && se[12].station_from == 48);
                const struct gm_wall_section_metrics mt = Processor::wallSectionMetrics(prm, se[5], 2);
                EXPECT(mt.chainage_from == 105.0 && mt.chainage_to == 106.0);
                EXPECT(std::fabs(mt.radial_m + 0.008) < 1e-4 && std::fabs(mt.radius_m - 1.992) < 1e-4);     // closed by 8 mm
                EXPECT(std::fabs(mt.centre_u - 0.003) < 1e-4 && std::fabs(mt.centre_v + 0.004) < 1e-4);
                EXPECT(std::fabs(mt.oval_m - 0.004) < 1e-4 && std::fabs(mt.diameter_max - mt.diameter_min - 0.016) < 1e-3);
                EXPECT(mt.oval_angle_deg < 1.0 || mt.oval_angle_deg > 179.0);
                EXPECT(mt.coverage == 82.0 / 90.0 && mt.rms_m < 1e-5);
            }
            if (t == 5) {   // against the earlier epoch: the convergence and the ovalisation alone
                const struct gm_wall_section_metrics mt = Processor::wallSectionMetrics(prm, se[2], 2);
                EXPECT(std::fabs(mt.radial_m + 0.008) < 1e-5 && std::fabs(mt.centre_u) < 1e-5 && std::fabs(mt.centre_v) < 1e-5);
                EXPECT(std::fabs(mt.oval_m - 0.004) < 1e-5);
            }
            if (t == 6) EXPECT(se.empty() && su.empty() && info.sections == 0);
        }
        // the map was not changed
        std::vector<gm_wall_raw_cell> again(raw.size());
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &again[0], again.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&again[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        refused = false;
        try { proc.wallMapSections(65, 2, sp, se); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        refused = false;
        try { proc.wallMapSections(0, kN, sp, se, proc.wallMap()); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);   // the baseline is the map itself
        sp.harmonics = 5;
        refused = false;
        try { proc.wallMapSections(0, kN, sp, se); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        gm_wall_map_destroy(then);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_sections_test ok\n");
    return 0;
}
