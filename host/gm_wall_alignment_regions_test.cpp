// gm_wall_alignment_regions_test -- the host mirror's deviation regions on a wall alignment:
// Processor::createWallAlignment on straight - clothoid - arc - straight, the element maps filled with raw cells
// (gm_wall_map_add_raw through gm_wall_alignment_map): a sparse pseudo-random field and one patch of overbreak that lies
// across the clothoid -> arc joint.  Processor::wallAlignmentRegions must give the C ABI's info and records byte for byte,
// the patch as ONE region whose station extents lie in different elements, and the window of the host-only
// gm_wall_alignment_region_window; the element maps' own gm_wall_map_regions cut the patch in two.  Prints
// "gm_wall_alignment_regions_test ok" on success.
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

static unsigned long long lcg(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

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

int main()
{
    try {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_sectors = 24;
        prm.t_min = 3.0;
        const double K = 1.0 / 80.0;
        std::vector<gm_wall_element> el;
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 20, 0.0, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 33, 0.0, K / 8.25));
        el.push_back(element(GM_WALL_ELEMENT_ARC, 70, K, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 5, 0.0, 0.0));
        const uint32_t ne = (uint32_t)el.size(), nsec = 24, total = 128, base[5] = {0, 20, 53, 123, 128};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        gm_wall_region_params rp;
        gm_wall_region_default_params(&rp);
        rp.min_cells = 4;
        bool refused = false;
        try { proc.wallAlignmentRegions(rp, 0, total); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.createWallAlignment(prm, el);

        // the virtual map's raw cells: one in nine flagged at random, and the patch: stations 50 .. 55 (the joint is at 53),
        // sectors 22 .. 1 across the seam, 0.2 m outside with its peak at (53, 0)
        std::vector<gm_wall_raw_cell> cells((size_t)total * nsec);
        std::memset(&cells[0], 0, cells.size() * sizeof(gm_wall_raw_cell));
        unsigned long long seed = 5;
        for (size_t c = 0; c < cells.size(); ++c) {
            const unsigned long long r = lcg(seed);
            const uint32_t G = (uint32_t)(c / nsec), k = (uint32_t)(c % nsec);
            const bool patch = G >= 50 && G <= 55 && (k >= 22 || k <= 1);
            const bool near_patch = G >= 48 && G <= 57 && (k >= 20 || k <= 3);
            int64_t d = 0;
            if (patch) d = (G == 53 && k == 0) ? 300000 : 200000;
            else if (!near_patch && r % 9 == 0) d = (r & 16) ? 90000 : -90000;
            cells[c].count = 10;
            cells[c].sum = 10 * d + (int64_t)(r % 7);
        }
        for (uint32_t i = 0; i < ne; ++i) {
            gm_wall_map *m = 0;
            EXPECT(gm_wall_alignment_map(proc.wallAlignment(), i, &m) == GM_OK);
            EXPECT(gm_wall_map_add_raw(m, 0, base[i + 1] - base[i], &cells[(size_t)base[i] * nsec]) == GM_OK);
        }

        const uint32_t windows[3][2] = {{0, total}, {31, 60}, {53, 70}};
        for (int wi = 0; wi < 3; ++wi) {
            const uint32_t s0 = windows[wi][0], n = windows[wi][1];
            gm_wall_alignment_regions_info mi, ai, hw;
            const std::vector<gm_wall_region> got = proc.wallAlignmentRegions(rp, s0, n, &mi);
            std::vector<gm_wall_region> want(got.size() ? got.size() : 1);
            uint32_t nw = 0;
            EXPECT(gm_wall_alignment_regions(proc.wallAlignment(), 0, s0, n, &rp, &ai, &want[0], (uint32_t)want.size(), &nw, 0) == GM_OK);
            EXPECT(nw == got.size() && std::memcmp(&mi, &ai, sizeof(mi)) == 0);
            EXPECT(got.empty() || std::memcmp(&got[0], &want[0], got.size() * sizeof(gm_wall_region)) == 0);
            EXPECT(mi.struct_size == sizeof(mi) && mi.station0 == s0 && mi.n_stations == n && mi.regions == got.size() && mi.total == total);
            EXPECT(gm_wall_alignment_region_window(&prm, &el[0], ne, s0, n, &hw) == GM_OK);
            EXPECT(hw.n_pieces == mi.n_pieces && hw.element_from == mi.element_from && hw.element_to == mi.element_to &&
                   hw.station_from == mi.station_from && hw.station_to == mi.station_to && hw.cell_area == mi.cell_area && hw.total == mi.total);
            for (size_t i = 1; i < got.size(); ++i) EXPECT(got[i - 1].label < got[i].label);
            if (wi == 2) continue;   // (that window starts at the joint: it holds the patch's second half alone)
            // the patch is one region through the joint plane
            const gm_wall_region *p = 0;
            for (size_t i = 0; i < got.size(); ++i)
                if (got[i].peak_cell == 53u * nsec) p = &got[i];
            EXPECT(p && p->cells == 24 && p->sign == 1 && p->station_min == 50 && p->station_max == 55 && p->peak == 300000);
            EXPECT(p && p->label == 50u * nsec && p->sector_min == 0 && p->sector_max == 23 && p->sector_min_turned == 10 && p->sector_max_turned == 13);
            if (p && wi == 0) {
                struct gm_wall_alignment_region_metrics m;
                EXPECT(gm_wall_alignment_region_metrics(&prm, &el[0], ne, p, &m) == GM_OK);
                EXPECT(m.element_from == 1 && m.element_to == 2 && m.station_from == 30 && m.station_to == 2);
                EXPECT(m.peak_element == 2 && m.peak_station == 0 && m.peak_sector == 0 && m.angle_from_deg == 330.0 && m.angle_to_deg == 30.0);
                std::printf("%zu regions of %llu components; the patch: %u cells, stations %u .. %u, chainage %.2f .. %.2f, peak %.3f m at (%.3f, %.3f, %.3f)\n",
                            got.size(), (unsigned long long)mi.components, p->cells, p->station_min, p->station_max, m.chainage_from, m.chainage_to,
                            m.peak_m, m.peak_point[0], m.peak_point[1], m.peak_point[2]);
            }
        }
        // each element map alone sees half of it
        for (uint32_t i = 1; i <= 2; ++i) {
            gm_wall_map *m = 0;
            EXPECT(gm_wall_alignment_map(proc.wallAlignment(), i, &m) == GM_OK);
            gm_wall_regions_info ri;
            std::vector<gm_wall_region> part(256);
            uint32_t np = 0;
            EXPECT(gm_wall_map_regions(m, 0, 0, base[i + 1] - base[i], &rp, &ri, &part[0], 256, &np, 0) == GM_OK);
            uint32_t halves = 0;
            for (uint32_t k = 0; k < np; ++k)
                if (part[k].cells == 12 && part[k].sector_min == 0 && part[k].sector_max == 23) ++halves;
            EXPECT(halves == 1);
        }
        // the capacity rule and a window outside the alignment
        gm_wall_alignment_regions_info ci;
        gm_wall_region one;
        uint32_t nc = 0;
        EXPECT(gm_wall_alignment_regions(proc.wallAlignment(), 0, 0, total, &rp, &ci, &one, 1, &nc, 0) == GM_ERR_CAPACITY && nc > 1);
        EXPECT(gm_wall_alignment_regions(proc.wallAlignment(), 0, 100, 29, &rp, &ci, 0, 0, &nc, 0) == GM_ERR_INVALID_ARG);
        EXPECT(gm_wall_alignment_regions(proc.wallAlignment(), proc.wallAlignment(), 0, total, &rp, &ci, 0, 0, &nc, 0) == GM_ERR_INVALID_ARG);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_regions_test ok\n");
    return 0;
}
