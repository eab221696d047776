// gm_wall_alignment_align_host_test -- gm_wall_alignment_align_plan and gm_wall_alignment_align_select, the device-free
// half of an align on a wall alignment, as a stand-alone program: linked with gm_wall_host.hip and
// gm_wall_alignment_host.hip alone (no device, no Python), so that it runs under the host sanitizers.  Plans before and
// after every joint of straight - clothoid - arc - clothoid - straight, four sides, the largest search, nine pieces, the
// selection and the pose of whole-station shifts, the refusals.  Prints "gm_wall_alignment_align_host_test ok" on success.
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

// the pose of a sensor 0.1 m above the axis at chainage s, looking along it
static void pose_at(const gm_wall_params &prm, const std::vector<gm_wall_element> &el, double s, double pose[12])
{
    const uint32_t ne = (uint32_t)el.size();
    double P[3], pu[3], pv[3], u[3], v[3], a[3];
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, 0.0, 0.0, P) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, 0.0, 1.0, pu) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, 1.5707963267948966, 1.0, pv) == GM_OK);
    for (int c = 0; c < 3; ++c) { u[c] = pu[c] - P[c]; v[c] = pv[c] - P[c]; }
    a[0] = u[1] * v[2] - u[2] * v[1]; a[1] = u[2] * v[0] - u[0] * v[2]; a[2] = u[0] * v[1] - u[1] * v[0];
    for (int r = 0; r < 3; ++r) { pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r]; pose[4 * r + 3] = P[r] + 0.1 * u[r]; }
}

int main()
{
    gm_wall_params prm;
    gm_wall_default_params(&prm);
    const double K = 1.0 / 80.0, ds = prm.station_length;
    std::vector<gm_wall_element> el;
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, 0.0, K / 20.0));
    el.push_back(element(GM_WALL_ELEMENT_ARC, 80, K, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, K, -K / 20.0));
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    const uint32_t ne = (uint32_t)el.size();
    gm_wall_align_params ap;
    gm_wall_align_default_params(&ap);
    const uint32_t P = ap.half_patch_stations, A = ap.max_station_shift, B = ap.max_sector_shift, nb = 2 * B + 1, nsh = (2 * A + 1) * nb;
    double pose[12];
    gm_wall_alignment_align_plan_info pl;
    for (int j = 1; j < 5; ++j)
        for (int w = -1; w <= 1; w += 2) {
            pose_at(prm, el, 80.0 * ds * j + w, pose);
            EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 5.0, &ap, &pl) == GM_OK);
            EXPECT(pl.struct_size == sizeof(pl) && pl.add.n_sides == 2 && pl.home == (uint32_t)(w > 0) && pl.own == 0 && pl.total == 400);
            EXPECT(pl.anchor_global == 80 * (int64_t)pl.add.element + pl.add.side_anchor[pl.home] && pl.row0[pl.home] == (int32_t)P);
            EXPECT(pl.n_pieces == 2 && pl.piece[0].element == pl.add.side_element[0] && pl.piece[1].first_row == 80 * (int64_t)pl.piece[1].element);
            for (uint32_t k = 0; k < 2; ++k)   // a side's anchor station, as a global station, is within a station of the sensor's
                EXPECT(std::llabs((int64_t)pl.row0[k] - (int64_t)P) <= 1);
            // the selection and the pose of a whole shift: the pose moves |a| stations along the alignment and stays a rotation
            for (int a = -(int)A; a <= (int)A; a += (int)A) {
                std::vector<gm_wall_align_score> t(nsh);
                std::memset(&t[0], 0, nsh * sizeof(t[0]));
                t[(size_t)(a + (int)A) * nb + B].n = 1000;
                t[(size_t)(a + (int)A) * nb + B].ssd = 1u << 20;
                gm_wall_alignment_align_info info;
                EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 5.0, &ap, &t[0], nsh, &info) == GM_OK);
                EXPECT(info.struct_size == sizeof(info) && info.best_station == a && info.best_sector == 0 && info.shift_m == a * ds);
                EXPECT(!(info.status & GM_ALIGN_FAILED_MASK) && info.n_sides == 2 && info.anchor_global == pl.anchor_global);
                double want[12], worst = 0.0;
                pose_at(prm, el, 80.0 * ds * j + w + a * ds, want);
                for (int k = 0; k < 12; ++k) worst = std::fmax(worst, std::fabs(info.pose[k] - want[k]));
                EXPECT(worst < 1e-12);
            }
        }
    // mid-straight with the image inside the element: the element map's own align
    pose_at(prm, el, 10.0, pose);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 1.0, &ap, &pl) == GM_OK && pl.own == 1 && pl.n_pieces == 1 && pl.add.n_sides == 1);
    // before the alignment's start and far past its end: rows outside [0, total), then no piece at all
    pose_at(prm, el, 0.3, pose);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 1.0, &ap, &pl) == GM_OK && pl.own == 1 && pl.anchor_global == 1);
    pose_at(prm, el, 200.0, pose);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 1.0, &ap, &pl) == GM_OK && pl.n_pieces == 0 && pl.own == 1);
    std::vector<gm_wall_align_score> none(nsh);
    std::memset(&none[0], 0, nsh * sizeof(none[0]));
    gm_wall_alignment_align_info info;
    EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 1.0, &ap, &none[0], nsh, &info) == GM_OK);
    EXPECT(info.status == GM_ALIGN_NO_OVERLAP && std::isnan(info.pose[0]) && std::isnan(info.shift_m) && info.best_station == 0);
    // four sides, the widest search: P + A = 109 stations on a grid of 90 sectors
    gm_wall_params p90 = prm;
    p90.n_sectors = 90;
    std::vector<gm_wall_element> sh;
    sh.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    sh.push_back(element(GM_WALL_ELEMENT_ARC, 8, K, 0.0));
    sh.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 8, K, -K / 2.0));
    sh.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    gm_wall_align_params wide = ap;
    wide.half_patch_stations = 45;
    wide.max_station_shift = 64;
    wide.max_sector_shift = 1;
    pose_at(p90, sh, 23.5, pose);
    EXPECT(gm_wall_alignment_align_plan(&p90, &sh[0], 4, pose, 5.0, &wide, &pl) == GM_OK && pl.add.n_sides == 4 && pl.home == 2 && pl.n_pieces == 4);
    EXPECT(pl.total == 176 && pl.piece[3].first_row == 96 && pl.piece[3].n_stations == 80);
    // nine one-station pieces under a reach that meets three of them; eight are accepted
    for (uint32_t n_el = 8; n_el <= 9; ++n_el) {
        std::vector<gm_wall_element> tiny(n_el, element(GM_WALL_ELEMENT_ARC, 1, K, 0.0));
        pose_at(prm, tiny, 1.1, pose);
        const gm_status st = gm_wall_alignment_align_plan(&prm, &tiny[0], n_el, pose, 0.01, &ap, &pl);
        EXPECT(st == (n_el == 8 ? GM_OK : GM_ERR_UNSUPPORTED) && pl.add.n_sides == 3 && pl.n_pieces == (n_el == 8 ? 8u : 0u));
    }
    // refusals
    pose_at(prm, el, 39.0, pose);
    std::vector<gm_wall_align_score> t(nsh);
    std::memset(&t[0], 0, nsh * sizeof(t[0]));
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 5.0, &ap, 0) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, 0, 5.0, &ap, &pl) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_plan(&prm, 0, ne, pose, 5.0, &ap, &pl) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, -1.0, &ap, &pl) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 5.0, 0, &pl) == GM_OK);   // NULL parameters: the defaults
    EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 5.0, &ap, 0, nsh, &info) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 5.0, &ap, &t[0], nsh, 0) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 5.0, &ap, &t[0], nsh + 1, &info) == GM_ERR_INVALID_ARG);
    gm_wall_align_params bad = ap;
    bad.half_patch_stations = 0;
    EXPECT(gm_wall_alignment_align_plan(&prm, &el[0], ne, pose, 5.0, &bad, &pl) == GM_ERR_INVALID_ARG);
    bad = ap;
    bad.struct_size = 8;
    EXPECT(gm_wall_alignment_align_select(&prm, &el[0], ne, pose, 5.0, &bad, &t[0], nsh, &info) == GM_ERR_INVALID_ARG);
    std::vector<gm_wall_element> many(1, element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    for (int k = 0; k < 6; ++k) many.push_back(element(GM_WALL_ELEMENT_ARC, 4, K, 0.0));
    many.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    pose_at(prm, many, 23.0, pose);
    EXPECT(gm_wall_alignment_align_plan(&prm, &many[0], (uint32_t)many.size(), pose, 5.0, &ap, &pl) == GM_ERR_UNSUPPORTED && pl.n_pieces == 0);
    pose[0] = NAN;
    EXPECT(gm_wall_alignment_align_plan(&prm, &many[0], (uint32_t)many.size(), pose, 5.0, &ap, &pl) == GM_ERR_INVALID_ARG);
    if (fails) return 1;
    std::printf("gm_wall_alignment_align_host_test ok\n");
    return 0;
}
