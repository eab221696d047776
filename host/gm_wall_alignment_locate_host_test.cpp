// gm_wall_alignment_locate_host_test -- gm_wall_alignment_locate_plan, the device-free start of a locate on a wall
// alignment, as a stand-alone program: linked with gm_wall_host.hip and gm_wall_alignment_host.hip alone (no device, no
// Python), so that it runs under the host sanitizers.  Plans before and after every joint of straight - clothoid - arc -
// clothoid - straight, four sides, the refusals.  Prints "gm_wall_alignment_locate_host_test ok" on success.
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

static double dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// the pose of a sensor on the axis at chainage s, looking along it
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
    const double K = 1.0 / 80.0;
    std::vector<gm_wall_element> el;
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, 0.0, K / 20.0));
    el.push_back(element(GM_WALL_ELEMENT_ARC, 80, K, 0.0));
    el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, K, -K / 20.0));
    el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    const uint32_t ne = (uint32_t)el.size();
    double pose[12];
    for (int j = 1; j < 5; ++j)
        for (int w = -1; w <= 1; w += 2) {
            pose_at(prm, el, 20.0 * j + w, pose);
            gm_wall_alignment_locate_start st;
            EXPECT(gm_wall_alignment_locate_plan(&prm, &el[0], ne, pose, 5.0, &st) == GM_OK);
            EXPECT(st.struct_size == sizeof(st) && st.add.n_sides == 2 && st.home == (uint32_t)(w > 0));
            EXPECT(st.add.side_element[st.home] == st.add.element && st.side_kind[0] == el[st.add.side_element[0]].kind);
            EXPECT(std::fabs(st.s0 + dot(st.c, st.d)) < 1e-15 && st.s0 > -1e-12 && st.s0 < 0.25 + 1e-9);
            EXPECT(std::fabs(dot(st.d, st.d) - 1.0) < 1e-12 && std::fabs(dot(st.d, st.u)) < 1e-12 && std::fabs(dot(st.u, st.v)) < 1e-12);
            const double *h = st.side[st.home];
            EXPECT(h[0] == 0.0 && h[1] == 0.0 && h[2] == 0.0 && h[3] == 1.0 && h[4] == 0.0 && h[5] == 0.0);
            for (uint32_t k = 0; k < 2; ++k)
                for (int q = 1; q < 4; ++q) EXPECT(std::fabs(dot(&st.side[k][3 * q], &st.side[k][3 * q]) - 1.0) < 1e-12);
            EXPECT(std::fabs(dot(&st.joint[0][3], &st.joint[0][3]) - 1.0) < 1e-12 && st.joint[1][3] == 0.0 && st.side[2][3] == 0.0);
        }
    // four sides: two 2 m elements between the straights
    std::vector<gm_wall_element> sh;
    sh.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    sh.push_back(element(GM_WALL_ELEMENT_ARC, 8, K, 0.0));
    sh.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 8, K, -K / 2.0));
    sh.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    pose_at(prm, sh, 23.5, pose);
    gm_wall_alignment_locate_start st;
    EXPECT(gm_wall_alignment_locate_plan(&prm, &sh[0], 4, pose, 5.0, &st) == GM_OK && st.add.n_sides == 4 && st.home == 2);
    EXPECT(st.side_axis[1][0] == (float)K && st.side_axis[2][1] == (float)(-K / 2.0) && st.side_axis[0][0] == 0.0f);
    // refusals
    EXPECT(gm_wall_alignment_locate_plan(&prm, &sh[0], 4, pose, 5.0, 0) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_locate_plan(&prm, &sh[0], 4, 0, 5.0, &st) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_locate_plan(&prm, &sh[0], 4, pose, -1.0, &st) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_alignment_locate_plan(&prm, 0, 4, pose, 5.0, &st) == GM_ERR_INVALID_ARG);
    std::vector<gm_wall_element> many(1, element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    for (int k = 0; k < 6; ++k) many.push_back(element(GM_WALL_ELEMENT_ARC, 4, K, 0.0));
    many.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
    pose_at(prm, many, 23.0, pose);
    EXPECT(gm_wall_alignment_locate_plan(&prm, &many[0], (uint32_t)many.size(), pose, 5.0, &st) == GM_ERR_UNSUPPORTED);
    pose[0] = NAN;
    EXPECT(gm_wall_alignment_locate_plan(&prm, &many[0], (uint32_t)many.size(), pose, 5.0, &st) == GM_ERR_INVALID_ARG);
    if (fails) return 1;
    std::printf("gm_wall_alignment_locate_host_test ok\n");
    return 0;
}
