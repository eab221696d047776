// gm_wall_alignment_test -- the host mirror's wall alignment: Processor::createWallAlignment on straight - clothoid - arc,
// then frames on the alignment's own tube 1 m before and after each joint through the mirror (processFrame,
// addToWallAlignment), each element map compared byte for byte with a second alignment fed the frame's valid cloud through
// the C ABI's stage call (gm_wall_alignment_add_points), whose per-point owners go back through
// gm_wall_alignment_project.  Prints "gm_wall_alignment_test ok" on success.
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

static unsigned long long lcg(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}
static double uni(unsigned long long &s) { return (double)(lcg(s) % 1000000) / 1000000.0; }

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

static std::vector<gm_wall_raw_cell> read_all(gm_wall_alignment *al, uint32_t i, uint32_t n_stations)
{
    gm_wall_map *m = 0;
    EXPECT(gm_wall_alignment_map(al, i, &m) == GM_OK && m);
    std::vector<gm_wall_raw_cell> raw((size_t)n_stations * 90);
    uint64_t nc = 0;
    EXPECT(gm_wall_map_read_raw(m, 0, n_stations, &raw[0], raw.size(), &nc) == GM_OK && nc == raw.size());
    return raw;
}

int main()
{
    try {
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        const double K = 1.0 / 80.0;
        std::vector<gm_wall_element> el;
        el.push_back(element(GM_WALL_ELEMENT_STRAIGHT, 80, 0.0, 0.0));
        el.push_back(element(GM_WALL_ELEMENT_CLOTHOID, 80, 0.0, K / 20.0));
        el.push_back(element(GM_WALL_ELEMENT_ARC, 80, K, 0.0));
        const uint32_t ne = (uint32_t)el.size();

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        std::vector<gm_wall_element> bad(1, element(GM_WALL_ELEMENT_ARC, 80, -K, 0.0));
        try { proc.createWallAlignment(prm, bad); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused && !proc.wallAlignment());
        proc.createWallAlignment(prm, el);
        gm_wall_alignment *abi = 0;
        EXPECT(gm_wall_alignment_create(proc.ctx(), &prm, &el[0], ne, &abi) == GM_OK && abi);

        const unsigned n = 4000;
        unsigned long long seed = 99;
        unsigned frames = 0;
        for (int f = 0; f < 4; ++f) {
            const double s0 = 20.0 * (1 + f / 2) + (f % 2 ? 1.0 : -1.0);   // 19, 21, 39, 41
            double P[3], pu[3], pv[3], u[3], v[3], a[3], pose[12];
            EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 0.0, P) == GM_OK);
            EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 1.0, pu) == GM_OK);
            EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 1.5707963267948966, 1.0, pv) == GM_OK);
            for (int c = 0; c < 3; ++c) { u[c] = pu[c] - P[c]; v[c] = pv[c] - P[c]; }
            a[0] = u[1] * v[2] - u[2] * v[1]; a[1] = u[2] * v[0] - u[0] * v[2]; a[2] = u[0] * v[1] - u[1] * v[0];
            for (int r = 0; r < 3; ++r) {
                pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
                pose[4 * r + 3] = P[r] + 0.15 * u[r] - 0.1 * v[r];
            }
            std::vector<float> rows(4 * (size_t)n, 0.0f);
            for (unsigned i = 0; i < n; ++i) {
                const double s = s0 - 4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed), rho = 2.0 + 0.02 * (uni(seed) - 0.5);
                double x[3];
                EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, phi, rho, x) == GM_OK);
                for (int c = 0; c < 3; ++c)   // Rm^T (x - tr)
                    rows[4 * (size_t)i + c] = (float)(pose[c] * (x[0] - pose[3]) + pose[4 + c] * (x[1] - pose[7]) + pose[8 + c] * (x[2] - pose[11]));
            }
            const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
            EXPECT(fr.n_valid > n / 2);
            const gm_wall_alignment_add_info ai = proc.addToWallAlignment(pose);
            EXPECT(ai.struct_size == sizeof(ai) && ai.n_sides == 2 && ai.side_element[0] == (uint32_t)(f / 2) && std::fabs(ai.chainage - s0) < 1e-9);
            EXPECT(ai.element == (uint32_t)(f / 2 + f % 2));
            const PointCloud cloud = proc.choppedCloud();
            const uint32_t nv = (uint32_t)cloud.size();
            std::vector<float> xyz(3 * (size_t)nv), e(nv ? nv : 1);
            std::vector<int32_t> cell(nv ? nv : 1), owner(nv ? nv : 1);
            for (size_t i = 0; i < nv; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
            gm_wall_alignment_add_info ai2;
            EXPECT(gm_wall_alignment_add_points(abi, &xyz[0], nv, 0, pose, &ai2, &e[0], &cell[0], &owner[0]) == GM_OK);
            EXPECT(std::memcmp(&ai, &ai2, sizeof(ai)) == 0);
            frames += ai.n_sides;
            // the device's owner is the fp64 rule's away from the joint plane (1e-5 m: ten times the fp32 chain's bound)
            unsigned near = 0, mapped = 0;
            for (uint32_t i = 0; i < nv; ++i) {
                double x[3], s, phi, ee;
                for (int r = 0; r < 3; ++r)
                    x[r] = pose[4 * r] * xyz[3 * i] + pose[4 * r + 1] * xyz[3 * i + 1] + pose[4 * r + 2] * xyz[3 * i + 2] + pose[4 * r + 3];
                uint32_t who = 99;
                EXPECT(gm_wall_alignment_project(&prm, &el[0], ne, x, &who, &s, &phi, &ee) == GM_OK);
                const double sj = 20.0 * (1 + f / 2);
                if (std::fabs(s - sj) < 1e-5) { ++near; continue; }
                EXPECT((int32_t)who == owner[i]);
                if (cell[i] >= 0) { ++mapped; EXPECT(std::fabs(ee - e[i]) < 1e-5); }
            }
            EXPECT(near < 4 && mapped > nv / 2);
            for (uint32_t i = 0; i < ne; ++i) {
                const std::vector<gm_wall_raw_cell> ra = read_all(proc.wallAlignment(), i, 80), rb = read_all(abi, i, 80);
                EXPECT(std::memcmp(&ra[0], &rb[0], ra.size() * sizeof(gm_wall_raw_cell)) == 0);
            }
            std::printf("frame %d at %.0f m: %u valid, %u mapped, sides %u and %u\n", f, s0, nv, mapped, ai.side_element[0], ai.side_element[1]);
        }
        gm_wall_alignment_totals ta, tb;
        EXPECT(gm_wall_alignment_info(proc.wallAlignment(), &ta) == GM_OK && gm_wall_alignment_info(abi, &tb) == GM_OK);
        EXPECT(std::memcmp(&ta, &tb, sizeof(ta)) == 0 && ta.frames == frames && ta.n_elements == ne && ta.n_stations == 240);
        EXPECT(ta.chainage_min == 0.0 && ta.chainage_max == 60.0 && ta.mapped > 2 * n);
        gm_wall_alignment_destroy(abi);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_test ok\n");
    return 0;
}
