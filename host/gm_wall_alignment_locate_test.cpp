// gm_wall_alignment_locate_test -- the host mirror's locate on a wall alignment: Processor::createWallAlignment on
// straight - clothoid - arc, a survey of the alignment's own tube around the clothoid -> arc joint, then frames 1 m before
// and after the joint located through the mirror (processFrame, locateWallAlignment) from a perturbed pose, in DESIGN and
// in MAP mode, each info compared byte for byte with the C ABI's stage call (gm_wall_alignment_locate_points) on the frame's
// valid cloud.  Prints "gm_wall_alignment_locate_test ok" on success.
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

// the pose of a sensor at chainage s0 (0.15 m up, 0.1 m aside) and n points of the tube around it, in sensor coordinates
static void frame(const gm_wall_params &prm, const std::vector<gm_wall_element> &el, double s0, unsigned n, unsigned long long &seed,
                  double pose[12], std::vector<float> &rows)
{
    const uint32_t ne = (uint32_t)el.size();
    double P[3], pu[3], pv[3], u[3], v[3], a[3];
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 0.0, P) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 0.0, 1.0, pu) == GM_OK);
    EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s0, 1.5707963267948966, 1.0, pv) == GM_OK);
    for (int c = 0; c < 3; ++c) { u[c] = pu[c] - P[c]; v[c] = pv[c] - P[c]; }
    a[0] = u[1] * v[2] - u[2] * v[1]; a[1] = u[2] * v[0] - u[0] * v[2]; a[2] = u[0] * v[1] - u[1] * v[0];
    for (int r = 0; r < 3; ++r) {
        pose[4 * r] = a[r]; pose[4 * r + 1] = -v[r]; pose[4 * r + 2] = u[r];
        pose[4 * r + 3] = P[r] + 0.15 * u[r] - 0.1 * v[r];
    }
    rows.assign(4 * (size_t)n, 0.0f);
    for (unsigned i = 0; i < n; ++i) {
        const double s = s0 - 4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed), rho = 2.0 + 0.01 * (uni(seed) - 0.5);
        double x[3];
        EXPECT(gm_wall_alignment_point(&prm, &el[0], ne, s, phi, rho, x) == GM_OK);
        for (int c = 0; c < 3; ++c)   // Rm^T (x - tr)
            rows[4 * (size_t)i + c] = (float)(pose[c] * (x[0] - pose[3]) + pose[4 + c] * (x[1] - pose[7]) + pose[8 + c] * (x[2] - pose[11]));
    }
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
        gm_wall_locate_params lp;
        gm_wall_locate_default_params(&lp);
        double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        bool refused = false;
        try { proc.locateWallAlignment(eye, lp); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);
        proc.createWallAlignment(prm, el);
        gm_wall_alignment *abi = 0;
        EXPECT(gm_wall_alignment_create(proc.ctx(), &prm, &el[0], ne, &abi) == GM_OK && abi);

        const unsigned n = 4000;
        unsigned long long seed = 7;
        double pose[12];
        std::vector<float> rows;
        // the survey: the tube around the joint at 40 m, into both alignments
        for (int f = 0; f < 4; ++f) {
            frame(prm, el, 37.0 + 2.0 * f, n, seed, pose, rows);
            std::vector<float> xyz(3 * (size_t)n);
            for (size_t i = 0; i < n; ++i) { xyz[3 * i] = rows[4 * i]; xyz[3 * i + 1] = rows[4 * i + 1]; xyz[3 * i + 2] = rows[4 * i + 2]; }
            EXPECT(gm_wall_alignment_add_points(proc.wallAlignment(), &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
            EXPECT(gm_wall_alignment_add_points(abi, &xyz[0], n, 0, pose, 0, 0, 0, 0) == GM_OK);
        }
        for (int f = 0; f < 2; ++f) {
            frame(prm, el, f ? 41.0 : 39.0, n, seed, pose, rows);
            double pin[12];
            std::memcpy(pin, pose, sizeof(pin));
            pin[7] += 0.04; pin[11] -= 0.03;                            // 4 cm and 3 cm off across the axis
            const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
            EXPECT(fr.n_valid > n / 2);
            const PointCloud cloud = proc.choppedCloud();
            const uint32_t nv = (uint32_t)cloud.size();
            std::vector<float> xyz(3 * (size_t)nv);
            for (size_t i = 0; i < nv; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
            // (both locates of the frame first: the stage call below takes the context's slot 0 for its own cloud)
            gm_wall_alignment_locate_info both[2];
            for (uint32_t ref = 0; ref < 2; ++ref) {
                lp.reference = ref;
                lp.min_count = 2;
                both[ref] = proc.locateWallAlignment(pin, lp);
            }
            for (uint32_t ref = 0; ref < 2; ++ref) {
                lp.reference = ref;
                const gm_wall_alignment_locate_info &li = both[ref];
                gm_wall_alignment_locate_info lj;
                EXPECT(gm_wall_alignment_locate_points(abi, &xyz[0], nv, 0, pin, &lp, &lj, 0, 0, 0) == GM_OK);
                EXPECT(li.struct_size == sizeof(li) && std::memcmp(&li, &lj, sizeof(li)) == 0);
                EXPECT(li.status == GM_LOCATE_OK && li.passes == 3 && li.n_points == nv && li.n_sides == 2);
                EXPECT(li.side_element[0] == 1 && li.side_element[1] == 2 && li.element == (uint32_t)(1 + f));
                EXPECT(li.side_kind[0] == GM_WALL_ELEMENT_CLOTHOID && li.side_kind[1] == GM_WALL_ELEMENT_ARC);
                EXPECT(li.pass[2].used > nv / 2);
                const double dy = li.pose[7] - pose[7], dz = li.pose[11] - pose[11];
                EXPECT(std::fabs(dy) < 5e-3 && std::fabs(dz) < 5e-3);   // from 4 cm and 3 cm
                std::printf("frame %d ref %u: %u valid, used %u, came back to %.1e, %.1e m\n", f, ref, nv, li.pass[2].used, dy, dz);
            }
        }
        gm_wall_alignment_destroy(abi);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_alignment_locate_test ok\n");
    return 0;
}
