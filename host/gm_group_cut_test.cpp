// gm_group_cut_test.cpp -- the slab cut of a group (csrc/gm_group_cut.hpp) on the CPU.  Plain g++, no device: the header
// is all of the library this program sees.  The thread count is an argument of the cut, so its threaded passes run here
// at a few thousand rows.  Built twice by tests/test_host_group_cut.py, with -fsanitize=address,undefined and with
// -fsanitize=thread: a row written out of bounds, or a word two threads share, ends the program.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../geometric_mapping_amd/csrc/gm_group_cut.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

namespace {
const double kInf = std::numeric_limits<double>::infinity();
const float kNegInfF = -std::numeric_limits<float>::infinity();

gm_config config(double bound, double leaf, double radius)
{
    gm_config c;
    std::memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.flags = GM_CFG_VOXEL_GRID;
    c.boxFilterBound = bound; c.voxelGridLeafSize = leaf; c.neighborRadius = radius;
    return c;
}

// rows of `step` bytes with x, y, z at ox, oy, oz; every other byte is a pattern of the row's index
struct Frame {
    std::vector<uint8_t> bytes;
    uint32_t n = 0, step = 16, ox = 0, oy = 4, oz = 8, flags = 0;
    void add(float x, float y, float z)
    {
        const size_t at = bytes.size();
        bytes.resize(at + step);
        for (uint32_t k = 0; k < step; ++k) bytes[at + k] = (uint8_t)(n * 7u + k * 13u + 1u);
        std::memcpy(&bytes[at + ox], &x, 4); std::memcpy(&bytes[at + oy], &y, 4); std::memcpy(&bytes[at + oz], &z, 4);
        ++n;
    }
    float x(uint32_t i) const { return gm::load_f32(&bytes[(size_t)i * step + ox], (flags & GM_CLOUD_BIGENDIAN) != 0); }
    float y(uint32_t i) const { return gm::load_f32(&bytes[(size_t)i * step + oy], (flags & GM_CLOUD_BIGENDIAN) != 0); }
    float z(uint32_t i) const { return gm::load_f32(&bytes[(size_t)i * step + oz], (flags & GM_CLOUD_BIGENDIAN) != 0); }
    gm_cloud cloud() const { return gm_cloud{n ? bytes.data() : nullptr, n, step, ox, oy, oz, flags}; }
};

uint32_t g_lcg = 12345u;
float uniform(float lo, float hi)   // fixed-seed LCG (Numerical Recipes), 24 bits per draw
{
    g_lcg = g_lcg * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(g_lcg >> 8) * (1.0f / 16777216.0f);
}

// a tunnel-like cloud: x over most of the box, denser in the middle
void fill_random(Frame &f, uint32_t n, float half)
{
    for (uint32_t i = 0; i < n; ++i) {
        const float x = (i & 1) ? uniform(-half, half) : uniform(-0.3f * half, 0.3f * half);
        f.add(x, uniform(-half, half), uniform(-half, half));
    }
}

struct Cut {
    gm::CutPlan plan;
    std::vector<std::vector<uint8_t>> rows;
    std::vector<std::vector<uint32_t>> ids;
};

// both calls of the cut, with the caller's allocation between them: exactly the sizes the plan names
Cut run_cut(const gm_config &cfg, uint32_t R, const Frame &f, uint32_t T)
{
    Cut c;
    std::vector<float> xs;
    const gm_cloud cloud = f.cloud();
    gm::cut_plan(cfg, R, cloud, T, xs, c.plan);
    c.rows.resize(R); c.ids.resize(R);
    std::vector<uint8_t *> rows(R);
    std::vector<uint32_t *> ids(R);
    for (uint32_t r = 0; r < R; ++r) {
        c.rows[r].resize((size_t)c.plan.total[r] * f.step);
        c.ids[r].resize(c.plan.total[r]);
        rows[r] = c.rows[r].data(); ids[r] = c.ids[r].data();
    }
    gm::cut_scatter(cloud, T, xs, c.plan, rows.data(), ids.data());
    return c;
}

bool same_edges(const gm::CutPlan &a, const gm::CutPlan &b)
{
    return a.edges.size() == b.edges.size() && std::memcmp(a.edges.data(), b.edges.data(), a.edges.size() * sizeof(double)) == 0;
}
bool same_cut(const Cut &a, const Cut &b)
{
    return same_edges(a.plan, b.plan) && a.plan.on_lattice == b.plan.on_lattice && a.plan.n_inside == b.plan.n_inside &&
           a.plan.total == b.plan.total && a.rows == b.rows && a.ids == b.ids;
}

// the cut's contract restated with plain loops: n_inside, who takes which row, rows verbatim and in input order
int check_membership(const gm_config &cfg, uint32_t R, const Frame &f, const Cut &c)
{
    const float lo = (float)-cfg.boxFilterBound, hi = (float)cfg.boxFilterBound;
    const double halo = 1.01 * cfg.neighborRadius;
    REQUIRE(c.plan.edges.size() == (size_t)R + 1 && c.plan.edges[0] == -kInf && c.plan.edges[R] == kInf);
    for (uint32_t r = 0; r < R; ++r) REQUIRE(c.plan.edges[r] <= c.plan.edges[r + 1]);
    uint32_t inside = 0;
    for (uint32_t i = 0; i < f.n; ++i) {
        const float x = f.x(i), y = f.y(i), z = f.z(i);
        if (std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi) ++inside;
    }
    REQUIRE(c.plan.n_inside == inside);
    for (uint32_t r = 0; r < R; ++r) {
        std::vector<uint32_t> want;
        for (uint32_t i = 0; i < f.n; ++i) {
            const double x = (double)f.x(i);
            if (x >= c.plan.edges[r] - halo && x < c.plan.edges[r + 1] + halo) want.push_back(i);   // (ascending by construction)
        }
        REQUIRE(c.plan.total[r] == want.size() && c.ids[r] == want);
        for (size_t j = 0; j + 1 < c.ids[r].size(); ++j) REQUIRE(c.ids[r][j] < c.ids[r][j + 1]);
        for (size_t j = 0; j < c.ids[r].size(); ++j)
            REQUIRE(std::memcmp(&c.rows[r][j * f.step], &f.bytes[(size_t)c.ids[r][j] * f.step], f.step) == 0);
    }
    return 0;
}

// every inner edge is the smallest float of a lattice cell; *k_out: that cell
int check_on_plane(double edge, float inv_leaf, long long *k_out)
{
    const float e = (float)edge;
    REQUIRE((double)e == edge);
    const long long k = gm::lattice_cell(e, inv_leaf);
    REQUIRE(gm::lattice_cell(nextafterf(e, kNegInfF), inv_leaf) == k - 1);
    *k_out = k;
    return 0;
}

// bound 5, leaf 0.5, 4 ranks, no halo, x = -1.75, -1.25, ..., 1.75.  inv_leaf = 2, the box has cells -10 .. 10 (21 >= 16:
// on the lattice), the rows sit in cells -4 .. 3, one each.  8 rows in the box: the running count reaches 2 = 8 * 1/4
// behind cell -3, 4 behind cell -1, 6 behind cell 1, so the edges are the planes below cells -2, 0 and 2: x = -1, 0, 1.
int test_hand_derived()
{
    Frame f;
    for (int i = 0; i < 8; ++i) f.add(-1.75f + 0.5f * (float)i, 0.f, 0.f);
    const gm_config cfg = config(5.0, 0.5, 0.0);
    for (uint32_t T : {1u, 3u}) {
        const Cut c = run_cut(cfg, 4, f, T);
        REQUIRE(c.plan.on_lattice && c.plan.n_inside == 8 && c.plan.halo == 0.0);
        REQUIRE(c.plan.edges == (std::vector<double>{-kInf, -1.0, 0.0, 1.0, kInf}));
        REQUIRE(c.plan.total == (std::vector<uint32_t>{2, 2, 2, 2}));
        for (uint32_t r = 0; r < 4; ++r) REQUIRE(c.ids[r] == (std::vector<uint32_t>{2 * r, 2 * r + 1}));
        const long long cell[3] = {-2, 0, 2};
        for (int g = 1; g < 4; ++g) {
            long long k;
            if (check_on_plane(c.plan.edges[g], 2.0f, &k)) return 1;
            REQUIRE(k == cell[g - 1]);
        }
        if (check_membership(cfg, 4, f, c)) return 1;
    }
    return 0;
}

// lattice_plane(k) is the first float of cell k, for a leaf that is a power of two and for one that is not; and the
// edges of a random frame lie on such planes
int test_lattice_planes()
{
    for (double leaf : {0.5, 0.3}) {
        const float inv = 1.0f / (float)leaf;
        for (long long k = -40; k <= 40; ++k) {
            const float e = gm::lattice_plane(k, inv);
            REQUIRE(gm::lattice_cell(e, inv) == k && gm::lattice_cell(nextafterf(e, kNegInfF), inv) == k - 1);
        }
        Frame f;
        fill_random(f, 2000, 5.0f);
        const gm_config cfg = config(5.0, leaf, 0.1);
        const Cut c = run_cut(cfg, 4, f, 2);
        REQUIRE(c.plan.on_lattice);
        for (int g = 1; g < 4; ++g) {
            long long k;
            if (check_on_plane(c.plan.edges[g], inv, &k)) return 1;
        }
        REQUIRE(c.plan.edges[1] < c.plan.edges[3]);   // (the frame spreads over many cells: the cut is a real one)
        if (check_membership(cfg, 4, f, c)) return 1;
    }
    return 0;
}

// every thread count gives the bytes of one thread, more threads than rows included
int test_thread_invariance()
{
    const gm_config cfg = config(5.0, 0.5, 0.25);
    for (uint32_t n : {3001u, 5u}) {
        Frame f;
        fill_random(f, n, 5.5f);   // (some rows outside the box)
        const Cut one = run_cut(cfg, 4, f, 1);
        if (check_membership(cfg, 4, f, one)) return 1;
        for (uint32_t T : {2u, 3u, 7u, 16u}) REQUIRE(same_cut(run_cut(cfg, 4, f, T), one));
    }
    return 0;
}

// with a halo, rows near an edge go to both neighbours; a NaN x goes nowhere; a row out of the box in y only is sent
// (membership looks at x alone) but is not one of n_inside
int test_membership()
{
    const gm_config cfg = config(5.0, 0.5, 0.2);
    Frame f;
    fill_random(f, 1500, 5.0f);
    const uint32_t i_nan = f.n;
    f.add(std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f);
    const uint32_t i_yout = f.n;
    f.add(0.1f, 7.f, 0.f);
    fill_random(f, 1500, 5.0f);
    const Cut c = run_cut(cfg, 4, f, 3);
    if (check_membership(cfg, 4, f, c)) return 1;
    REQUIRE(c.plan.n_inside == f.n - 2 && c.plan.halo == 1.01 * 0.2);
    std::vector<uint32_t> times(f.n, 0u);
    for (uint32_t r = 0; r < 4; ++r)
        for (uint32_t id : c.ids[r]) ++times[id];
    uint32_t twice = 0;
    for (uint32_t i = 0; i < f.n; ++i) {
        REQUIRE(times[i] <= 2 && (times[i] >= 1 || i == i_nan));
        if (times[i] == 2) {   // within the halo of an inner edge
            ++twice;
            bool near = false;
            for (int g = 1; g < 4; ++g) near = near || std::fabs((double)f.x(i) - c.plan.edges[g]) <= c.plan.halo;
            REQUIRE(near);
        }
    }
    REQUIRE(twice > 0 && times[i_nan] == 0 && times[i_yout] >= 1);
    // the interval is half open: without a halo a row exactly on edge g belongs to rank g alone, the float below it to
    // rank g - 1 alone.  (Rows out of the box in y: they are sent but do not move the edges.)
    const gm_config cfg0 = config(5.0, 0.5, 0.0);
    const Cut before = run_cut(cfg0, 4, f, 2);
    const uint32_t first = f.n;
    for (int g = 1; g < 4; ++g) {
        f.add((float)before.plan.edges[g], 7.f, 0.f);
        f.add(nextafterf((float)before.plan.edges[g], kNegInfF), 7.f, 0.f);
    }
    const Cut c0 = run_cut(cfg0, 4, f, 2);
    REQUIRE(same_edges(c0.plan, before.plan) && c0.plan.n_inside == before.plan.n_inside);
    if (check_membership(cfg0, 4, f, c0)) return 1;
    for (uint32_t g = 1; g < 4; ++g)
        for (uint32_t r = 0; r < 4; ++r) {
            const std::vector<uint32_t> &ids = c0.ids[r];
            REQUIRE(std::binary_search(ids.begin(), ids.end(), first + 2 * (g - 1)) == (r == g));
            REQUIRE(std::binary_search(ids.begin(), ids.end(), first + 2 * (g - 1) + 1) == (r == g - 1));
        }
    return 0;
}

// 32-byte rows with x, y, z at 4, 12, 20, little- and big-endian: the same edges and ids, rows copied verbatim
int test_row_formats()
{
    const gm_config cfg = config(5.0, 0.5, 0.2);
    Frame le;
    le.step = 32; le.ox = 4; le.oy = 12; le.oz = 20;
    fill_random(le, 1200, 5.2f);
    Frame be = le;
    be.flags = GM_CLOUD_BIGENDIAN;
    for (uint32_t i = 0; i < be.n; ++i)
        for (uint32_t o : {be.ox, be.oy, be.oz}) {
            uint8_t *p = &be.bytes[(size_t)i * be.step + o];
            std::swap(p[0], p[3]); std::swap(p[1], p[2]);
        }
    const Cut a = run_cut(cfg, 4, le, 3), b = run_cut(cfg, 4, be, 3);
    if (check_membership(cfg, 4, le, a) || check_membership(cfg, 4, be, b)) return 1;
    REQUIRE(same_edges(a.plan, b.plan) && a.plan.total == b.plan.total && a.plan.n_inside == b.plan.n_inside && a.ids == b.ids);
    Frame plain;   // the same points in 16-byte rows: the row format does not move the cut
    for (uint32_t i = 0; i < le.n; ++i) plain.add(le.x(i), le.y(i), le.z(i));
    const Cut p = run_cut(cfg, 4, plain, 1);
    REQUIRE(same_edges(a.plan, p.plan) && a.ids == p.ids);
    return 0;
}

int test_degenerate()
{
    {   // an empty frame: every inner edge at 0, nothing sent
        const gm_config cfg = config(5.0, 0.5, 0.2);
        Frame f;
        for (uint32_t T : {1u, 4u}) {
            const Cut c = run_cut(cfg, 4, f, T);
            REQUIRE(c.plan.edges == (std::vector<double>{-kInf, 0.0, 0.0, 0.0, kInf}));
            REQUIRE(c.plan.n_inside == 0 && c.plan.total == (std::vector<uint32_t>{0, 0, 0, 0}));
        }
    }
    {   // every point in one lattice cell: the inner edges coincide behind it, nothing is lost
        const gm_config cfg = config(5.0, 0.5, 0.0);
        Frame f;
        for (int i = 0; i < 300; ++i) f.add(uniform(1.01f, 1.49f), uniform(-1.f, 1.f), 0.f);
        const Cut c = run_cut(cfg, 4, f, 3);
        REQUIRE(c.plan.edges == (std::vector<double>{-kInf, 1.5, 1.5, 1.5, kInf}));
        REQUIRE(c.plan.total == (std::vector<uint32_t>{300, 0, 0, 0}));
        if (check_membership(cfg, 4, f, c)) return 1;
    }
    {   // one rank takes every row but the NaN one
        const gm_config cfg = config(5.0, 0.5, 0.2);
        Frame f;
        fill_random(f, 700, 6.0f);
        f.add(std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f);
        const Cut c = run_cut(cfg, 1, f, 3);
        REQUIRE(c.plan.edges == (std::vector<double>{-kInf, kInf}) && c.plan.total == (std::vector<uint32_t>{700}));
        if (check_membership(cfg, 1, f, c)) return 1;
    }
    {   // leaf 50 in a box of +-5: two cells, too coarse to cut along.  4096 uniform bins over [lo, hi]: the edge behind
        // bin b is the float of lo + (b + 1) / ubin, b the first bin at which the running count reaches g / R
        const gm_config cfg = config(5.0, 50.0, 0.2);
        const uint32_t R = 4;
        Frame f;
        fill_random(f, 2500, 5.5f);
        const Cut c = run_cut(cfg, R, f, 3);
        REQUIRE(!c.plan.on_lattice);
        const double lo = -5.0, ubin = 4096.0 / 10.0;
        std::vector<uint32_t> hist(4096, 0u);
        uint64_t n_in = 0;
        for (uint32_t i = 0; i < f.n; ++i) {
            const float x = f.x(i), y = f.y(i), z = f.z(i);
            if (std::fabs(x) > 5.f || std::fabs(y) > 5.f || std::fabs(z) > 5.f) continue;
            const uint32_t b = (uint32_t)(((double)x - lo) * ubin);
            ++hist[b < 4096u ? b : 4095u];
            ++n_in;
        }
        REQUIRE(c.plan.n_inside == n_in);
        uint64_t run = 0;
        uint32_t g = 1;
        for (uint32_t b = 0; b < 4096 && g < R; ++b) {
            run += hist[b];
            for (; g < R && run * R >= n_in * g; ++g) REQUIRE(c.plan.edges[g] == (double)(float)(lo + (double)(b + 1) / ubin));
        }
        REQUIRE(g == R);
        if (check_membership(cfg, R, f, c)) return 1;
        REQUIRE(same_cut(run_cut(cfg, R, f, 1), c));
    }
    {   // leaf 0.001 in a box of +-600: about 1.2 M cells, more than 2^20 bins, so two cells share a bin and every edge
        // lies an even number of cells above the box's first cell
        const gm_config cfg = config(600.0, 0.001, 0.05);
        const float inv = 1.0f / (float)0.001;
        const long long c_lo = gm::lattice_cell(-600.f, inv), ncell = gm::lattice_cell(600.f, inv) - c_lo + 1;
        REQUIRE(ncell > (1ll << 20) && ncell <= (1ll << 21));
        Frame f;
        fill_random(f, 2000, 600.0f);
        const Cut c = run_cut(cfg, 4, f, 3);
        REQUIRE(c.plan.on_lattice && c.plan.edges[1] < c.plan.edges[2] && c.plan.edges[2] < c.plan.edges[3]);
        for (int g = 1; g < 4; ++g) {
            long long k;
            if (check_on_plane(c.plan.edges[g], inv, &k)) return 1;
            REQUIRE((k - c_lo) % 2 == 0);
        }
        if (check_membership(cfg, 4, f, c)) return 1;
        REQUIRE(same_cut(run_cut(cfg, 4, f, 1), c));
    }
    return 0;
}
}  // namespace

int main()
{
    if (test_hand_derived() || test_lattice_planes() || test_thread_invariance() || test_membership() || test_row_formats() ||
        test_degenerate())
        return 1;
    std::printf("gm_group_cut_test ok\n");
    return 0;
}
