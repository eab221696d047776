// gm_wall_mesh_host_test -- the device-free half of the wall mesh (csrc/gm_wall_host.hip: gm_wall_mesh_triangulate,
// gm_wall_mesh_write_ply, gm_wall_mesh_default_params) as a stand-alone program: linked with that one source file and
// nothing else of the library, it initialises no device, and tests/test_host_wall_mesh_pure.py builds it with the host
// sanitizers.  Every buffer is heap-allocated at exactly the size the call is told, so a write or a read past an end is
// seen.  Prints "gm_wall_mesh_host_test ok" on success.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gm_hip.h"

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

// the alive blocks of an NJ x NK grid at `fill` tenths, means in +-0.1
static std::vector<gm_wall_cloud_point> vertices(unsigned NJ, unsigned NK, unsigned fill, unsigned long long seed)
{
    std::vector<gm_wall_cloud_point> v;
    for (unsigned b = 0; b < NJ * NK; ++b) {
        if (lcg(seed) % 10 >= fill) continue;
        gm_wall_cloud_point p;
        std::memset(&p, 0, sizeof(p));
        p.block = b;
        p.mean = 0.1f * ((float)(lcg(seed) % 2001) - 1000.0f) / 1000.0f;
        p.x = (float)b;
        v.push_back(p);
    }
    return v;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    gm_wall_mesh_params mp;
    gm_wall_mesh_default_params(&mp);
    gm_wall_mesh_default_params(0);
    EXPECT(mp.struct_size == sizeof(mp) && mp.flags == 0 && mp.max_step == 0.0 && mp.cloud.struct_size == sizeof(mp.cloud));

    const unsigned grids[][2] = {{1, 1}, {1, 5}, {2, 1}, {2, 2}, {2, 3}, {3, 3}, {9, 33}, {40, 64}, {0, 7}};
    const uint32_t flags[] = {0, GM_WALL_MESH_OUTWARD, GM_WALL_MESH_NO_WRAP, GM_WALL_MESH_OUTWARD | GM_WALL_MESH_NO_WRAP};
    unsigned long long calls = 0;
    for (size_t gi = 0; gi < sizeof(grids) / sizeof(grids[0]); ++gi)
        for (unsigned fill = 0; fill <= 10; fill += 5)
            for (size_t fi = 0; fi < 4; ++fi)
                for (int cutting = 0; cutting < 2; ++cutting) {
                    const unsigned NJ = grids[gi][0], NK = grids[gi][1];
                    const std::vector<gm_wall_cloud_point> v = vertices(NJ, NK, fill, 17 + gi);
                    const double step = cutting ? 0.05 : 0.0;
                    gm_wall_mesh_info info, info2;
                    uint64_t n = 99;
                    EXPECT(gm_wall_mesh_triangulate(NJ, NK, v.empty() ? 0 : v.data(), v.size(), flags[fi], step, &info, 0, 0, &n) == GM_OK);
                    EXPECT(n == info.triangles && info.quads == info.quads_two + info.quads_one + info.quads_none);
                    EXPECT(info.triangles == 2 * info.quads_two + info.quads_one - info.cut_by_step);
                    const bool wrap = NK >= 3 && !(flags[fi] & GM_WALL_MESH_NO_WRAP);
                    EXPECT(info.wrapped == (wrap ? 1u : 0u) && info.quads == (uint64_t)(NJ ? NJ - 1 : 0) * (wrap ? NK : (NK ? NK - 1 : 0)));
                    if (fill == 10 && !cutting) EXPECT(info.triangles == 2 * info.quads);
                    if (fill == 0) EXPECT(info.triangles == 0 && info.quads_none == info.quads);
                    std::vector<gm_wall_mesh_triangle> t((size_t)n);   // exactly the count
                    uint64_t m = 0;
                    EXPECT(gm_wall_mesh_triangulate(NJ, NK, v.empty() ? 0 : v.data(), v.size(), flags[fi], step, &info2,
                                                    t.empty() ? 0 : t.data(), t.size(), &m) == GM_OK && m == n);
                    EXPECT(std::memcmp(&info, &info2, sizeof(info)) == 0);
                    for (size_t i = 0; i < t.size(); ++i) EXPECT(t[i].v[0] < v.size() && t[i].v[1] < v.size() && t[i].v[2] < v.size());
                    if (n > 1) {   // one short: nothing written
                        std::vector<gm_wall_mesh_triangle> s((size_t)n - 1);
                        std::memset(s.data(), 0x5A, s.size() * sizeof(gm_wall_mesh_triangle));
                        EXPECT(gm_wall_mesh_triangulate(NJ, NK, v.data(), v.size(), flags[fi], step, &info2, s.data(), s.size(), &m) ==
                               GM_ERR_CAPACITY && m == n);
                        EXPECT(s[0].v[0] == 0x5A5A5A5Au && s.back().v[2] == 0x5A5A5A5Au);
                    }
                    // the file, read back
                    const std::string path = dir + "/mesh.ply";
                    EXPECT(gm_wall_mesh_write_ply(path.c_str(), v.empty() ? 0 : v.data(), v.size(), t.empty() ? 0 : t.data(), t.size()) == GM_OK);
                    FILE *f = std::fopen(path.c_str(), "rb");
                    EXPECT(f != 0);
                    if (f) {
                        std::vector<char> blob(1 << 22);
                        const size_t got = std::fread(blob.data(), 1, blob.size(), f);
                        std::fclose(f);
                        const std::string all(blob.data(), got);
                        const size_t h = all.find("end_header\n");
                        EXPECT(h != std::string::npos && all.compare(0, 4, "ply\n") == 0);
                        const size_t body = h + 11;
                        EXPECT(got == body + 24 * v.size() + 13 * t.size());
                        for (size_t i = 0; i < v.size() && got >= body + 24 * v.size(); ++i) EXPECT(std::memcmp(&all[body + 24 * i], &v[i], 24) == 0);
                        for (size_t i = 0; i < t.size() && got == body + 24 * v.size() + 13 * t.size(); ++i) {
                            const char *r = &all[body + 24 * v.size() + 13 * i];
                            EXPECT(r[0] == 3 && std::memcmp(r + 1, t[i].v, 12) == 0);
                        }
                    }
                    ++calls;
                }
    // refusals
    gm_wall_mesh_info info;
    std::vector<gm_wall_cloud_point> v = vertices(3, 3, 10, 1);
    uint64_t n = 0;
    EXPECT(gm_wall_mesh_triangulate(3, 3, v.data(), v.size(), 4, 0.0, &info, 0, 0, &n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_mesh_triangulate(3, 3, v.data(), v.size(), 0, -1.0, &info, 0, 0, &n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_mesh_triangulate(3, 3, v.data(), v.size(), 0, 0.0, 0, 0, 0, &n) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_mesh_triangulate(3, 2, v.data(), v.size(), 0, 0.0, &info, 0, 0, &n) == GM_ERR_INVALID_ARG);   // blocks >= NJ NK
    v[4].block = 3;
    EXPECT(gm_wall_mesh_triangulate(3, 3, v.data(), v.size(), 0, 0.0, &info, 0, 0, &n) == GM_ERR_INVALID_ARG);   // not ascending
    gm_wall_mesh_triangle bad = {{0, 1, 9}};
    EXPECT(gm_wall_mesh_write_ply((dir + "/bad.ply").c_str(), v.data(), v.size(), &bad, 1) == GM_ERR_INVALID_ARG);
    EXPECT(gm_wall_mesh_write_ply((dir + "/no/such/dir/x.ply").c_str(), v.data(), v.size(), 0, 0) == GM_ERR_DEVICE);
    EXPECT(gm_wall_mesh_write_ply(0, v.data(), v.size(), 0, 0) == GM_ERR_INVALID_ARG);
    std::printf("%llu triangulations\n", calls);
    if (fails) return 1;
    std::printf("gm_wall_mesh_host_test ok\n");
    return 0;
}
