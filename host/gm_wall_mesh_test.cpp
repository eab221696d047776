// gm_wall_mesh_test -- the host mirror's wall mesh: a 65 x 65 wall map (oblique design, chainage 5 km) with holes is
// filled through gm_wall_map_add_raw, and Processor::wallMapMesh is compared, byte for byte, with a direct
// gm_wall_map_mesh call, with Processor::wallMapCloud for the vertices, with gm_wall_mesh_triangulate on those vertices
// and with a scalar C++ restatement of the triangle rule of include/gm_hip.h -- at the map's resolution, decimated with
// ragged blocks, outward, unwrapped, with a step cut and through a sub-window.
// Prints "gm_wall_mesh_test ok" on success.
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

static uint32_t ordered(float e)
{
    uint32_t b;
    std::memcpy(&b, &e, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

static const unsigned kN = 65, kNs = 65;
static const uint32_t kDead = 0xFFFFFFFFu;

// the rule, one quad at a time, on the vertex list of an NJ x NK block grid
static std::vector<gm_wall_mesh_triangle> restate(const std::vector<gm_wall_cloud_point> &v, unsigned NJ, unsigned NK, uint32_t flags,
                                                  double max_step, gm_wall_mesh_info &info)
{
    std::vector<gm_wall_mesh_triangle> out;
    std::memset(&info, 0, sizeof(info));
    const bool wrap = NK >= 3 && !(flags & GM_WALL_MESH_NO_WRAP);
    const unsigned NKq = wrap ? NK : NK - 1;
    info.wrapped = wrap ? 1u : 0u;
    std::vector<uint32_t> index((size_t)NJ * NK, kDead);
    for (size_t i = 0; i < v.size(); ++i) index[v[i].block] = (uint32_t)i;
    const float step = (float)max_step;
    for (unsigned J = 0; J + 1 < NJ; ++J)
        for (unsigned K = 0; K < NKq; ++K) {
            const unsigned K1 = (K + 1) % NK;
            const uint32_t corner[4] = {index[J * NK + K], index[(J + 1) * NK + K], index[(J + 1) * NK + K1], index[J * NK + K1]};
            ++info.quads;
            unsigned alive = 0;
            for (int c = 0; c < 4; ++c) alive += corner[c] != kDead;
            uint32_t tri[2][3];
            unsigned nt = 0;
            if (alive == 4) {
                ++info.quads_two;
                const uint32_t a[3] = {corner[0], corner[1], corner[2]}, b[3] = {corner[0], corner[2], corner[3]};
                std::memcpy(tri[0], a, 12);
                std::memcpy(tri[1], b, 12);
                nt = 2;
            } else if (alive == 3) {
                ++info.quads_one;
                unsigned k = 0;
                for (int c = 0; c < 4; ++c)
                    if (corner[c] != kDead) tri[0][k++] = corner[c];
                nt = 1;
            } else {
                ++info.quads_none;
            }
            for (unsigned t = 0; t < nt; ++t) {
                bool cut = false;
                for (int x = 0; x < 3 && max_step > 0.0; ++x)
                    for (int y = x + 1; y < 3; ++y) {
                        volatile float d = v[tri[t][x]].mean - v[tri[t][y]].mean;
                        cut = cut || std::fabs(d) > step;
                    }
                if (cut) { ++info.cut_by_step; continue; }
                gm_wall_mesh_triangle r;
                r.v[0] = tri[t][0];
                r.v[1] = (flags & GM_WALL_MESH_OUTWARD) ? tri[t][2] : tri[t][1];
                r.v[2] = (flags & GM_WALL_MESH_OUTWARD) ? tri[t][1] : tri[t][2];
                out.push_back(r);
            }
        }
    info.triangles = out.size();
    return out;
}

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(T)) == 0);
}
static bool same_counts(const gm_wall_mesh_info &a, const gm_wall_mesh_info &b)
{
    return a.wrapped == b.wrapped && a.quads == b.quads && a.quads_two == b.quads_two && a.quads_one == b.quads_one &&
           a.quads_none == b.quads_none && a.cut_by_step == b.cut_by_step && a.triangles == b.triangles;
}

int main()
{
    try {
        EXPECT(sizeof(gm_wall_mesh_triangle) == 12);
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = 5000.0;
        prm.station_length = 0.3;
        prm.radius = 3.1;
        prm.point[0] = 3.0; prm.point[1] = -1.0; prm.point[2] = 0.5;
        prm.direction[0] = 0.9; prm.direction[1] = 0.2; prm.direction[2] = -0.1;
        gm_wall_mesh_params mp;
        gm_wall_mesh_default_params(&mp);
        EXPECT(mp.struct_size == sizeof(gm_wall_mesh_params) && mp.flags == 0 && mp.max_step == 0.0 && mp.reserved == 0 &&
               mp.cloud.struct_size == sizeof(gm_wall_cloud_params) && mp.cloud.block_stations == 1 && mp.cloud.min_count == 1);

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        std::vector<gm_wall_cloud_point> verts;
        std::vector<gm_wall_mesh_triangle> tris;
        bool refused = false;
        try { proc.wallMapMesh(0, kN, mp, &verts, &tris); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        gm_wall_mesh_info info, info2, info3, info4;
        proc.wallMapMesh(0, kN, mp, &verts, &tris, &info);
        EXPECT(verts.empty() && tris.empty() && info.quads == 64 * 65 && info.quads_none == info.quads && info.wrapped == 1);

        // 70 % of the cells filled: holes of every shape; counts 1 .. 20, sums of both signs
        std::vector<gm_wall_raw_cell> raw(kN * kNs);
        std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
        unsigned long long seed = 4711;
        for (size_t i = 0; i < raw.size(); ++i) {
            if (lcg(seed) % 10 >= 7) continue;
            const uint32_t cnt = 1 + (uint32_t)(lcg(seed) % 20);
            const float lo = -0.25f * (float)(lcg(seed) % 1000) / 1000.0f, hi = 0.25f * (float)(lcg(seed) % 1000) / 1000.0f;
            const double mean = lo + (hi - lo) * (double)(lcg(seed) % 1000) / 1000.0;
            raw[i].sum = (int64_t)std::floor(mean * cnt * 1048576.0 + 0.5);
            raw[i].count = cnt;
            raw[i].min_key = ~ordered(lo);
            raw[i].max_key = ordered(hi);
        }
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);
        const gm_wall_info wi = proc.wallMapInfo();
        for (int i = 0; i < 3; ++i) mp.cloud.anchor[i] = wi.o[i] + 5000.0 * wi.a[i];

        struct Case { unsigned s0, n, bs, bk, min_count; uint32_t flags; double step; };
        const Case cases[] = {{0, kN, 1, 1, 1, 0, 0.0},
                              {0, kN, 1, 1, 8, GM_WALL_MESH_OUTWARD, 0.1},
                              {0, kN, 7, 5, 8, GM_WALL_MESH_NO_WRAP, 0.05},
                              {3, 40, 2, 3, 1, GM_WALL_MESH_OUTWARD | GM_WALL_MESH_NO_WRAP, 0.0},
                              {0, kN, 64, 64, 1, 0, 0.0},
                              {10, 55, 200, 5000, 1, 0, 0.0},
                              {60, 0, 4, 4, 1, 0, 0.0}};
        for (size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++t) {
            const Case &c = cases[t];
            mp.cloud.block_stations = c.bs; mp.cloud.block_sectors = c.bk; mp.cloud.min_count = c.min_count;
            mp.flags = c.flags; mp.max_step = c.step;
            proc.wallMapMesh(c.s0, c.n, mp, &verts, &tris, &info);
            // the vertices are the cloud's rows
            gm_wall_cloud_info ci;
            EXPECT(same(verts, proc.wallMapCloud(c.s0, c.n, mp.cloud, &ci)) && std::memcmp(&ci, &info.cloud, sizeof(ci)) == 0);
            // the ABI directly
            uint64_t nv = 0, nt = 0;
            EXPECT(gm_wall_map_mesh(proc.wallMap(), c.s0, c.n, &mp, &info2, 0, 0, 0, 0, &nv, &nt) == GM_OK && nv == verts.size() &&
                   nt == tris.size());
            std::vector<gm_wall_cloud_point> dv(nv ? nv : 1);
            std::vector<gm_wall_mesh_triangle> dt(nt ? nt : 1);
            EXPECT(gm_wall_map_mesh(proc.wallMap(), c.s0, c.n, &mp, &info2, &dv[0], nv, &dt[0], nt, &nv, &nt) == GM_OK);
            dv.resize(nv);
            dt.resize(nt);
            EXPECT(same(verts, dv) && same(tris, dt) && std::memcmp(&info, &info2, sizeof(info)) == 0);
            // the host-only rule on those vertices
            const unsigned NJ = info.cloud.blocks_stations, NK = info.cloud.blocks_sectors;
            uint64_t ht = 0;
            std::vector<gm_wall_mesh_triangle> hv(nt ? nt : 1);
            EXPECT(gm_wall_mesh_triangulate(NJ, NK, verts.empty() ? 0 : &verts[0], verts.size(), c.flags, c.step, &info3, &hv[0], hv.size(),
                                            &ht) == GM_OK && ht == nt);
            hv.resize(ht);
            EXPECT(same(tris, hv) && same_counts(info, info3));
            // the rule restated
            const std::vector<gm_wall_mesh_triangle> want = restate(verts, NJ, NK ? NK : 1, c.flags, c.step, info4);
            EXPECT(same(tris, want) && same_counts(info, info4));
            EXPECT(info.quads == info.quads_two + info.quads_one + info.quads_none);
            EXPECT(info.triangles == 2 * info.quads_two + info.quads_one - info.cut_by_step && info.triangles == tris.size());
            for (size_t i = 0; i < tris.size(); ++i) EXPECT(tris[i].v[0] < nv && tris[i].v[1] < nv && tris[i].v[2] < nv);
            std::printf("case %zu: window %u+%u, blocks %ux%u -> %llu vertices, %llu quads (%llu two, %llu one, %llu none), %llu cut, %llu triangles\n",
                        t, c.s0, c.n, c.bs, c.bk, (unsigned long long)nv, (unsigned long long)info.quads, (unsigned long long)info.quads_two,
                        (unsigned long long)info.quads_one, (unsigned long long)info.quads_none, (unsigned long long)info.cut_by_step,
                        (unsigned long long)info.triangles);
            if (t == 0) EXPECT(info.quads == 64 * 65 && info.quads_two > 500 && info.quads_one > 500 && info.quads_none > 500 && info.wrapped == 1);
            if (t == 1) EXPECT(info.cut_by_step > 0);
            if (t == 2) EXPECT(info.wrapped == 0 && info.quads == 9 * 12);
            if (t == 5) EXPECT(nv == 1 && info.quads == 0 && tris.empty());
            if (t == 6) EXPECT(nv == 0 && info.quads == 0 && tris.empty());
        }
        // either output alone
        mp.flags = 0; mp.max_step = 0.0; mp.cloud.block_stations = 1; mp.cloud.block_sectors = 1; mp.cloud.min_count = 1;
        std::vector<gm_wall_cloud_point> v2;
        std::vector<gm_wall_mesh_triangle> t2;
        proc.wallMapMesh(0, kN, mp, &verts, &tris);
        proc.wallMapMesh(0, kN, mp, &v2, 0);
        proc.wallMapMesh(0, kN, mp, 0, &t2);
        EXPECT(same(verts, v2) && same(tris, t2) && !tris.empty());
        // the map was not changed
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK && nc == back.size());
        EXPECT(std::memcmp(&back[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        refused = false;
        try { proc.wallMapMesh(64, 2, mp, &verts, &tris); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
        mp.flags = 4;
        refused = false;
        try { proc.wallMapMesh(0, kN, mp, &verts, &tris); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_mesh_test ok\n");
    return 0;
}
