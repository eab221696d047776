// gm_wall_objects_test -- the host mirror's objects of a check: an 80 x 90 wall map is filled with deterministic raw
// cells through gm_wall_map_add_raw, a synthetic tunnel frame with a strip moved out and a box standing in the profile
// goes through processFrame and Processor::checkWallMap, and Processor::wallCheckObjects is compared, byte for byte, with
// a direct gm_wall_map_check_objects call, with the stage call gm_wall_check_objects on the check's rows, and with a
// scalar C++ restatement of the rule of include/gm_hip.h (a flood fill over the flagged blocks) -- for two parameter
// sets.  Prints "gm_wall_objects_test ok" on success.
//
// gm_wall_objects_test --time FILE needs no device: it reads rows a caller fetched with gm_wall_map_get_check (FILE: int64
// anchor, uint32 n_stations, n_sectors, n_rows, repetitions, a gm_wall_object_params, then the rows), runs the scalar
// restatement on them and prints one JSON line with its wall times -- the host half of the path the device call replaces
// (tools/wall_objects_timing.py adds the copy).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <utility>
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

static uint32_t ordered(float e)
{
    uint32_t b;
    std::memcpy(&b, &e, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static float unordered(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// (int64) rint(x scale): one fp32 product, rounded to nearest even (every value here is far inside the int32 range)
static int64_t fix(float x, float scale)
{
    volatile float p = x * scale;
    return (int64_t)std::nearbyint((double)p);
}

static const unsigned kN = 80, kNs = 90;

// the rule, one row at a time; the list in (label, sign) order, object_of_row beside it
static std::vector<gm_wall_object> restate(const std::vector<gm_wall_check_point> &rows, int64_t anchor, const gm_wall_object_params &op,
                                           gm_wall_objects_info &info, std::vector<int32_t> &of_row, unsigned n_st = kN, unsigned n_sec = kNs)
{
    std::memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    info.n_rows = (uint32_t)rows.size();
    of_row.assign(rows.size(), -1);
    const int64_t H = op.half_window_stations, bs = op.block_stations, bk = op.block_sectors;
    const int64_t NK = (n_sec + bk - 1) / bk;
    const int64_t lo = std::max<int64_t>(0, anchor - H), hi = std::min<int64_t>(n_st, anchor + H);
    int64_t J0 = 0, nJ = 0;
    if (lo < hi) {
        J0 = lo / bs;
        nJ = (hi - 1) / bs - J0 + 1;
        info.station0 = (uint32_t)(J0 * bs);
        info.n_stations = (uint32_t)(std::min<int64_t>((J0 + nJ) * bs, n_st) - J0 * bs);
    }
    info.blocks_stations = (uint32_t)nJ;
    info.blocks_sectors = (uint32_t)NK;
    typedef std::pair<int, std::pair<int64_t, int64_t> > Key;   // plane, (J - J0, K)
    std::map<Key, std::vector<size_t> > members;
    for (size_t i = 0; i < rows.size(); ++i) {
        const gm_wall_check_point &r = rows[i];
        const int64_t dq = fix(r.delta, 1048576.0f);
        if (r.cell < 0 || r.cell >= (int32_t)(n_st * n_sec) || dq == 0 || !std::isfinite(r.x) || !std::isfinite(r.y) || !std::isfinite(r.z) ||
            !std::isfinite(r.e)) {
            ++info.rejected;
            continue;
        }
        const int64_t J = r.cell / n_sec / bs, K = r.cell % n_sec / bk;
        if (J < J0 || J >= J0 + nJ) { ++info.outside_window; continue; }
        members[Key(dq > 0 ? 1 : 0, std::make_pair(J - J0, K))].push_back(i);
    }
    std::set<Key> flagged, seen;
    for (std::map<Key, std::vector<size_t> >::const_iterator it = members.begin(); it != members.end(); ++it) {
        if (it->second.size() >= op.min_block_points) {
            flagged.insert(it->first);
            if (it->first.first) ++info.flagged_pos; else ++info.flagged_neg;
        } else {
            info.sparse += (uint32_t)it->second.size();
        }
    }
    std::vector<std::pair<std::pair<uint32_t, int32_t>, std::pair<gm_wall_object, std::vector<size_t> > > > found;
    for (std::set<Key>::const_iterator it = flagged.begin(); it != flagged.end(); ++it) {
        if (seen.count(*it)) continue;
        std::vector<Key> comp, stack(1, *it);
        seen.insert(*it);
        while (!stack.empty()) {
            const Key k = stack.back();
            stack.pop_back();
            comp.push_back(k);
            for (int dj = -1; dj <= 1; ++dj)
                for (int dk = -1; dk <= 1; ++dk) {
                    if ((!dj && !dk) || (op.connectivity == 4 && dj && dk)) continue;
                    const int64_t J = k.second.first + dj, K = ((k.second.second + dk) % NK + NK) % NK;
                    if (J < 0 || J >= nJ) continue;
                    const Key nb(k.first, std::make_pair(J, K));
                    if (flagged.count(nb) && !seen.count(nb)) { seen.insert(nb); stack.push_back(nb); }
                }
        }
        ++info.components;
        std::vector<size_t> idx;
        int64_t label = -1;
        for (size_t c = 0; c < comp.size(); ++c) {
            const std::vector<size_t> &v = members[comp[c]];
            idx.insert(idx.end(), v.begin(), v.end());
            const int64_t B = (J0 + comp[c].second.first) * NK + comp[c].second.second;
            if (label < 0 || B < label) label = B;
        }
        if (idx.size() < op.min_points) { info.small += (uint32_t)idx.size(); continue; }
        info.in_object += (uint32_t)idx.size();
        gm_wall_object o;
        std::memset(&o, 0, sizeof(o));
        o.label = (uint32_t)label;
        o.sign = comp[0].first ? 1 : -1;
        o.blocks = (uint32_t)comp.size();
        o.points = idx.size();
        uint64_t best = 0;
        uint32_t kx[3] = {0, 0, 0}, kn[3] = {0, 0, 0}, ke_min = 0, ke_max = 0, smin = ~0u, smax = 0, kmin = ~0u, kmax = 0, tmin = ~0u, tmax = 0;
        for (size_t c = 0; c < idx.size(); ++c) {
            const gm_wall_check_point &r = rows[idx[c]];
            const int64_t dq = fix(r.delta, 1048576.0f);
            const uint32_t j = (uint32_t)r.cell / n_sec, k = (uint32_t)r.cell % n_sec, t = (k + n_sec / 2) % n_sec;
            const uint64_t key = ((uint64_t)(dq < 0 ? -dq : dq) << 32) | (uint32_t)~r.index;
            if (key > best) best = key;
            o.sum_delta += dq;
            o.sum_x += fix(r.x, 65536.0f); o.sum_y += fix(r.y, 65536.0f); o.sum_z += fix(r.z, 65536.0f);
            smin = std::min(smin, j); smax = std::max(smax, j);
            kmin = std::min(kmin, k); kmax = std::max(kmax, k);
            tmin = std::min(tmin, t); tmax = std::max(tmax, t);
            const float xyz[3] = {r.x, r.y, r.z};
            for (int a = 0; a < 3; ++a) {
                kx[a] = std::max(kx[a], ordered(xyz[a]));
                kn[a] = std::max(kn[a], ~ordered(xyz[a]));
            }
            ke_max = std::max(ke_max, ordered(r.e));
            ke_min = std::max(ke_min, ~ordered(r.e));
        }
        o.peak_index = ~(uint32_t)best;
        o.peak = (int64_t)(best >> 32) * o.sign;
        o.station_min = smin; o.station_max = smax;
        o.sector_min = kmin; o.sector_max = kmax;
        o.sector_min_turned = tmin; o.sector_max_turned = tmax;
        for (int a = 0; a < 3; ++a) { o.box_min[a] = unordered(~kn[a]); o.box_max[a] = unordered(kx[a]); }
        o.e_min = unordered(~ke_min);
        o.e_max = unordered(ke_max);
        found.push_back(std::make_pair(std::make_pair(o.label, o.sign), std::make_pair(o, idx)));
    }
    std::sort(found.begin(), found.end(),
              [](const std::pair<std::pair<uint32_t, int32_t>, std::pair<gm_wall_object, std::vector<size_t> > > &a,
                 const std::pair<std::pair<uint32_t, int32_t>, std::pair<gm_wall_object, std::vector<size_t> > > &b) { return a.first < b.first; });
    std::vector<gm_wall_object> out;
    for (size_t p = 0; p < found.size(); ++p) {
        out.push_back(found[p].second.first);
        for (size_t c = 0; c < found[p].second.second.size(); ++c) of_row[found[p].second.second[c]] = (int32_t)p;
    }
    info.objects = (uint32_t)out.size();
    return out;
}

static bool same(const std::vector<gm_wall_object> &a, const std::vector<gm_wall_object> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(gm_wall_object)) == 0);
}
static bool same(const gm_wall_objects_info &a, const gm_wall_objects_info &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static int time_restatement(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); return 2; }
    int64_t anchor = 0;
    uint32_t head[4] = {0, 0, 0, 0};   // n_stations, n_sectors, n_rows, repetitions
    gm_wall_object_params op;
    bool ok = std::fread(&anchor, 8, 1, f) == 1 && std::fread(head, 4, 4, f) == 4 && std::fread(&op, sizeof(op), 1, f) == 1 &&
              op.struct_size == sizeof(op) && head[0] >= 1 && head[1] >= 1 && op.block_stations >= 1 && op.block_sectors >= 1;
    std::vector<gm_wall_check_point> rows(ok ? head[2] : 0);
    if (ok && head[2]) ok = std::fread(&rows[0], sizeof(gm_wall_check_point), head[2], f) == head[2];
    std::fclose(f);
    if (!ok) { std::printf("bad file %s\n", path); return 2; }
    std::printf("{\"rows\": %u, \"restate_ms\": [", head[2]);
    gm_wall_objects_info info;
    std::vector<int32_t> of_row;
    size_t objects = 0;
    for (uint32_t r = 0; r < (head[3] ? head[3] : 1u); ++r) {
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        objects = restate(rows, anchor, op, info, of_row, head[0], head[1]).size();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s%.3f", r ? ", " : "", ms);
    }
    std::printf("], \"objects\": %u, \"components\": %u, \"in_object\": %u}\n", (unsigned)objects, info.components, info.in_object);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::strcmp(argv[1], "--time") == 0) return time_restatement(argv[2]);
    try {
        EXPECT(sizeof(gm_wall_object) == 128 && sizeof(gm_wall_objects_info) == 64);
        gm_wall_object_params op;
        gm_wall_object_default_params(&op);
        EXPECT(op.struct_size == sizeof(gm_wall_object_params) && op.block_stations == 1 && op.block_sectors == 1 && op.min_block_points == 2 &&
               op.min_points == 8 && op.connectivity == 8 && op.half_window_stations == 128 && op.reserved == 0);
        gm_wall_check_params cp;
        gm_wall_check_default_params(&cp);
        cp.min_count = 4;
        cp.threshold = 0.04;
        gm_wall_params prm;
        gm_wall_default_params(&prm);
        prm.n_stations = kN;
        prm.n_sectors = kNs;
        prm.t_min = -10.0;
        const double pose[12] = {1, 0, 0, 0.125, 0, 1, 0, 0.0625, 0, 0, 1, -0.03125};

        Processor proc(5.0, 0.5, 0.25, 0.2, 0, GM_CFG_VOXEL_GRID);
        bool refused = false;
        try { proc.wallCheckObjects(op); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no map yet
        proc.createWallMap(prm);
        refused = false;
        try { proc.wallCheckObjects(op); } catch (const Error &e) { refused = e.status == GM_ERR_NOT_READY; }
        EXPECT(refused);   // no check yet

        // the survey: every cell filled, counts 4 .. 23, means within 2 cm of the design
        std::vector<gm_wall_raw_cell> raw(kN * kNs);
        std::memset(&raw[0], 0, raw.size() * sizeof(gm_wall_raw_cell));
        unsigned long long seed = 4711;
        for (size_t i = 0; i < raw.size(); ++i) {
            const uint32_t cnt = 4 + (uint32_t)(lcg(seed) % 20);
            const float lo = -0.05f * (float)uni(seed), hi = 0.05f * (float)uni(seed);
            const double mean = 0.4 * (lo + (hi - lo) * uni(seed));
            raw[i].sum = (int64_t)std::floor(mean * cnt * 1048576.0 + 0.5);
            raw[i].count = cnt;
            raw[i].min_key = ~ordered(lo);
            raw[i].max_key = ordered(hi);
        }
        EXPECT(gm_wall_map_add_raw(proc.wallMap(), 0, kN, &raw[0]) == GM_OK);

        // the frame: a tunnel of radius 2 along the design axis, 1 cm of noise; a strip of the ring (phi < 0.5) moved out by
        // 10 cm over the whole length, and a box 1.5 m long between phi = 3 and 3.6 standing 0.4 m inside the profile
        const unsigned n = 20000;
        std::vector<float> rows(4 * n);
        for (unsigned i = 0; i < n; ++i) {
            const double t = -4.5 + 9.0 * uni(seed), phi = 6.283185307179586 * uni(seed);
            double r = 2.0 + 0.02 * (uni(seed) - 0.5);
            if (phi < 0.5) r += 0.1;
            if (phi >= 3.0 && phi < 3.6 && t >= 0.5 && t < 2.0) r -= 0.4;
            rows[4 * i] = (float)(t - pose[3]); rows[4 * i + 1] = (float)(r * std::cos(phi) - pose[7]);
            rows[4 * i + 2] = (float)(r * std::sin(phi) - pose[11]);
            rows[4 * i + 3] = 0.0f;
        }
        const gm_frame_result fr = proc.processFrame(&rows[0], n, 16, 0, 4, 8);
        EXPECT(fr.n_valid > n / 2);
        gm_wall_check_info cinfo;
        const std::vector<gm_wall_check_point> changed = proc.checkWallMap(pose, cp, &cinfo);
        EXPECT(cinfo.changed_pos > 500 && cinfo.changed_neg > 100 && changed.size() == cinfo.changed_pos + cinfo.changed_neg);
        gm_wall_add_info ai;   // the anchor of that check: the per-add frame is a function of the pose alone
        gm_wall_map *scratch = 0;
        EXPECT(gm_wall_map_create(proc.ctx(), &prm, &scratch) == GM_OK);
        const float one[3] = {0.0f, 0.0f, 0.0f};
        EXPECT(gm_wall_map_add_points(scratch, one, 1, 0, pose, &ai, 0, 0) == GM_OK);

        for (int pass = 0; pass < 2; ++pass) {
            if (pass) { op.block_stations = 2; op.block_sectors = 3; op.connectivity = 4; op.min_points = 20; op.half_window_stations = 12; }
            gm_wall_objects_info info, info2, info3, info4;
            const std::vector<gm_wall_object> got = proc.wallCheckObjects(op, &info);
            // the ABI directly, with object_of_row
            uint32_t count = 0;
            EXPECT(gm_wall_map_check_objects(proc.wallMap(), 0, &op, &info2, 0, 0, &count, 0, 0) == GM_OK && count == got.size());
            std::vector<gm_wall_object> direct(count ? count : 1);
            std::vector<int32_t> of_row(changed.size() ? changed.size() : 1), of_row3, of_row4(changed.size() ? changed.size() : 1);
            EXPECT(gm_wall_map_check_objects(proc.wallMap(), 0, &op, &info2, &direct[0], count, &count, &of_row[0], (uint32_t)changed.size()) == GM_OK);
            direct.resize(count);
            of_row.resize(changed.size());
            of_row4.resize(changed.size());
            EXPECT(same(got, direct) && same(info, info2));
            // the scalar restatement on the check's rows
            const std::vector<gm_wall_object> want = restate(changed, ai.anchor_station, op, info3, of_row3);
            EXPECT(same(got, want) && same(info, info3) && of_row == of_row3);
            // the stage call on the same rows
            std::vector<gm_wall_object> staged(count ? count : 1);
            EXPECT(gm_wall_check_objects(proc.wallMap(), changed.empty() ? 0 : &changed[0], (uint32_t)changed.size(), ai.anchor_station, &op,
                                         &info4, &staged[0], count, &count, changed.empty() ? 0 : &of_row4[0]) == GM_OK);
            staged.resize(count);
            EXPECT(same(got, staged) && same(info, info4) && of_row == of_row4);
            EXPECT(info.rejected == 0 && info.rejected + info.outside_window + info.sparse + info.small + info.in_object == info.n_rows &&
                   info.n_rows == changed.size());
            for (size_t i = 1; i < got.size(); ++i)
                EXPECT(got[i - 1].label < got[i].label || (got[i - 1].label == got[i].label && got[i - 1].sign < got[i].sign));
            // the strip and the box are there
            unsigned strips = 0, boxes = 0;
            for (size_t i = 0; i < got.size(); ++i) {
                struct gm_wall_object_metrics mt;
                EXPECT(gm_wall_object_metrics(&prm, &op, &got[i], &mt) == GM_OK);
                if (got[i].sign > 0 && got[i].points > 300 && mt.mean_m > 0.07 && mt.mean_m < 0.13) ++strips;
                if (got[i].sign < 0 && got[i].points > 50 && mt.mean_m < -0.3 && mt.chainage_from >= 0.25 && mt.chainage_to <= 2.25) ++boxes;
            }
            std::printf("pass %d: %u rows, %u outside, %u sparse, %u small, %u in %u objects of %u components (%u strip, %u box)\n", pass,
                        info.n_rows, info.outside_window, info.sparse, info.small, info.in_object, info.objects, info.components, strips, boxes);
            EXPECT(strips == 1 && boxes == 1);
        }
        // the check's rows are still there, and the map was not changed
        gm_wall_check_info cinfo2;
        uint32_t count = 0;
        std::vector<gm_wall_check_point> again(changed.size() ? changed.size() : 1);
        EXPECT(gm_wall_map_get_check(proc.wallMap(), 0, &cinfo2, &again[0], (uint32_t)changed.size(), &count) == GM_OK && count == changed.size());
        EXPECT(std::memcmp(&again[0], &changed[0], changed.size() * sizeof(gm_wall_check_point)) == 0 && std::memcmp(&cinfo, &cinfo2, sizeof(cinfo)) == 0);
        std::vector<gm_wall_raw_cell> back(raw.size());
        uint64_t nc = 0;
        EXPECT(gm_wall_map_read_raw(proc.wallMap(), 0, kN, &back[0], back.size(), &nc) == GM_OK);
        EXPECT(std::memcmp(&back[0], &raw[0], raw.size() * sizeof(gm_wall_raw_cell)) == 0);
        op.connectivity = 5;
        refused = false;
        try { proc.wallCheckObjects(op); } catch (const Error &e) { refused = e.status == GM_ERR_INVALID_ARG; }
        EXPECT(refused);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_wall_objects_test ok\n");
    return 0;
}
