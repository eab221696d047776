// gm_cloud_output_test.cpp -- the page-locked /choppedCloud rows (Processor::enableCloudOutput) when a larger frame is
// submitted while an earlier one is still in flight: the buffers of every (device, slot) are replaced, and the earlier
// frame's cloud must still be the one choppedCloud() returns.  Two pipelines: one context with two slots, and two ranks
// on one device.  Every comparison is of bytes, against the blocking processFrame of the same rows on a context without
// the page-locked output.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gm_tunnel_processing.hpp"

using namespace gm_host;

static unsigned long long lcg = 88172645463325252ull;
static double urand() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0; }

// n points on a tunnel of radius 2 along x, 16-byte rows x, y, z, 0
static std::vector<float> tunnel(unsigned n)
{
    std::vector<float> rows((size_t)n * 4, 0.0f);
    for (unsigned i = 0; i < n; ++i) {
        const double t = -6 + 12 * urand(), th = 6.283185307179586 * urand(), rr = 2.0 + 0.01 * (urand() - 0.5);
        rows[4 * (size_t)i] = (float)t; rows[4 * (size_t)i + 1] = (float)(rr * std::cos(th)); rows[4 * (size_t)i + 2] = (float)(rr * std::sin(th));
    }
    return rows;
}

static int failures = 0;

static void same_cloud(const char *pipeline, const char *frame, const PointCloud &got, const PointCloud &want)
{
    if (got.size() != want.size()) {
        std::printf("FAILED %s: frame %s has %u rows, processFrame alone %u\n", pipeline, frame, (unsigned)got.size(), (unsigned)want.size());
        ++failures;
        return;
    }
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < want.size(); ++i)
        if (std::memcmp(&got[i], &want[i], sizeof(PointXYZ)) != 0) { if (!bad) first = i; ++bad; }
    if (bad) {
        std::printf("FAILED %s: frame %s: %u of %u rows differ from processFrame alone (first at row %u)\n", pipeline, frame,
                    (unsigned)bad, (unsigned)want.size(), (unsigned)first);
        ++failures;
    }
}

// A (small) and B (larger than the buffers) submitted back to back, then both waited for
static void grow_in_flight(const char *pipeline, Processor &p, const std::vector<float> &a, const std::vector<float> &b,
                           const PointCloud &want_a, const PointCloud &want_b)
{
    p.enableCloudOutput(1000);
    p.submitFrame(&a[0], (unsigned)(a.size() / 4), 16, 0, 4, 8);
    p.submitFrame(&b[0], (unsigned)(b.size() / 4), 16, 0, 4, 8);
    gm_frame_result r = p.waitFrame();
    if (r.n_in != a.size() / 4) { std::printf("FAILED %s: the first frame back is not A\n", pipeline); ++failures; }
    same_cloud(pipeline, "A", p.choppedCloud(), want_a);
    r = p.waitFrame();
    if (r.n_in != b.size() / 4) { std::printf("FAILED %s: the second frame back is not B\n", pipeline); ++failures; }
    same_cloud(pipeline, "B", p.choppedCloud(), want_b);
    // a third frame, smaller again, into the slot A used: its rows are the replaced ones
    p.submitFrame(&a[0], (unsigned)(a.size() / 4), 16, 0, 4, 8);
    p.waitFrame();
    same_cloud(pipeline, "A again", p.choppedCloud(), want_a);
}

int main()
{
    const std::vector<float> a = tunnel(800), b = tunnel(6000);
    try {
        PointCloud want_a, want_b;
        {
            Processor ref;   // no page-locked output: the cloud is fetched from the device
            gm_frame_result r = ref.processFrame(&a[0], 800, 16, 0, 4, 8);
            want_a = ref.choppedCloud();
            if (!r.n_valid || want_a.size() != r.n_valid) { std::printf("FAILED: frame A alone has no valid cloud\n"); return 1; }
            r = ref.processFrame(&b[0], 6000, 16, 0, 4, 8);
            want_b = ref.choppedCloud();
            if (r.n_valid <= 1000 || want_b.size() != r.n_valid) { std::printf("FAILED: frame B alone does not outgrow 1000 rows\n"); return 1; }
        }
        {
            const std::vector<int> devs(1, 0);
            Processor p(5.0, 0.5, 0.5, 0.2, devs, GM_CFG_DEFAULT, 2);
            grow_in_flight("one context, two slots", p, a, b, want_a, want_b);
        }
        if (failures) return 1;   // (first things first: the two-rank pipeline would only repeat it)
        {
            const std::vector<int> devs(2, 0);
            Processor p(5.0, 0.5, 0.5, 0.2, devs, GM_CFG_DEFAULT, 2);
            grow_in_flight("two ranks on one device", p, a, b, want_a, want_b);
        }
    } catch (const Error &e) {
        std::printf("FAILED: gm error %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    if (failures) return 1;
    std::printf("gm_cloud_output_test ok\n");
    return 0;
}
