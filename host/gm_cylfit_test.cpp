// gm_cylfit_test -- the host mirror's cylinder regression: Processor::getCylinder (gm_fit_cylinder) on a synthetic half
// tube from a perturbed start, then the rvizCylinder overload that takes the fit.  Checks the fit against the analytic
// truth and the marker against the fit: position = fit.point, scale = 2 r (x, y), orientation maps z onto fit.axis.
// Prints "gm_cylfit_test ok" on success.  Usage: gm_cylfit_test [n_points]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gm_tunnel_processing.hpp"

using namespace gm_host;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
    } while (0)

// deterministic uniform [0, 1) (64-bit LCG, top 53 bits)
static double uni(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
}

int main(int argc, char **argv)
{
    const unsigned n = argc > 1 ? (unsigned)std::atoi(argv[1]) : 100000u;
    const double R = 2.0, tau = 0.03, pi = 3.14159265358979323846;
    // upper half of a tube of radius 2 along x, 10 m long, +-0.01 m uniform radial noise
    PointCloud cloud(n);
    unsigned long long s = 12345;
    for (unsigned i = 0; i < n; ++i) {
        const double x = -5.0 + 10.0 * uni(s), th = pi * uni(s), r = R + 0.02 * (uni(s) - 0.5);
        cloud[i].x = (float)x; cloud[i].y = (float)(r * std::cos(th)); cloud[i].z = (float)(r * std::sin(th)); cloud[i].pad = 0.f;
    }
    // start: axis tilted 0.04 rad, point 0.05 m off, radius 0.05 m too large
    const float init[7] = {0.f, 0.035f, -0.035f, (float)std::cos(0.04), (float)(std::sin(0.04) / std::sqrt(2.0)),
                           (float)(std::sin(0.04) / std::sqrt(2.0)), 2.05f};
    try {
        Processor proc;   // the launch file's parameters; stage calls need no RANSAC flag
        std::vector<uint8_t> inl;
        const gm_cylinder_fit f = proc.getCylinder(cloud, init, tau, std::vector<uint8_t>(), 0, &inl);
        EXPECT(f.struct_size == sizeof(gm_cylinder_fit));
        EXPECT(f.status == GM_FIT_OK && f.passes == 3);
        EXPECT(std::fabs(f.radius - R) < 1e-3);
        const double an = std::sqrt(f.axis[0] * f.axis[0] + f.axis[1] * f.axis[1] + f.axis[2] * f.axis[2]);
        EXPECT(std::fabs(an - 1.0) < 1e-9 && std::fabs(f.axis[0]) > std::cos(1e-3) && f.axis[0] > 0);
        EXPECT(std::sqrt(f.point[1] * f.point[1] + f.point[2] * f.point[2]) < 2e-3);
        unsigned cnt = 0;
        for (size_t i = 0; i < inl.size(); ++i) cnt += inl[i] ? 1u : 0u;
        EXPECT(inl.size() == n && cnt == f.inliers && cnt > 0.95 * n);

        Marker m;
        EXPECT(Processor::rvizCylinder(f, 12.0, m));
        EXPECT(m.type == MARKER_CYLINDER && m.action == MARKER_ADD && m.ns == "cylinder");
        for (int k = 0; k < 3; ++k) EXPECT(m.position[k] == f.point[k]);
        EXPECT(std::fabs(m.scale[0] - 2.0 * f.radius) < 1e-12 && std::fabs(m.scale[1] - 2.0 * f.radius) < 1e-12);
        EXPECT(m.scale[2] == 12.0);
        // rotate z = (0, 0, 1) by q = (x, y, z, w): the third column of the rotation matrix
        const double qx = m.orientation[0], qy = m.orientation[1], qz = m.orientation[2], qw = m.orientation[3];
        const double z[3] = {2 * (qx * qz + qw * qy), 2 * (qy * qz - qw * qx), 1 - 2 * (qx * qx + qy * qy)};
        for (int k = 0; k < 3; ++k) EXPECT(std::fabs(z[k] - f.axis[k]) < 1e-9);

        // a failed fit (no starting model) gives no marker and leaves it untouched
        const float nan7[7] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN};
        const gm_cylinder_fit bad = proc.getCylinder(cloud, nan7, tau);
        EXPECT(bad.status == GM_FIT_NO_MODEL && std::isnan(bad.radius));
        Marker m2 = m;
        EXPECT(!Processor::rvizCylinder(bad, 12.0, m2));
        EXPECT(m2.position[0] == m.position[0] && m2.scale[0] == m.scale[0]);
        std::printf("fit: r=%.6f axis=(%.6f %.6f %.6f) point=(%.6f %.6f %.6f) inliers=%u rms=%.5f last_step=%.2e\n",
                    f.radius, f.axis[0], f.axis[1], f.axis[2], f.point[0], f.point[1], f.point[2], f.inliers, f.rms,
                    f.last_step);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gm_cylfit_test ok\n");
    return 0;
}
