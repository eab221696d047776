// gm_wall_host.hip -- the part of the wall map's C ABI that needs no device (include/gm_hip.h states each rule): the
// defaults, the parameter checks, the classification of one cell, the metrics, the direction table, the mesh's triangle
// rule and its PLY file, the gauge of a polygon, the runs, the align's selection, the sections' basis, solve and metrics,
// the quantities' column, metrics and runs, and the design axis of a map, straight, arc or clothoid (DesignAxis: what the
// gm_wall_arc_* and gm_wall_clothoid_* entries, the alignment and the map's add, cloud and mesh all ask).
// No device call, no context, no map: it links against libm and the C++ library alone, and host/gm_wall_host_test.cpp,
// host/gm_wall_sections_host_test.cpp, host/gm_wall_mesh_host_test.cpp, host/gm_wall_quantities_host_test.cpp,
// host/gm_wall_arc_host_test.cpp and host/gm_wall_clothoid_host_test.cpp run it under the host sanitizers;
// host/gm_wall_axis_dump.cpp prints the axis entries' results for a comparison of two builds.
#include <stdio.h>

#include <vector>

#define GM_WALL_HOST_ONLY
#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

gm_status check_params(const gm_wall_params *p)
{
    if (!p || p->struct_size != sizeof(gm_wall_params)) return GM_ERR_INVALID_ARG;
    if (p->n_stations < 1u || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS ||
        (uint64_t)p->n_stations * p->n_sectors > GM_WALL_MAX_CELLS)
        return GM_ERR_INVALID_ARG;
    if (!(p->station_length > 0.0) || !isfinite(p->station_length) || !((float)p->station_length > 0.0f) ||
        !isfinite((float)p->station_length) || !isfinite(p->t_min) || !(p->gate > 0.0) || !(p->gate <= 8.0) ||
        !(p->radius > 0.0) || !isfinite((float)p->radius))
        return GM_ERR_INVALID_ARG;
    double up2 = 0.0, fw2 = 0.0, d2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(p->up[k]) || !isfinite(p->forward[k]) || !isfinite(p->direction[k]) || !isfinite(p->point[k]))
            return GM_ERR_INVALID_ARG;
        up2 += p->up[k] * p->up[k];
        fw2 += p->forward[k] * p->forward[k];
        d2 += p->direction[k] * p->direction[k];
    }
    if (!(up2 > 0.0) || !(fw2 > 0.0) || !(d2 > 0.0) || !isfinite(up2) || !isfinite(fw2) || !isfinite(d2)) return GM_ERR_INVALID_ARG;
    return GM_OK;
}

void design_frame_of(const gm_wall_params &p, DesignFrame &d)
{
    const double dn = sqrt(dot(p.direction, p.direction));
    const double s = dot(p.direction, p.forward);
    for (int k = 0; k < 3; ++k) d.a[k] = (s >= 0.0 ? p.direction[k] : -p.direction[k]) / dn;
    const double ca = dot(p.point, d.a), ua = dot(p.up, d.a);
    double u[3];
    for (int k = 0; k < 3; ++k) u[k] = p.up[k] - ua * d.a[k];
    const double ul = sqrt(dot(u, u)), upl = sqrt(dot(p.up, p.up));
    d.status = GM_SURF_OK;
    if (ul < 0.1 * upl) {
        double e2[3];
        fit_basis(d.a, u, e2);
        d.status |= GM_SURF_UP_FALLBACK;
    } else {
        for (int k = 0; k < 3; ++k) u[k] /= ul;
    }
    const double *a = d.a;
    const double v[3] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]};
    for (int k = 0; k < 3; ++k) {
        d.o[k] = p.point[k] - ca * a[k];
        d.u[k] = u[k];
        d.v[k] = v[k];
    }
    d.R = p.radius;
}

// ---- the design axis (gm_wall_map.hpp: DesignAxis).  The clothoid's quadrature, table and Newton foot first ----

// the 8-node Gauss-Legendre rule on [-1, 1]
static const double kGl8X[8] = {-0.9602898564975362, -0.7966664774136267, -0.525532409916329, -0.18343464249564978,
                                0.18343464249564978, 0.525532409916329,   0.7966664774136267, 0.9602898564975362};
static const double kGl8W[8] = {0.10122853629037669, 0.22238103445337434, 0.31370664587788705, 0.36268378337836177,
                                0.36268378337836177, 0.31370664587788705, 0.22238103445337434, 0.10122853629037669};

// I(ta, tb) of the header, added to (X, Y)
static void clothoid_integrate(const ClothoidFrame &f, double ta, double tb, double &X, double &Y)
{
    const double ka = fabs(f.kappa(ta)), kb = fabs(f.kappa(tb));
    const double load = std::min(std::max(ka, kb) * fabs(tb - ta) / 0.25, 4095.0);
    const int K = 1 + (load >= 0.0 ? (int)load : 0);   // (a NaN: one panel; the caller refuses what is not finite)
    const double w = (tb - ta) / (double)K, h = 0.5 * w;
    double sx_all = 0.0, sy_all = 0.0;
    for (int q = 0; q < K; ++q) {
        const double mid = ta + ((double)q + 0.5) * w;
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < 8; ++i) {
            const double ps = f.psi(mid + h * kGl8X[i]);
            sx += kGl8W[i] * cos(ps);
            sy += kGl8W[i] * sin(ps);
        }
        sx_all += h * sx;
        sy_all += h * sy;
    }
    X += sx_all;
    Y += sy_all;
}

// (X, Y) at tau = s - s0: the table entry at or below it plus the panels from there
static void clothoid_xy(const ClothoidFrame &f, double tau, double &X, double &Y)
{
    const double jd = floor((tau - f.tau0) / f.ds);
    const size_t j = jd >= 0.0 ? (jd < (double)f.nst ? (size_t)jd : (size_t)f.nst) : 0;   // (a NaN: 0)
    X = f.tab[2 * j];
    Y = f.tab[2 * j + 1];
    clothoid_integrate(f, f.tau0 + (double)j * f.ds, tau, X, Y);
}

// the foot of the perpendicular of a map point on a clothoid axis: returns tau; yc of the final evaluation
static double clothoid_foot(const DesignAxis &ax, const double x[3], double &yc)
{
    const ClothoidFrame &f = ax.cl;
    const double r[3] = {x[0] - f.pt[0], x[1] - f.pt[1], x[2] - f.pt[2]};
    const double xa = dot(r, ax.d.a), xn = dot(r, ax.n);
    size_t best = 0;
    double best_d2 = INFINITY;
    for (size_t j = 0; j <= (size_t)f.nst; ++j) {
        const double ex = xa - f.tab[2 * j], ey = xn - f.tab[2 * j + 1];
        const double d2 = ex * ex + ey * ey;
        if (d2 < best_d2) { best_d2 = d2; best = j; }
    }
    double tau = f.tau0 + (double)best * f.ds;
    for (int it = 0; it <= GM_WALL_CLOTHOID_HOST_STEPS; ++it) {
        double X, Y;
        clothoid_xy(f, tau, X, Y);
        const double psi = f.psi(tau);
        const double c = cos(psi), s = sin(psi);
        const double dx = xa - X, dy = xn - Y;
        const double g = dx * c + dy * s;
        yc = dy * c - dx * s;
        if (it < GM_WALL_CLOTHOID_HOST_STEPS) tau = tau + g / (1.0 - f.kappa(tau) * yc);
    }
    return tau;
}

// the section of a curved axis at tau = s - s0: a(s), n(s), P(s); returns kappa(s)
static double curved_section(const DesignAxis &ax, double tau, double as[3], double ns[3], double P[3])
{
    const bool on_cl = ax.kind == kAxisClothoid;
    const double psi = on_cl ? ax.cl.psi(tau) : ax.arc.kappa * tau;
    const double cp = cos(psi), sp = sin(psi);
    double X = 0.0, Y = 0.0;
    if (on_cl) clothoid_xy(ax.cl, tau, X, Y);
    for (int k = 0; k < 3; ++k) {
        as[k] = ax.d.a[k] * cp + ax.n[k] * sp;
        ns[k] = ax.n[k] * cp - ax.d.a[k] * sp;
        if (on_cl) P[k] = (ax.cl.pt[k] + X * ax.d.a[k]) + Y * ax.n[k];
        else P[k] = ax.arc.C[k] - ns[k] * ax.arc.inv_kappa;
    }
    return on_cl ? ax.cl.kappa(tau) : ax.arc.kappa;
}

gm_status axis_check(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, DesignAxis &ax)
{
    if (check_params(p) != GM_OK) return GM_ERR_INVALID_ARG;
    if (arc && (arc->struct_size != sizeof(gm_wall_arc) || !isfinite(arc->curvature[0]) || !isfinite(arc->curvature[1]) ||
                !isfinite(arc->curvature[2]) || !isfinite(arc->point_chainage)))
        return GM_ERR_INVALID_ARG;
    if (cl && (cl->struct_size != sizeof(gm_wall_clothoid) || cl->reserved != 0u || !isfinite(cl->normal[0]) || !isfinite(cl->normal[1]) ||
               !isfinite(cl->normal[2]) || !isfinite(cl->curvature) || !isfinite(cl->rate) || !isfinite(cl->point_chainage)))
        return GM_ERR_INVALID_ARG;
    ax = DesignAxis();
    design_frame_of(*p, ax.d);
    if (!arc && !cl) return GM_OK;
    // n: the curvature vector's, or the normal's, direction across the design direction
    const double *side = arc ? arc->curvature : cl->normal;
    const double na = dot(side, ax.d.a);
    double m[3];
    for (int k = 0; k < 3; ++k) m[k] = side[k] - na * ax.d.a[k];
    const double lm = sqrt(dot(m, m));
    if (arc) {
        ArcFrame &f = ax.arc;
        const double kappa = lm;
        if (!isfinite(kappa) || kappa < 1e-6 || (p->radius + p->gate) * kappa > 0.5) return GM_ERR_INVALID_ARG;
        const double s0 = arc->point_chainage, s_end = p->t_min + (double)p->n_stations * p->station_length;
        if (!(fabs(kappa * (p->t_min - s0)) <= 3.0) || !(fabs(kappa * (s_end - s0)) <= 3.0)) return GM_ERR_INVALID_ARG;
        f.kappa = kappa;
        f.inv_kappa = 1.0 / kappa;
        f.s0 = s0;
        for (int k = 0; k < 3; ++k) {
            ax.n[k] = m[k] / kappa;
            f.C[k] = p->point[k] + ax.n[k] * f.inv_kappa;
        }
    } else {
        ClothoidFrame &f = ax.cl;
        const double l0 = sqrt(dot(cl->normal, cl->normal));
        if (!isfinite(lm) || !(lm > 1e-6 * l0) || !(lm > 0.0)) return GM_ERR_INVALID_ARG;
        const double L = (double)p->n_stations * p->station_length;
        if (fabs(cl->rate) * L < 1e-6) return GM_ERR_INVALID_ARG;
        f.k0 = cl->curvature;
        f.rate = cl->rate;
        f.s0 = cl->point_chainage;
        f.tau0 = p->t_min - f.s0;
        f.ds = p->station_length;
        f.nst = p->n_stations;
        const double t0 = f.tau0, t1 = f.tau0 + L;
        const double kmax = std::max(fabs(f.kappa(t0)), fabs(f.kappa(t1)));
        if (!((p->radius + p->gate) * kmax <= 0.5)) return GM_ERR_INVALID_ARG;
        if (!(fabs(f.psi(t0)) <= 3.0) || !(fabs(f.psi(t1)) <= 3.0)) return GM_ERR_INVALID_ARG;
        const double tz = -f.k0 / f.rate;   // kappa = 0 there
        if (t0 < tz && tz < t1 && !(fabs(f.psi(tz)) <= 3.0)) return GM_ERR_INVALID_ARG;
        for (int k = 0; k < 3; ++k) { f.pt[k] = p->point[k]; ax.n[k] = m[k] / lm; }
        try {
            f.tab.assign(2 * ((size_t)f.nst + 1), 0.0);
        } catch (...) {
            return GM_ERR_OOM;
        }
        double X = 0.0, Y = 0.0;
        clothoid_integrate(f, 0.0, f.tau0, X, Y);
        f.tab[0] = X; f.tab[1] = Y;
        for (uint32_t j = 0; j < f.nst; ++j) {
            clothoid_integrate(f, f.tau0 + (double)j * f.ds, f.tau0 + (double)(j + 1u) * f.ds, X, Y);
            f.tab[2 * ((size_t)j + 1)] = X; f.tab[2 * ((size_t)j + 1) + 1] = Y;
        }
    }
    const double *a = ax.d.a, *n = ax.n;
    ax.b[0] = a[1] * n[2] - a[2] * n[1]; ax.b[1] = a[2] * n[0] - a[0] * n[2]; ax.b[2] = a[0] * n[1] - a[1] * n[0];
    ax.un = dot(ax.d.u, ax.n); ax.ub = dot(ax.d.u, ax.b);
    ax.vn = dot(ax.d.v, ax.n); ax.vb = dot(ax.d.v, ax.b);
    ax.kind = arc ? kAxisArc : kAxisClothoid;
    return GM_OK;
}

double DesignAxis::section(double s, double as[3], double ns[3], double P[3]) const
{
    if (kind != kAxisStraight) return curved_section(*this, s - (kind == kAxisClothoid ? cl.s0 : arc.s0), as, ns, P);
    for (int k = 0; k < 3; ++k) { as[k] = d.a[k]; ns[k] = d.u[k]; P[k] = d.o[k] + s * d.a[k]; }
    return 0.0;
}

double DesignAxis::station_section(const gm_wall_params &p, double j, double as[3], double ns[3], double P[3]) const
{
    if (kind == kAxisClothoid) return curved_section(*this, cl.tau0 + j * p.station_length, as, ns, P);
    return section(p.t_min + j * p.station_length, as, ns, P);
}

double DesignAxis::frame(double s, double o[3], double a[3], double u[3], double v[3], double *n_out) const
{
    double ns[3];
    const double kappa = section(s, a, ns, o);
    for (int k = 0; k < 3; ++k) {
        u[k] = kind == kAxisStraight ? d.u[k] : un * ns[k] + ub * b[k];
        v[k] = kind == kAxisStraight ? d.v[k] : vn * ns[k] + vb * b[k];
        if (n_out) n_out[k] = ns[k];
    }
    return kappa;
}

double DesignAxis::foot(const double x[3], double &yc, double &zb) const
{
    const double *org = kind == kAxisClothoid ? cl.pt : (kind == kAxisArc ? arc.C : d.o);
    const double r[3] = {x[0] - org[0], x[1] - org[1], x[2] - org[2]};
    if (kind == kAxisStraight) {
        yc = dot(r, d.u);
        zb = dot(r, d.v);
        return dot(r, d.a);
    }
    zb = dot(r, b);
    if (kind == kAxisClothoid) return cl.s0 + clothoid_foot(*this, x, yc);
    const double xa = dot(r, d.a), xn = dot(r, n);
    yc = arc.inv_kappa - sqrt(xa * xa + xn * xn);
    return arc.s0 + atan2(xa, -xn) / arc.kappa;
}

void DesignAxis::project(const double x[3], double &chainage, double &angle, double &e) const
{
    double th;
    if (kind == kAxisStraight) {
        const double r[3] = {x[0] - d.o[0], x[1] - d.o[1], x[2] - d.o[2]};
        const double t = dot(r, d.a);
        const double w[3] = {r[0] - t * d.a[0], r[1] - t * d.a[1], r[2] - t * d.a[2]};
        chainage = t + offset;
        e = sqrt(dot(w, w)) - d.R;
        th = atan2(dot(w, d.v), dot(w, d.u));
    } else {
        double yc = 0.0, zb;
        chainage = foot(x, yc, zb);
        e = sqrt(yc * yc + zb * zb) - d.R;
        th = atan2(yc * vn + zb * vb, yc * un + zb * ub);
    }
    angle = th < 0.0 ? th + kTwoPi : th;
}

void DesignAxis::point(double chainage, double angle, double rho, double xyz[3]) const
{
    const double c = cos(angle), s = sin(angle);
    const double yc = rho * (c * un + s * vn), zb = rho * (c * ub + s * vb);
    if (kind == kAxisStraight) {
        const double t = chainage - offset;
        for (int k = 0; k < 3; ++k) xyz[k] = (d.o[k] + t * d.a[k]) + rho * (c * d.u[k] + s * d.v[k]);
    } else if (kind == kAxisClothoid) {
        double as[3], ns[3], P[3];
        section(chainage, as, ns, P);
        for (int k = 0; k < 3; ++k) xyz[k] = (P[k] + yc * ns[k]) + zb * b[k];
    } else {   // (about the centre: P(s) is not formed)
        const double psi = arc.kappa * (chainage - arc.s0);
        const double cp = cos(psi), sp = sin(psi);
        const double r = yc - arc.inv_kappa;
        for (int k = 0; k < 3; ++k) {
            const double nr = n[k] * cp - d.a[k] * sp;
            xyz[k] = (arc.C[k] + r * nr) + zb * b[k];
        }
    }
}

bool DesignAxis::add_frame(const gm_wall_params &p, const double Rm[3][3], const double tr[3], AxisAddFrame &out) const
{
    const double ds = p.station_length;
    double jd, yc, zb;
    if (kind == kAxisClothoid) {
        const double tau = clothoid_foot(*this, tr, yc);
        out.s = cl.s0 + tau;
        jd = floor((tau - cl.tau0) / ds);   // (s - t_min, taken in tau: moving s0 and t_min together moves no anchor)
    } else {
        out.s = foot(tr, yc, zb);
        jd = floor((out.s - p.t_min) / ds);
    }
    if (!(fabs(jd) < 4.0e18)) return false;
    out.anchor = (int64_t)jd;
    out.sf = p.t_min + jd * ds;
    double as[3], ns[3];
    const double kf = station_section(p, jd, as, ns, out.P);
    const double *bs = kind == kAxisStraight ? d.v : b;   // (a straight axis: u, v where a curved one has n, b)
    const double of[3] = {out.P[0] - tr[0], out.P[1] - tr[1], out.P[2] - tr[2]};
    out.a1 = 0.0;
    for (int c = 0; c < 3; ++c) {   // Rm^T x
        const double oo = Rm[0][c] * of[0] + Rm[1][c] * of[1] + Rm[2][c] * of[2];
        const double aa = Rm[0][c] * as[0] + Rm[1][c] * as[1] + Rm[2][c] * as[2];
        const double nn = Rm[0][c] * ns[0] + Rm[1][c] * ns[1] + Rm[2][c] * ns[2];
        const double bb = Rm[0][c] * bs[0] + Rm[1][c] * bs[1] + Rm[2][c] * bs[2];
        out.o64[c] = oo; out.a64[c] = aa;
        out.o[c] = (float)oo; out.a[c] = (float)aa; out.n[c] = (float)nn; out.b[c] = (float)bb;
        out.u64[c] = kind == kAxisStraight ? nn : un * nn + ub * bb;
        out.v64[c] = kind == kAxisStraight ? bb : vn * nn + vb * bb;
        out.a1 += fabs(aa);
    }
    out.kappa = (float)kf;
    out.rate = (float)cl.rate;
    out.un = (float)un; out.ub = (float)ub; out.vn = (float)vn; out.vb = (float)vb;
    return true;
}

double DesignAxis::reach(const gm_wall_params &p, double B, double a1) const
{
    const double ds = p.station_length;
    // The LDS window affects speed only (a mapped point outside it goes to the map directly).
    // A clothoid, sized from the largest |kappa| of the map: a mapped point and the sensor both lie within rho = R + gate of
    // the axis, and rho max |kappa| <= 0.5 (a refusal of the creation), where the foot of the perpendicular moves by at most
    // 1 / (1 - rho max |kappa|) <= 2 times the distance between two points.  A point of the crop cube |p|_inf <= B is
    // within sqrt(3) B of the sensor, whose own foot lies less than ds past the anchor section: |t| <= 2 sqrt(3) B + ds
    // (the one station goes into add_window's slack).  The tangent turns along the reach, so |a'|_1 does not sharpen it.
    if (kind == kAxisClothoid) return 2.0 * B * 1.7320508075688772 / ds;
    // An arc: wherever cy >= 0.5, |t| = |atan2(cx, cy)| / kappa <= |cx| / (cy kappa) <= 2 |x|, and |x| <= B |a'|_1 + ds over
    // the crop cube |p|_inf <= B as on a straight map (the sensor lies within ds of the anchor section: the stations that
    // costs at the window's ends take the global path).
    if (kind == kAxisArc) return 2.0 * B * a1 / ds;
    // A straight axis: t = p.a' + (s - chainage of the anchor station's start) lies in [-B |a'|_1, B |a'|_1 + ds) for the
    // points of the crop cube |p|_inf <= B, so their stations relative to the anchor in [floor(-reach), floor(reach) + 1].
    return B * a1 / ds;
}

void DesignAxis::row(double tc, const double anchor[3], double *row) const
{
    const double tau = tc - (kind == kAxisClothoid ? cl.s0 : arc.s0);
    const double psi = kind == kAxisClothoid ? cl.psi(tau) : arc.kappa * tau;
    if (kind == kAxisClothoid) {   // (P(tc) - anchor, cos psi, sin psi); an arc: (cos psi, sin psi)
        double as[3], ns[3], P[3];
        curved_section(*this, tau, as, ns, P);
        for (int k = 0; k < 3; ++k) row[k] = P[k] - anchor[k];
        row += 3;
    }
    row[0] = cos(psi);
    row[1] = sin(psi);
}

int pose_split(const double pose[12], double Rm[3][3], double tr[3])
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c)
            if (!isfinite(pose[4 * r + c])) return 1;
        for (int c = 0; c < 3; ++c) Rm[r][c] = pose[4 * r + c];
        tr[r] = pose[4 * r + 3];
    }
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = Rm[0][i] * Rm[0][j] + Rm[1][i] * Rm[1][j] + Rm[2][i] * Rm[2][j] - (i == j ? 1.0 : 0.0);
            dev = std::max(dev, fabs(g));
        }
    const double det = Rm[0][0] * (Rm[1][1] * Rm[2][2] - Rm[1][2] * Rm[2][1]) - Rm[0][1] * (Rm[1][0] * Rm[2][2] - Rm[1][2] * Rm[2][0]) +
                       Rm[0][2] * (Rm[1][0] * Rm[2][1] - Rm[1][1] * Rm[2][0]);
    return (!(dev <= 1e-6) || !(det > 0.0)) ? 2 : 0;
}

void cloud_directions(uint32_t nsec, uint32_t bk, double *cos_sin)
{
    const uint32_t NK = (nsec + bk - 1u) / bk;
    for (uint32_t K = 0; K < NK; ++K) {
        const uint32_t nk = nsec - K * bk < bk ? nsec - K * bk : bk;
        const double f = (double)(2u * K * bk + nk) / (double)(2u * nsec);
        const double phi = kTwoPi * f;
        cos_sin[2 * K] = cos(phi);
        cos_sin[2 * K + 1] = sin(phi);
    }
}

bool clearance_ok(const gm_wall_params *p, const gm_wall_clearance_params &c, const int32_t *gauge_q, uint32_t n_gauges,
                  const uint8_t *station_gauge, uint32_t n, long long &T, long long &Rq)
{
    T = 0; Rq = 0;
    if (!p || !gauge_q || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return false;
    if (c.struct_size != sizeof(gm_wall_clearance_params) || c.reference > (uint32_t)GM_WALL_CLEAR_MEAN || c.min_count < 1u) return false;
    if (!(c.margin >= 0.0) || !(c.margin <= 8.0)) return false;
    if (!(p->radius > 0.0) || !isfinite(p->radius)) return false;
    const double rq = rint(p->radius * 1048576.0);
    if (!(rq <= 4294967296.0)) return false;
    if (n_gauges < 1u || n_gauges > GM_WALL_CLEAR_MAX_GAUGES) return false;
    const size_t entries = (size_t)n_gauges * p->n_sectors;
    for (size_t i = 0; i < entries; ++i)
        if (gauge_q[i] < 0) return false;
    if (station_gauge)
        for (uint32_t j = 0; j < n; ++j)
            if (station_gauge[j] >= n_gauges) return false;
    T = (long long)rint(c.margin * 1048576.0);
    Rq = (long long)rq;
    return true;
}

bool section_prm_ok(const gm_wall_section_params &p, long long &Tr)
{
    Tr = 0;
    if (p.struct_size != sizeof(gm_wall_section_params) || p.section_stations < 1u || p.harmonics > GM_WALL_SECTION_MAX_HARMONICS ||
        p.passes < 1u || p.passes > GM_WALL_SECTION_MAX_PASSES || p.min_count < 1u || p.min_columns < 1u)
        return false;
    if (!(p.max_gap_deg >= 0.0) || !(p.max_gap_deg <= 360.0) || !(p.reject > 0.0) || !(p.reject <= 8.0)) return false;
    Tr = (long long)rint(p.reject * 1048576.0);
    return Tr >= 1;
}

bool quantity_ok(const gm_wall_params *p, const gm_wall_quantity_params &q, const int32_t *lo_q, const int32_t *hi_q,
                 uint32_t n_profiles, const uint8_t *section_profile, uint32_t n, const uint8_t *zone, uint32_t n_zones,
                 long long &Rq)
{
    Rq = 0;
    if (!p || !lo_q || !hi_q || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS)
        return false;
    if (q.struct_size != sizeof(gm_wall_quantity_params) || q.section_stations < 1u || q.min_count < 1u) return false;
    if (!(p->radius > 0.0) || !isfinite(p->radius)) return false;
    const double rq = rint(p->radius * 1048576.0);
    if (!(rq <= 4294967296.0)) return false;
    if (n_profiles < 1u || n_profiles > GM_WALL_QUANTITY_MAX_PROFILES || n_zones < 1u || n_zones > GM_WALL_QUANTITY_MAX_ZONES) return false;
    const size_t entries = (size_t)n_profiles * p->n_sectors;
    for (size_t i = 0; i < entries; ++i)
        if (lo_q[i] < -(int32_t)kWallSectionSat || hi_q[i] > (int32_t)kWallSectionSat || lo_q[i] > hi_q[i]) return false;
    if (section_profile) {
        const uint32_t NS = n ? (n - 1u) / q.section_stations + 1u : 0u;
        for (uint32_t i = 0; i < NS; ++i)
            if (section_profile[i] >= n_profiles) return false;
    }
    if (zone)
        for (uint32_t k = 0; k < p->n_sectors; ++k)
            if (zone[k] >= n_zones && zone[k] != GM_WALL_QUANTITY_UNMEASURED) return false;
    Rq = (long long)rq;
    return true;
}

void section_basis(uint32_t nsec, uint32_t H, int32_t *B)
{
    const uint32_t P = 1u + 2u * H;
    const double den = (double)(2u * nsec);
    for (uint32_t k = 0; k < nsec; ++k) {
        const double f = (double)(2u * k + 1u) / den;
        const double phi = kTwoPi * f;
        int32_t *row = B + (size_t)k * P;
        row[0] = 1 << 20;
        for (uint32_t h = 1; h <= H; ++h) {
            const double ang = (double)h * phi;
            const double c = cos(ang);
            const double s = sin(ang);
            const double cs = c * 1048576.0;
            const double ss = s * 1048576.0;
            row[2u * h - 1u] = (int32_t)rint(cs);
            row[2u * h] = (int32_t)rint(ss);
        }
    }
}

uint32_t section_solve(const gm_wall_section_sums &s, uint32_t H, uint32_t min_columns, int64_t cq[9])
{
    const uint32_t P = 1u + 2u * H;
    for (int p = 0; p < 9; ++p) cq[p] = 0;
    if (s.fitted < std::max(min_columns, P)) return GM_SECTION_TOO_FEW;
    // one operation per statement: the same roundings as the twin's, whatever the compiler may contract
    double A[9][9], L[9][9], b[9], y[9], c[9];
    uint32_t idx = 0;
    for (uint32_t p = 0; p < P; ++p)
        for (uint32_t q = p; q < P; ++q) {
            const double v = (double)s.N[idx++];
            A[p][q] = v * 0x1p-40;
            A[q][p] = A[p][q];
        }
    for (uint32_t p = 0; p < P; ++p) {
        const double v = (double)s.r[p];
        b[p] = v * 0x1p-20;
    }
    for (uint32_t j = 0; j < P; ++j) {
        double d = A[j][j];
        for (uint32_t k = 0; k < j; ++k) {
            const double t = L[j][k] * L[j][k];
            d = d - t;
        }
        const double lim = 1e-12 * A[j][j];
        if (!(d > lim)) return GM_SECTION_SINGULAR;
        const double ljj = sqrt(d);
        L[j][j] = ljj;
        for (uint32_t i = j + 1u; i < P; ++i) {
            double v = A[i][j];
            for (uint32_t k = 0; k < j; ++k) {
                const double t = L[i][k] * L[j][k];
                v = v - t;
            }
            L[i][j] = v / ljj;
        }
    }
    for (uint32_t i = 0; i < P; ++i) {
        double v = b[i];
        for (uint32_t k = 0; k < i; ++k) {
            const double t = L[i][k] * y[k];
            v = v - t;
        }
        y[i] = v / L[i][i];
    }
    for (uint32_t i = P; i-- > 0u;) {
        double v = y[i];
        for (uint32_t k = i + 1u; k < P; ++k) {
            const double t = L[k][i] * c[k];
            v = v - t;
        }
        c[i] = v / L[i][i];
    }
    for (uint32_t p = 0; p < P; ++p) {
        const double rc = rint(c[p]);
        if (!(fabs(rc) <= 16777216.0)) {
            for (int q = 0; q < 9; ++q) cq[q] = 0;
            return GM_SECTION_UNBOUNDED;
        }
        cq[p] = (int64_t)rc;
    }
    return GM_SECTION_OK;
}

bool check_prm_ok(const gm_wall_check_params &c, long long &T)
{
    T = 0;
    if (c.struct_size != sizeof(gm_wall_check_params) || c.reference > (uint32_t)GM_WALL_CHECK_ENVELOPE || c.min_count < 1u) return false;
    if (!(c.threshold > 0.0) || !(c.threshold <= 8.0) || !(c.gate > 0.0) || !(c.gate <= 8.0)) return false;
    T = (long long)rint(c.threshold * 1048576.0);
    return T >= 1;
}

bool add_checked_prm_ok(const gm_wall_add_checked_params &p, long long &S)
{
    S = 0;
    if (p.struct_size != sizeof(gm_wall_add_checked_params) || p.skip < 1u || p.skip > (uint32_t)(GM_WALL_SKIP_NEG | GM_WALL_SKIP_POS)) return false;
    if (!(p.min_delta >= 0.0) || !(p.min_delta <= 8.0)) return false;
    S = (long long)rint(p.min_delta * 1048576.0);
    return true;
}

bool locate_prm_ok(const gm_wall_locate_params &p)
{
    return p.struct_size == sizeof(gm_wall_locate_params) && p.reference <= (uint32_t)GM_WALL_LOCATE_MAP && p.min_count >= 1u &&
           p.gate > 0.0 && p.gate <= 8.0;
}

bool align_prm_ok(const gm_wall_align_params &p, uint32_t nsec)
{
    if (p.struct_size != sizeof(gm_wall_align_params) || nsec < 1u || nsec > GM_WALL_MAX_SECTORS) return false;
    if (p.half_patch_stations < 1u || 2ull * p.half_patch_stations * nsec > GM_WALL_ALIGN_MAX_PATCH_CELLS) return false;
    if (p.max_station_shift > GM_WALL_ALIGN_MAX_SHIFT || p.max_sector_shift > GM_WALL_ALIGN_MAX_SHIFT) return false;
    if (2u * p.max_sector_shift + 1u > nsec) return false;
    if ((2u * p.max_station_shift + 1u) * (2u * p.max_sector_shift + 1u) > GM_WALL_ALIGN_MAX_SHIFTS) return false;
    if (p.min_count < 1u || p.min_frame_count < 1u || p.min_overlap < 1u) return false;
    if (!(p.gate > 0.0) || !(p.gate <= 8.0) || !(p.clip > 0.0) || !(p.clip <= 8.0) || !(rint(p.clip * 1048576.0) >= 1.0)) return false;
    return p.min_distinction >= 1.0 && isfinite(p.min_distinction);
}

bool object_prm_ok(const gm_wall_object_params &p)
{
    return p.struct_size == sizeof(gm_wall_object_params) && p.block_stations >= 1u && p.block_sectors >= 1u &&
           p.min_block_points >= 1u && p.min_points >= 1u && (p.connectivity == 4u || p.connectivity == 8u) &&
           p.half_window_stations >= 1u && p.half_window_stations <= (1u << 20);
}

bool object_window(uint64_t n_stations, uint32_t n_sectors, const gm_wall_object_params &op, int64_t jf, ObjectWindow &w)
{
    const int64_t H = op.half_window_stations, ns = (int64_t)n_stations;   // (compared before added: j_f is any int64)
    const int64_t lo = jf > H ? jf - H : 0, hi = jf >= ns - H ? ns : jf + H;
    w = ObjectWindow();
    w.NK = (n_sectors + op.block_sectors - 1u) / op.block_sectors;
    if (lo >= hi) return true;
    const uint64_t bs = op.block_stations, J0 = (uint64_t)lo / bs, J1 = (uint64_t)(hi - 1) / bs;
    w.J0 = (uint32_t)J0;
    w.nJ = (uint32_t)(J1 - J0 + 1u);
    w.station0 = (uint32_t)(J0 * bs);
    w.n_stations = (uint32_t)(std::min<uint64_t>((J1 + 1u) * bs, (uint64_t)ns) - J0 * bs);
    return (uint64_t)w.nJ * w.NK <= GM_WALL_OBJECT_MAX_BLOCKS;
}

bool align_select_table(const gm_wall_align_params &ap, double ds, uint32_t nsec, const gm_wall_align_score *t, gm_wall_align_info *info)
{
    const int A = (int)ap.max_station_shift, B = (int)ap.max_sector_shift, nb = 2 * B + 1, ns = (2 * A + 1) * nb;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_align_info);
    info->half_patch_stations = ap.half_patch_stations;
    info->max_station_shift = ap.max_station_shift;
    info->max_sector_shift = ap.max_sector_shift;
    auto cheb = [&](int i, int a0, int b0) { return std::max(abs(i / nb - A - a0), abs(i % nb - B - b0)); };
    auto valid = [&](int i) { return t[i].n >= ap.min_overlap; };
    auto cost = [&](int i) { return (double)t[i].ssd / (double)t[i].n; };
    int best = -1;
    for (int i = 0; i < ns; ++i) {
        if (!valid(i)) continue;
        if (best >= 0) {   // ssd_i / n_i against ssd_best / n_best, exactly
            const unsigned __int128 l = (unsigned __int128)t[i].ssd * t[best].n, r = (unsigned __int128)t[best].ssd * t[i].n;
            if (l > r || (l == r && cheb(i, 0, 0) >= cheb(best, 0, 0))) continue;
        }
        best = i;
    }
    if (best < 0) {
        info->status = GM_ALIGN_NO_OVERLAP;
        info->frac_station = info->frac_sector = info->shift_m = info->roll = info->bias_m = nan;
        info->rms_best = info->rms_runner = info->distinction = nan;
        for (int k = 0; k < 12; ++k) info->pose[k] = nan;
        return false;
    }
    const int ia = best / nb, ib = best % nb, sa = ia - A, sb = ib - B;
    const double c0 = cost(best);
    auto fraction = [&](int lo, int hi, bool have) {
        if (!have || !valid(lo) || !valid(hi)) return 0.0;
        const double cm = cost(lo), cp = cost(hi), den = cm - 2.0 * c0 + cp;
        if (!(den > 0.0)) return 0.0;
        const double f = 0.5 * (cm - cp) / den;
        return f < -0.5 ? -0.5 : (f > 0.5 ? 0.5 : f);
    };
    const double fa = fraction(best - nb, best + nb, ia > 0 && ia < 2 * A);
    const double fb = fraction(best - 1, best + 1, ib > 0 && ib < 2 * B);
    double cr = inf;
    bool runner = false;
    for (int i = 0; i < ns; ++i)
        if (valid(i) && cheb(i, sa, sb) > 1) {
            const double c = cost(i);
            if (!runner || c < cr) cr = c;
            runner = true;
        }
    info->overlap = t[best].n;
    info->best_station = sa;
    info->best_sector = sb;
    info->frac_station = fa;
    info->frac_sector = fb;
    info->shift_m = ((double)sa + fa) * ds;
    info->roll = ((double)sb + fb) * (kTwoPi / (double)nsec);
    info->bias_m = ((double)t[best].sum_d * 0x1p-20) / (double)t[best].n;
    info->rms_best = sqrt(c0) * 0x1p-20;
    info->rms_runner = runner ? sqrt(cr) * 0x1p-20 : nan;
    info->distinction = (c0 == 0.0 || !runner) ? inf : cr / c0;
    info->status = GM_ALIGN_OK;
    if (info->distinction < ap.min_distinction) info->status |= GM_ALIGN_AMBIGUOUS;
    if ((A > 0 && abs(sa) == A) || (B > 0 && abs(sb) == B)) info->status |= GM_ALIGN_AT_BORDER;
    return true;
}

void align_select(const DesignFrame &d, const gm_wall_params &wp, const gm_wall_align_params &ap, const double Rm[3][3],
                  const double tr[3], const gm_wall_align_score *t, gm_wall_align_info *info)
{
    const double ds = wp.station_length;
    const bool ok = align_select_table(ap, ds, wp.n_sectors, t, info);
    const double rel[3] = {tr[0] - d.o[0], tr[1] - d.o[1], tr[2] - d.o[2]};
    const double jd = floor((dot(rel, d.a) - wp.t_min) / ds);
    info->anchor_station = fabs(jd) < 4.0e18 ? (int64_t)jd : 0;
    if (!ok) return;
    // Rm' = Q Rm, tr' = o + Q (tr - o) + shift_m a;  Q = cos I + sin [a]x + (1 - cos) a a^T
    const double cs = cos(info->roll), sn = sin(info->roll);
    const double *a = d.a;
    const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
    double Q[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Q[r][c] = (r == c ? cs : 0.0) + sn * K[r][c] + (1.0 - cs) * a[r] * a[c];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) info->pose[4 * r + c] = Q[r][0] * Rm[0][c] + Q[r][1] * Rm[1][c] + Q[r][2] * Rm[2][c];
        info->pose[4 * r + 3] = d.o[r] + (Q[r][0] * rel[0] + Q[r][1] * rel[1] + Q[r][2] * rel[2]) + info->shift_m * a[r];
    }
}

}  // namespace wall
}  // namespace gm

namespace {

// The extent outputs the two metrics calls share: chainage_from / _to and angle_from_deg / _to_deg of a record's station
// and sector extents, the turned pair when it is the shorter (the record lies across the seam).  false, and nothing
// written: the extents are not those of a record on this grid.  One operation per statement: the same roundings as the
// twin's, whatever the compiler may contract.
template <class R, class M>
bool extent_metrics(const gm_wall_params &p, const R &r, M *out)
{
    const uint32_t ns = p.n_sectors, half = ns / 2u;
    if (r.sector_min > r.sector_max || r.sector_max >= ns || r.sector_min_turned > r.sector_max_turned ||
        r.sector_max_turned >= ns || r.station_min > r.station_max)
        return false;
    const double from = (double)r.station_min * p.station_length;
    const double to = (double)(r.station_max + 1.0) * p.station_length;
    out->chainage_from = p.t_min + from;
    out->chainage_to = p.t_min + to;
    const uint32_t plain = r.sector_max - r.sector_min + 1u, turned = r.sector_max_turned - r.sector_min_turned + 1u;
    uint32_t k_from = r.sector_min, k_end = r.sector_max + 1u;
    if (turned < plain) {   // turned back: k = (t - n_sectors / 2) mod n_sectors
        k_from = (r.sector_min_turned + ns - half) % ns;
        k_end = (r.sector_max_turned + ns - half) % ns + 1u;
    }
    const double a0 = 360.0 * (double)k_from;
    const double a1 = 360.0 * (double)k_end;
    out->angle_from_deg = a0 / (double)ns;
    out->angle_to_deg = a1 / (double)ns;
    return true;
}

double cross2(const double a[2], const double b[2]) { return a[0] * b[1] - a[1] * b[0]; }

// 1 when the closed segments ab and cd share a point
bool segments_meet(const double a[2], const double b[2], const double c[2], const double d[2])
{
    const double ab[2] = {b[0] - a[0], b[1] - a[1]}, cd[2] = {d[0] - c[0], d[1] - c[1]};
    const double ac[2] = {c[0] - a[0], c[1] - a[1]}, ad[2] = {d[0] - a[0], d[1] - a[1]};
    const double ca[2] = {a[0] - c[0], a[1] - c[1]}, cb[2] = {b[0] - c[0], b[1] - c[1]};
    const double o1 = cross2(ab, ac), o2 = cross2(ab, ad), o3 = cross2(cd, ca), o4 = cross2(cd, cb);
    if (((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0))) return true;
    auto on = [](const double p[2], const double q[2], const double r[2]) {   // r collinear with pq: inside its box?
        return std::min(p[0], q[0]) <= r[0] && r[0] <= std::max(p[0], q[0]) && std::min(p[1], q[1]) <= r[1] && r[1] <= std::max(p[1], q[1]);
    };
    return (o1 == 0.0 && on(a, b, c)) || (o2 == 0.0 && on(a, b, d)) || (o3 == 0.0 && on(c, d, a)) || (o4 == 0.0 && on(c, d, b));
}

// the polygon of gm_wall_gauge_from_polygon is accepted: finite, no edge of length 0, simple, the axis strictly inside
bool gauge_polygon_ok(const std::vector<double> &P, uint32_t nv)
{
    for (uint32_t i = 0; i < 2u * nv; ++i)
        if (!isfinite(P[i])) return false;
    const double zero[2] = {0.0, 0.0};
    int wn = 0;
    for (uint32_t i = 0; i < nv; ++i) {
        const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
        if (a[0] == b[0] && a[1] == b[1]) return false;
        const double left = cross2(a, b);   // > 0: the axis lies to the left of a -> b
        if (left == 0.0 && segments_meet(a, b, zero, zero)) return false;   // the axis on the boundary
        if (a[1] <= 0.0) {
            if (b[1] > 0.0 && left > 0.0) ++wn;
        } else if (b[1] <= 0.0 && left < 0.0) {
            --wn;
        }
    }
    if (wn == 0) return false;
    for (uint32_t i = 0; i < nv; ++i) {
        const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
        for (uint32_t j = i + 1u; j < nv; ++j) {
            const double *c = &P[2 * j], *d = &P[2 * ((j + 1u) % nv)];
            const bool next = j == i + 1u, prev = i == 0u && j == nv - 1u;
            if (next || prev) {   // neighbours share one vertex; they may not fold back onto each other
                const double *s = next ? b : a, *x = next ? a : b, *y = next ? d : c;   // s shared; x, y the far ends
                const double e[2] = {x[0] - s[0], x[1] - s[1]}, f[2] = {y[0] - s[0], y[1] - s[1]};
                if (cross2(e, f) == 0.0 && e[0] * f[0] + e[1] * f[1] > 0.0) return false;
            } else if (segments_meet(a, b, c, d)) {
                return false;
            }
        }
    }
    return true;
}

// a parameter block at its defaults: zeroed but for struct_size; the caller sets the rest
template <class P>
bool defaults_begin(P *p)
{
    if (!p) return false;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(P);
    return true;
}

// The gm_wall_arc_* and gm_wall_clothoid_* entries, each pair one rule: exactly one of arc and cl is the entry's struct (a
// NULL one is refused), `given`: every other pointer is set and every scalar finite.  All refusals are GM_ERR_INVALID_ARG.
bool axis_entry(bool given, const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, DesignAxis &ax)
{
    return given && (arc || cl) && axis_check(p, arc, cl, ax) == GM_OK;
}

template <class Info>   // gm_wall_arc_add_info, gm_wall_clothoid_add_info: everything they share
gm_status axis_add_frame(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, const double pose[12],
                         Info *info, AxisAddFrame &f)
{
    DesignAxis ax;
    double Rm[3][3], tr[3];
    if (!axis_entry(pose && info, p, arc, cl, ax) || pose_split(pose, Rm, tr)) return GM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    if (!ax.add_frame(*p, Rm, tr, f)) return GM_ERR_INVALID_ARG;
    info->struct_size = (uint32_t)sizeof(Info);
    info->status = ax.d.status;
    info->anchor_station = f.anchor;
    info->sensor_chainage = f.s;
    info->anchor_chainage = f.sf;
    for (int k = 0; k < 3; ++k) { info->o[k] = f.o[k]; info->a[k] = f.a[k]; info->n[k] = f.n[k]; info->b[k] = f.b[k]; }
    info->kappa = f.kappa;
    info->un = f.un; info->ub = f.ub; info->vn = f.vn; info->vb = f.vb;
    info->R = (float)ax.d.R;
    info->station_length = (float)p->station_length;
    info->sector_angle = (float)(kTwoPi / (double)p->n_sectors);
    info->gate = (float)p->gate;
    return GM_OK;
}

gm_status axis_frame(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, double chainage, double o[3],
                     double a[3], double u[3], double v[3], double *curvature, double n[3])
{
    DesignAxis ax;
    if (!axis_entry(o && a && u && v && (arc || curvature) && isfinite(chainage), p, arc, cl, ax)) return GM_ERR_INVALID_ARG;
    const double kappa = ax.frame(chainage, o, a, u, v, n);
    if (curvature) *curvature = kappa;
    return GM_OK;
}

gm_status axis_project(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, const double xyz[3],
                       double *chainage, double *angle, double *e)
{
    DesignAxis ax;
    const bool given = xyz && chainage && angle && e && isfinite(xyz[0]) && isfinite(xyz[1]) && isfinite(xyz[2]);
    if (!axis_entry(given, p, arc, cl, ax)) return GM_ERR_INVALID_ARG;
    ax.project(xyz, *chainage, *angle, *e);
    return GM_OK;
}

gm_status axis_point(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, double chainage, double angle,
                     double rho, double xyz[3])
{
    DesignAxis ax;
    if (!axis_entry(xyz && isfinite(chainage) && isfinite(angle) && isfinite(rho), p, arc, cl, ax)) return GM_ERR_INVALID_ARG;
    ax.point(chainage, angle, rho, xyz);
    return GM_OK;
}

}  // namespace

extern "C" {

void gm_wall_default_params(gm_wall_params *p)
{
    if (!defaults_begin(p)) return;
    p->n_stations = 4000;
    p->n_sectors = 90;
    p->station_length = 0.25;
    p->t_min = 0.0;
    p->gate = 0.25;
    p->direction[0] = 1.0;
    p->radius = 2.0;
    p->up[2] = 1.0;
    p->forward[0] = 1.0;
}

gm_status gm_wall_arc_check_params(const gm_wall_params *params, const gm_wall_arc *arc)
{
    DesignAxis ax;
    return axis_entry(true, params, arc, nullptr, ax) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_arc_add_frame(const gm_wall_params *params, const gm_wall_arc *arc, const double pose[12],
                                gm_wall_arc_add_info *info)
{
    AxisAddFrame f;
    return axis_add_frame(params, arc, nullptr, pose, info, f);
}

gm_status gm_wall_arc_frame(const gm_wall_params *params, const gm_wall_arc *arc, double chainage, double o[3], double a[3],
                            double u[3], double v[3])
{
    return axis_frame(params, arc, nullptr, chainage, o, a, u, v, nullptr, nullptr);
}

gm_status gm_wall_arc_project(const gm_wall_params *params, const gm_wall_arc *arc, const double xyz[3], double *chainage,
                              double *angle, double *e)
{
    return axis_project(params, arc, nullptr, xyz, chainage, angle, e);
}

gm_status gm_wall_arc_point(const gm_wall_params *params, const gm_wall_arc *arc, double chainage, double angle, double rho,
                            double xyz[3])
{
    return axis_point(params, arc, nullptr, chainage, angle, rho, xyz);
}

gm_status gm_wall_clothoid_check_params(const gm_wall_params *params, const gm_wall_clothoid *clothoid)
{
    DesignAxis ax;
    return axis_entry(true, params, nullptr, clothoid, ax) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_clothoid_add_frame(const gm_wall_params *params, const gm_wall_clothoid *clothoid, const double pose[12],
                                     gm_wall_clothoid_add_info *info)
{
    AxisAddFrame f;
    const gm_status st = axis_add_frame(params, nullptr, clothoid, pose, info, f);
    if (st == GM_OK) info->rate = f.rate;
    return st;
}

gm_status gm_wall_clothoid_frame(const gm_wall_params *params, const gm_wall_clothoid *clothoid, double chainage, double o[3],
                                 double a[3], double u[3], double v[3], double *curvature, double n[3])
{
    return axis_frame(params, nullptr, clothoid, chainage, o, a, u, v, curvature, n);
}

gm_status gm_wall_clothoid_project(const gm_wall_params *params, const gm_wall_clothoid *clothoid, const double xyz[3],
                                   double *chainage, double *angle, double *e)
{
    return axis_project(params, nullptr, clothoid, xyz, chainage, angle, e);
}

gm_status gm_wall_clothoid_point(const gm_wall_params *params, const gm_wall_clothoid *clothoid, double chainage, double angle,
                                 double rho, double xyz[3])
{
    return axis_point(params, nullptr, clothoid, chainage, angle, rho, xyz);
}

void gm_wall_region_default_params(gm_wall_region_params *p)
{
    if (!defaults_begin(p)) return;
    p->min_count = 8;
    p->min_cells = 4;
    p->connectivity = 8;
    p->threshold = 0.05;
}

void gm_wall_cloud_default_params(gm_wall_cloud_params *p)
{
    if (!defaults_begin(p)) return;
    p->block_stations = 1;
    p->block_sectors = 1;
    p->min_count = 1;
    p->exaggeration = 1.0;
}

void gm_wall_clearance_default_params(gm_wall_clearance_params *p)
{
    if (!defaults_begin(p)) return;
    p->reference = GM_WALL_CLEAR_MIN;
    p->min_count = 8;
    p->margin = 0.10;
}

void gm_wall_check_default_params(gm_wall_check_params *p)
{
    if (!defaults_begin(p)) return;
    p->reference = GM_WALL_CHECK_MEAN;
    p->min_count = 8;
    p->threshold = 0.05;
    p->gate = 1.0;
}

void gm_wall_locate_default_params(gm_wall_locate_params *p)
{
    if (!defaults_begin(p)) return;
    p->reference = GM_WALL_LOCATE_DESIGN;
    p->min_count = 8;
    p->gate = 0.25;
}

void gm_wall_align_default_params(gm_wall_align_params *p)
{
    if (!defaults_begin(p)) return;
    p->half_patch_stations = 20;
    p->max_station_shift = 8;
    p->max_sector_shift = 4;
    p->min_count = 8;
    p->min_frame_count = 4;
    p->min_overlap = 64;
    p->gate = 0.25;
    p->clip = 0.05;
    p->min_distinction = 1.5;
}

void gm_wall_object_default_params(gm_wall_object_params *p)
{
    if (!defaults_begin(p)) return;
    p->block_stations = 1;
    p->block_sectors = 1;
    p->min_block_points = 2;
    p->min_points = 8;
    p->connectivity = 8;
    p->half_window_stations = 128;
}

void gm_wall_add_checked_default_params(gm_wall_add_checked_params *p)
{
    if (!defaults_begin(p)) return;
    p->skip = GM_WALL_SKIP_NEG | GM_WALL_SKIP_POS;
    p->min_delta = 0.0;
}

gm_status gm_wall_add_checked_check_params(const gm_wall_add_checked_params *p)
{
    long long S;
    return p && add_checked_prm_ok(*p, S) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_locate_check_params(const gm_wall_locate_params *p)
{
    return p && locate_prm_ok(*p) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_align_check_params(const gm_wall_align_params *p, uint32_t n_sectors)
{
    return p && align_prm_ok(*p, n_sectors) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_clearance_check_params(const gm_wall_params *p, const gm_wall_clearance_params *c, const int32_t *gauge_q,
                                         uint32_t n_gauges, const uint8_t *station_gauge, uint32_t n)
{
    long long T, Rq;
    const gm_wall_clearance_params cp = params_or(c, gm_wall_clearance_default_params);
    return clearance_ok(p, cp, gauge_q, n_gauges, station_gauge, n, T, Rq) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_check_classify(const gm_wall_check_params *prm, const gm_wall_raw_cell *cell, float e, int64_t *delta, uint32_t *cls)
{
    long long T;
    if (!prm || !cell || !delta || !cls || !check_prm_ok(*prm, T)) return GM_ERR_INVALID_ARG;
    *delta = 0;
    if (!(fabsf(e) <= (float)prm->gate)) {
        *cls = GM_WALL_CHECK_CLS_BEYOND_GATE;
        return GM_OK;
    }
    long long d;
    *cls = wall_check_rule(prm->reference, prm->min_count, T, cell->sum, cell->count, cell->min_key, cell->max_key, e, d);
    *delta = d;
    return GM_OK;
}

gm_status gm_wall_region_metrics(const gm_wall_params *p, const gm_wall_region *r, struct gm_wall_region_metrics *out)
{
    if (!p || !r || !out || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || r->cells < 1u) return GM_ERR_INVALID_ARG;
    if (!extent_metrics(*p, *r, out)) return GM_ERR_INVALID_ARG;
    const uint32_t ns = p->n_sectors;
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double sr = p->station_length * p->radius;
    const double ring = sr * kTwoPi;
    const double cell_area = ring / (double)ns;
    const double sum_m = (double)r->sum_d * 0x1p-20;
    out->area_m2 = (double)r->cells * cell_area;
    out->volume_m3 = sum_m * cell_area;
    out->peak_m = (double)r->peak * 0x1p-20;
    out->mean_m = sum_m / (double)r->cells;
    return GM_OK;
}

gm_status gm_wall_object_metrics(const gm_wall_params *p, const gm_wall_object_params *op, const gm_wall_object *o,
                                 struct gm_wall_object_metrics *out)
{
    if (!p || !o || !out || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || o->points < 1u) return GM_ERR_INVALID_ARG;
    if (op && op->struct_size != sizeof(gm_wall_object_params)) return GM_ERR_INVALID_ARG;
    if (!extent_metrics(*p, *o, out)) return GM_ERR_INVALID_ARG;
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double pts = (double)o->points;
    const double sx = (double)o->sum_x * 0x1p-16, sy = (double)o->sum_y * 0x1p-16, sz = (double)o->sum_z * 0x1p-16;
    out->centroid[0] = sx / pts;
    out->centroid[1] = sy / pts;
    out->centroid[2] = sz / pts;
    const double sum_m = (double)o->sum_delta * 0x1p-20;
    out->mean_m = sum_m / pts;
    out->peak_m = (double)o->peak * 0x1p-20;
    for (int k = 0; k < 3; ++k) out->size[k] = (double)o->box_max[k] - (double)o->box_min[k];
    return GM_OK;
}

gm_status gm_wall_cloud_directions(const gm_wall_params *p, const gm_wall_cloud_params *c, double *cos_sin, uint32_t capacity,
                                   uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return GM_ERR_INVALID_ARG;
    if (c && (c->struct_size != sizeof(gm_wall_cloud_params) || c->block_sectors < 1u)) return GM_ERR_INVALID_ARG;
    if (!cos_sin && capacity) return GM_ERR_INVALID_ARG;
    const uint32_t bk = std::min(c ? c->block_sectors : 1u, p->n_sectors);
    const uint32_t NK = (p->n_sectors + bk - 1u) / bk;
    if (n_out) *n_out = NK;
    if (capacity < NK) return GM_ERR_CAPACITY;
    cloud_directions(p->n_sectors, bk, cos_sin);
    return GM_OK;
}

void gm_wall_mesh_default_params(gm_wall_mesh_params *p)
{
    if (!defaults_begin(p)) return;
    gm_wall_cloud_default_params(&p->cloud);
}

gm_status gm_wall_mesh_triangulate(uint32_t NJ, uint32_t NK, const gm_wall_cloud_point *vertices, uint64_t n_vertices,
                                   uint32_t flags, double max_step, gm_wall_mesh_info *info, gm_wall_mesh_triangle *triangles,
                                   uint64_t capacity, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!info || (!vertices && n_vertices) || (!triangles && capacity) || !mesh_rule_ok(flags, max_step)) return GM_ERR_INVALID_ARG;
    const uint64_t nb = (uint64_t)NJ * NK;
    if (nb > GM_WALL_MAX_CELLS || NK > GM_WALL_MAX_SECTORS) return GM_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n_vertices; ++i)
        if (vertices[i].block >= nb || (i && vertices[i].block <= vertices[i - 1].block)) return GM_ERR_INVALID_ARG;
    const MeshGrid g = mesh_grid(NJ, NK, flags);
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_mesh_info);
    info->wrapped = g.wrapped;
    info->cloud.blocks_stations = NJ;
    info->cloud.blocks_sectors = NK;
    info->cloud.blocks = nb;
    info->cloud.points = n_vertices;
    info->quads = g.quads;
    std::vector<uint32_t> rank((size_t)nb, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < n_vertices; ++i) rank[vertices[i].block] = (uint32_t)i;
    const bool cutting = max_step > 0.0, outward = (flags & GM_WALL_MESH_OUTWARD) != 0;
    const float step = (float)max_step;
    // two walks of the quads: the counts, then (when they fit) the records
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t nt = 0;
        for (uint64_t Q = 0; Q < g.quads; ++Q) {
            const uint32_t J = (uint32_t)(Q / g.NKq), K = (uint32_t)(Q % g.NKq), K1 = K + 1u == NK ? 0u : K + 1u;
            const uint32_t r[4] = {rank[(size_t)J * NK + K], rank[(size_t)(J + 1u) * NK + K], rank[(size_t)(J + 1u) * NK + K1],
                                   rank[(size_t)J * NK + K1]};
            uint32_t alive = 0, dead = 0;
            for (uint32_t c = 0; c < 4u; ++c) {
                if (r[c] != 0xFFFFFFFFu) ++alive;
                else dead = c;
            }
            if (!pass) ++(alive == 4u ? info->quads_two : alive == 3u ? info->quads_one : info->quads_none);
            if (alive < 3u) continue;
            // every triangle is the cyclic order A, B, C, D with one corner left out
            const uint32_t drops[2] = {alive == 4u ? 3u : dead, 1u};
            for (uint32_t t = 0; t < (alive == 4u ? 2u : 1u); ++t) {
                uint32_t v[3], k = 0;
                for (uint32_t c = 0; c < 4u; ++c)
                    if (c != drops[t]) v[k++] = r[c];
                bool cut = false;
                if (cutting)
                    for (int x = 0; x < 3 && !cut; ++x) {
                        volatile float d = vertices[v[x]].mean - vertices[v[(x + 1) % 3]].mean;   // one fp32 operation, rounded once
                        cut = fabsf(d) > step;
                    }
                if (cut) {
                    if (!pass) ++info->cut_by_step;
                    continue;
                }
                if (pass) {
                    gm_wall_mesh_triangle &o = triangles[nt];
                    o.v[0] = v[0];
                    o.v[1] = outward ? v[2] : v[1];
                    o.v[2] = outward ? v[1] : v[2];
                }
                ++nt;
            }
        }
        if (!pass) {
            info->triangles = nt;
            if (n_out) *n_out = nt;
            if (!triangles) return GM_OK;                  // (capacity 0: a count query)
            if (capacity < nt) return GM_ERR_CAPACITY;
        }
    }
    return GM_OK;
}

gm_status gm_wall_mesh_write_ply(const char *path, const gm_wall_cloud_point *vertices, uint64_t n_vertices,
                                 const gm_wall_mesh_triangle *triangles, uint64_t n_triangles)
{
    const uint16_t probe = 1;
    if (!path || (!vertices && n_vertices) || (!triangles && n_triangles) || *(const uint8_t *)&probe != 1u) return GM_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n_triangles; ++i)
        for (int k = 0; k < 3; ++k)
            if (triangles[i].v[k] >= n_vertices) return GM_ERR_INVALID_ARG;
    FILE *f = fopen(path, "wb");
    if (!f) return GM_ERR_DEVICE;
    bool ok = fprintf(f,
                      "ply\nformat binary_little_endian 1.0\ncomment gm_wall_map_mesh\nelement vertex %llu\n"
                      "property float x\nproperty float y\nproperty float z\nproperty float mean\nproperty float min\n"
                      "property float max\nelement face %llu\nproperty list uchar uint vertex_indices\nend_header\n",
                      (unsigned long long)n_vertices, (unsigned long long)n_triangles) > 0;
    std::vector<uint8_t> buf;
    const size_t kRows = 4096;   // records per write
    buf.resize(kRows * 24);
    for (uint64_t i = 0; ok && i < n_vertices; i += kRows) {
        const size_t m = (size_t)std::min<uint64_t>(kRows, n_vertices - i);
        for (size_t j = 0; j < m; ++j) memcpy(&buf[j * 24], &vertices[i + j], 24);   // x, y, z, mean, min, max lead the record
        ok = fwrite(buf.data(), 24, m, f) == m;
    }
    for (uint64_t i = 0; ok && i < n_triangles; i += kRows) {
        const size_t m = (size_t)std::min<uint64_t>(kRows, n_triangles - i);
        for (size_t j = 0; j < m; ++j) {
            buf[j * 13] = 3u;
            memcpy(&buf[j * 13 + 1], triangles[i + j].v, 12);
        }
        ok = fwrite(buf.data(), 13, m, f) == m;
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? GM_OK : GM_ERR_DEVICE;
}

void gm_wall_section_default_params(gm_wall_section_params *p)
{
    if (!defaults_begin(p)) return;
    p->section_stations = 4;
    p->harmonics = 2;
    p->passes = 3;
    p->min_count = 8;
    p->min_columns = 24;
    p->max_gap_deg = 90.0;
    p->reject = 0.05;
}

gm_status gm_wall_section_check_params(const gm_wall_section_params *p)
{
    long long Tr;
    return p && section_prm_ok(*p, Tr) ? GM_OK : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_section_basis(uint32_t n_sectors, uint32_t harmonics, int32_t *basis, uint32_t capacity, uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (n_sectors < 1u || n_sectors > GM_WALL_MAX_SECTORS || harmonics > GM_WALL_SECTION_MAX_HARMONICS || (!basis && capacity))
        return GM_ERR_INVALID_ARG;
    const uint32_t entries = n_sectors * (1u + 2u * harmonics);
    if (n_out) *n_out = entries;
    if (!basis && !capacity) return GM_OK;
    if (capacity < entries) return GM_ERR_CAPACITY;
    section_basis(n_sectors, harmonics, basis);
    return GM_OK;
}

gm_status gm_wall_section_solve(const gm_wall_section_sums *sums, uint32_t harmonics, uint32_t min_columns, int64_t coef_q[9],
                                uint32_t *status)
{
    if (!sums || !coef_q || !status || harmonics > GM_WALL_SECTION_MAX_HARMONICS || min_columns < 1u) return GM_ERR_INVALID_ARG;
    *status = section_solve(*sums, harmonics, min_columns, coef_q);
    return GM_OK;
}

gm_status gm_wall_section_metrics(const gm_wall_params *p, const gm_wall_section *s, uint32_t harmonics,
                                  struct gm_wall_section_metrics *out)
{
    if (!p || !s || !out || check_params(p) != GM_OK || harmonics > GM_WALL_SECTION_MAX_HARMONICS || s->stations < 1u)
        return GM_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double from = (double)s->station_from * p->station_length;
    const double end = (double)s->station_from + (double)s->stations;
    const double to = end * p->station_length;
    out->chainage_from = p->t_min + from;
    out->chainage_to = p->t_min + to;
    if (s->status & GM_SECTION_FAILED_MASK) return GM_OK;
    const uint32_t P = 1u + 2u * harmonics;
    double c[9];
    for (uint32_t q = 0; q < 9u; ++q) c[q] = q < P ? (double)s->coef_q[q] * 0x1p-20 : 0.0;
    DesignFrame d;
    design_frame_of(*p, d);
    const double radius = d.R + c[0];
    out->radius_m = radius;
    out->radial_m = c[0];
    out->centre_u = c[1];
    out->centre_v = c[2];
    const double both = out->chainage_from + out->chainage_to;
    const double mid = both * 0.5;
    for (int k = 0; k < 3; ++k) {
        const double along = mid * d.a[k];
        const double cu = c[1] * d.u[k];
        const double cv = c[2] * d.v[k];
        const double s1 = d.o[k] + along;
        const double s2 = s1 + cu;
        out->centre[k] = s2 + cv;
    }
    const double oval = hypot(c[3], c[4]);
    out->oval_m = oval;
    if (oval > 0.0) {
        const double ang = atan2(c[4], c[3]);
        const double half = ang * 0.5;
        const double scaled = half * 180.0;
        double deg = scaled / 3.14159265358979323846;
        if (deg < 0.0) deg = deg + 180.0;
        if (deg >= 180.0) deg = deg - 180.0;
        out->oval_angle_deg = deg;
    }
    const double rmax = radius + oval;
    const double rmin = radius - oval;
    out->diameter_max = 2.0 * rmax;
    out->diameter_min = 2.0 * rmin;
    if (s->accepted) {
        const double msq = (double)s->rss / (double)s->accepted;
        const double root = sqrt(msq);
        out->rms_m = root * 0x1p-20;
    }
    const double r2 = radius * radius;
    double sq = 0.0;
    for (uint32_t q = 1; q < P; ++q) {
        const double t = c[q] * c[q];
        sq = sq + t;
    }
    const double a0 = 3.14159265358979323846 * r2;
    const double a1 = 1.57079632679489661923 * sq;
    out->area_m2 = a0 + a1;
    out->coverage = (double)s->accepted / (double)p->n_sectors;
    return GM_OK;
}

void gm_wall_quantity_default_params(gm_wall_quantity_params *p)
{
    if (!defaults_begin(p)) return;
    p->section_stations = 4;
    p->min_count = 8;
}

gm_status gm_wall_quantity_check_params(const gm_wall_params *p, const gm_wall_quantity_params *q, const int32_t *lo_q,
                                        const int32_t *hi_q, uint32_t n_profiles, const uint8_t *section_profile, uint32_t n,
                                        const uint8_t *zone, uint32_t n_zones)
{
    long long Rq;
    return quantity_ok(p, params_or(q, gm_wall_quantity_default_params), lo_q, hi_q, n_profiles, section_profile, n, zone, n_zones, Rq)
               ? GM_OK
               : GM_ERR_INVALID_ARG;
}

gm_status gm_wall_quantity_column(int64_t radius_q, uint64_t count, int64_t sum, int has_baseline, uint64_t base_count,
                                  int64_t base_sum, uint32_t min_count, int32_t lo, int32_t hi, uint32_t zone_entry,
                                  gm_wall_quantity_column_result *out)
{
    if (!out || radius_q < 1 || radius_q > (1ll << 32) || min_count < 1u || lo < -(int32_t)kWallSectionSat ||
        hi > (int32_t)kWallSectionSat || lo > hi)
        return GM_ERR_INVALID_ARG;
    const WallQuantityColumn c = wall_quantity_column(radius_q, count, sum, has_baseline != 0, base_count, base_sum, min_count, lo, hi,
                                                      zone_entry == GM_WALL_QUANTITY_UNMEASURED);
    out->cls = c.cls;
    out->v = c.usable ? (int32_t)c.v : kWallQuantityNoValue;
    out->under_area = c.under;
    out->over_area = c.over;
    out->excess_area = c.excess;
    out->over_line = c.line;
    return GM_OK;
}

// ((area 2^-20) pi) / n_sectors, then times the length: one operation per statement
struct QuantityVolumes { double area[4], volume[4]; };   // under, over, excess, paid
static QuantityVolumes quantity_volumes(const gm_wall_params &p, const gm_wall_quantity &r, double length)
{
    const int64_t units[4] = {r.under_area, r.over_area, r.excess_area, r.over_area - r.excess_area};
    QuantityVolumes q;
    for (int i = 0; i < 4; ++i) {
        const double scaled = (double)units[i] * 0x1p-20;
        const double ring = scaled * 3.14159265358979323846;
        q.area[i] = ring / (double)p.n_sectors;
        q.volume[i] = q.area[i] * length;
    }
    return q;
}

static double quantity_angle(uint32_t sector, uint32_t nsec)   // gm_wall_clearance_run.angle_deg
{
    const double num = 360.0 * ((double)sector * 2.0 + 1.0);
    return num / ((double)nsec * 2.0);
}

gm_status gm_wall_quantity_metrics(const gm_wall_params *p, const gm_wall_quantity *r, struct gm_wall_quantity_metrics *out)
{
    if (!p || !r || !out || check_params(p) != GM_OK || r->stations < 1u) return GM_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double from = (double)r->station_from * p->station_length;
    const double end = (double)r->station_from + (double)r->stations;
    const double to = end * p->station_length;
    out->chainage_from = p->t_min + from;
    out->chainage_to = p->t_min + to;
    out->length = (double)r->stations * p->station_length;
    const QuantityVolumes q = quantity_volumes(*p, *r, out->length);
    out->under_area_m2 = q.area[0]; out->over_area_m2 = q.area[1]; out->excess_area_m2 = q.area[2]; out->paid_area_m2 = q.area[3];
    out->under_volume_m3 = q.volume[0]; out->over_volume_m3 = q.volume[1]; out->excess_volume_m3 = q.volume[2];
    out->paid_volume_m3 = q.volume[3];
    out->peak_under_m = (double)r->peak_under * 0x1p-20;
    out->peak_over_m = (double)r->peak_over * 0x1p-20;
    if (r->peak_under_sector != UINT32_MAX) out->peak_under_angle_deg = quantity_angle(r->peak_under_sector, p->n_sectors);
    if (r->peak_over_sector != UINT32_MAX) out->peak_over_angle_deg = quantity_angle(r->peak_over_sector, p->n_sectors);
    const uint64_t usable = (uint64_t)r->under + r->within + r->over, measured = usable + r->unsurveyed;
    if (measured) out->coverage = (double)usable / (double)measured;
    return GM_OK;
}

gm_status gm_wall_quantity_runs(const gm_wall_params *p, const gm_wall_quantity *records, uint32_t n_sections, uint32_t n_zones,
                                uint32_t run_sections, uint32_t flags, gm_wall_quantity_run *runs, uint32_t capacity,
                                uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || check_params(p) != GM_OK || (!records && n_sections) || n_zones < 1u || n_zones > GM_WALL_QUANTITY_MAX_ZONES ||
        run_sections < 1u || (flags & ~(uint32_t)GM_WALL_QUANTITY_RUNS_ALL_ZONES) || (!runs && capacity))
        return GM_ERR_INVALID_ARG;
    const bool all = (flags & GM_WALL_QUANTITY_RUNS_ALL_ZONES) != 0u;
    const uint32_t NR = n_sections ? (n_sections - 1u) / run_sections + 1u : 0u, per = all ? 1u : n_zones;
    const uint64_t total = (uint64_t)NR * per;
    if (total > UINT32_MAX) return GM_ERR_INVALID_ARG;
    if (n_out) *n_out = (uint32_t)total;
    if (!runs) return GM_OK;
    if (capacity < total) return GM_ERR_CAPACITY;
    for (uint32_t R = 0; R < NR; ++R) {
        const uint32_t s0 = R * run_sections, s1 = n_sections - s0 < run_sections ? n_sections : s0 + run_sections;
        for (uint32_t o = 0; o < per; ++o) {
            gm_wall_quantity_run run;
            memset(&run, 0, sizeof(run));
            const gm_wall_quantity &head = records[(size_t)s0 * n_zones];
            run.station_from = head.station_from;
            run.zone = all ? UINT32_MAX : o;
            run.sections = s1 - s0;
            run.peak_under_station = run.peak_under_sector = run.peak_over_station = run.peak_over_sector = UINT32_MAX;
            for (uint32_t s = s0; s < s1; ++s) {
                const gm_wall_quantity &first = records[(size_t)s * n_zones];
                run.stations += first.stations;
                const double length = (double)first.stations * p->station_length;
                for (uint32_t z = all ? 0u : o; z < (all ? n_zones : o + 1u); ++z) {
                    const gm_wall_quantity &r = records[(size_t)s * n_zones + z];
                    run.under += r.under; run.within += r.within; run.over += r.over; run.unsurveyed += r.unsurveyed;
                    run.points += r.points;
                    const QuantityVolumes q = quantity_volumes(*p, r, length);
                    run.under_volume_m3 = run.under_volume_m3 + q.volume[0];
                    run.over_volume_m3 = run.over_volume_m3 + q.volume[1];
                    run.excess_volume_m3 = run.excess_volume_m3 + q.volume[2];
                    run.paid_volume_m3 = run.paid_volume_m3 + q.volume[3];
                    if (r.peak_under_sector != UINT32_MAX && r.peak_under > run.peak_under) {
                        run.peak_under = r.peak_under;
                        run.peak_under_station = r.station_from;
                        run.peak_under_sector = r.peak_under_sector;
                    }
                    if (r.peak_over_sector != UINT32_MAX && r.peak_over > run.peak_over) {
                        run.peak_over = r.peak_over;
                        run.peak_over_station = r.station_from;
                        run.peak_over_sector = r.peak_over_sector;
                    }
                }
            }
            const double from = (double)run.station_from * p->station_length;
            const double end = (double)run.station_from + (double)run.stations;
            const double to = end * p->station_length;
            run.chainage_from = p->t_min + from;
            run.chainage_to = p->t_min + to;
            runs[(size_t)R * per + o] = run;
        }
    }
    return GM_OK;
}

gm_status gm_wall_gauge_from_polygon(const gm_wall_params *p, const double *uv, uint32_t n_vertices, const double offset[2],
                                     int32_t *gauge_q, uint32_t capacity, uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || !uv || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || p->n_sectors > GM_WALL_MAX_SECTORS) return GM_ERR_INVALID_ARG;
    if (n_vertices < 3u || n_vertices > GM_WALL_GAUGE_MAX_VERTICES || (!gauge_q && capacity)) return GM_ERR_INVALID_ARG;
    if (offset && (!isfinite(offset[0]) || !isfinite(offset[1]))) return GM_ERR_INVALID_ARG;
    const uint32_t ns = p->n_sectors, nv = n_vertices;
    std::vector<double> P(2 * (size_t)nv);
    for (uint32_t i = 0; i < nv; ++i) {
        P[2 * i] = uv[2 * i] + (offset ? offset[0] : 0.0);
        P[2 * i + 1] = uv[2 * i + 1] + (offset ? offset[1] : 0.0);
    }
    if (!gauge_polygon_ok(P, nv)) return GM_ERR_INVALID_ARG;
    std::vector<double> dirs(2 * (size_t)ns + 2), r(nv);
    for (uint32_t k = 0; k < ns; ++k) {
        const double f = (double)k / (double)ns;
        const double phi = kTwoPi * f;
        dirs[2 * k] = cos(phi);
        dirs[2 * k + 1] = sin(phi);
    }
    dirs[2 * ns] = dirs[0]; dirs[2 * ns + 1] = dirs[1];   // the last ray is the first
    for (uint32_t i = 0; i < nv; ++i) r[i] = sqrt(P[2 * i] * P[2 * i] + P[2 * i + 1] * P[2 * i + 1]);
    // where the ray of every sector start leaves the polygon at the farthest: the largest t >= 0 over the edges it meets
    std::vector<double> ray(ns, -1.0);
    for (uint32_t k = 0; k < ns; ++k) {
        const double *d = &dirs[2 * k];
        for (uint32_t i = 0; i < nv; ++i) {
            const double *a = &P[2 * i], *b = &P[2 * ((i + 1u) % nv)];
            const double e[2] = {b[0] - a[0], b[1] - a[1]};
            const double den = cross2(e, d);
            if (den == 0.0) continue;   // parallel: its ends are vertices of the wedge
            const double s = -cross2(a, d) / den;
            if (!(s >= 0.0) || !(s <= 1.0)) continue;
            const double x[2] = {a[0] + s * e[0], a[1] + s * e[1]};
            const double t = x[0] * d[0] + x[1] * d[1];
            if (t >= 0.0 && t > ray[k]) ray[k] = t;
        }
    }
    std::vector<int32_t> out(ns);
    for (uint32_t k = 0; k < ns; ++k) {
        const double *d0 = &dirs[2 * k], *d1 = &dirs[2 * k + 2];
        double g = std::max(ray[k], ray[(k + 1u) % ns]);
        for (uint32_t i = 0; i < nv; ++i) {
            const double *v = &P[2 * i];
            if (ns == 1u || (cross2(d0, v) >= 0.0 && cross2(v, d1) >= 0.0)) g = std::max(g, r[i]);
        }
        const double q = ceil(g * 1048576.0);
        if (!(g > 0.0) || !(q < 2147483648.0)) return GM_ERR_INVALID_ARG;
        out[k] = (int32_t)q;
    }
    if (n_out) *n_out = ns;
    if (capacity < ns) return GM_ERR_CAPACITY;
    memcpy(gauge_q, out.data(), (size_t)ns * sizeof(int32_t));
    return GM_OK;
}

gm_status gm_wall_clearance_runs(const gm_wall_params *p, const gm_wall_clearance_station *stations, uint32_t n,
                                 uint32_t station0, uint32_t max_gap, gm_wall_clearance_run *runs, uint32_t capacity,
                                 uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!p || p->struct_size != sizeof(gm_wall_params) || p->n_sectors < 1u || (!stations && n) || (!runs && capacity) ||
        (uint64_t)station0 + n > 4294967296ull)
        return GM_ERR_INVALID_ARG;
    auto flagged = [&](uint32_t i) { return stations[i].tight + stations[i].infringed > 0u; };
    std::vector<gm_wall_clearance_run> out;
    for (uint32_t i = 0; i < n;) {
        if (!flagged(i)) { ++i; continue; }
        uint32_t last = i;
        for (uint32_t j = i + 1u; j < n && (uint64_t)j - last <= (uint64_t)max_gap + 1u; ++j)
            if (flagged(j)) last = j;
        gm_wall_clearance_run r;
        memset(&r, 0, sizeof(r));
        r.station_from = station0 + i;
        r.station_to = station0 + last;
        uint32_t at = i;
        for (uint32_t j = i; j <= last; ++j) {
            if (stations[j].min_clearance < stations[at].min_clearance) at = j;
            r.tight += stations[j].tight;
            r.infringed += stations[j].infringed;
        }
        // one operation per statement: the same roundings as the twin's, whatever the compiler may contract
        const double from = (double)r.station_from * p->station_length;
        const double to = ((double)r.station_to + 1.0) * p->station_length;
        r.chainage_from = p->t_min + from;
        r.chainage_to = p->t_min + to;
        r.min_clearance = stations[at].min_clearance;
        r.min_clearance_m = (double)r.min_clearance * 0x1p-20;
        r.min_station = station0 + at;
        r.min_sector = stations[at].min_sector;
        const double num = 360.0 * ((double)r.min_sector * 2.0 + 1.0);
        r.angle_deg = num / ((double)p->n_sectors * 2.0);
        out.push_back(r);
        i = last + 1u;
    }
    if (n_out) *n_out = (uint32_t)out.size();
    if (runs && capacity < out.size()) return GM_ERR_CAPACITY;
    if (runs && !out.empty()) memcpy(runs, out.data(), out.size() * sizeof(gm_wall_clearance_run));
    return GM_OK;
}

gm_status gm_wall_align_select(const gm_wall_params *wall, const gm_wall_align_params *prm, const double pose[12],
                               const gm_wall_align_score *table, uint32_t n_scores, gm_wall_align_info *info)
{
    if (!wall || !pose || !table || !info || check_params(wall) != GM_OK) return GM_ERR_INVALID_ARG;
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    if (!align_prm_ok(ap, wall->n_sectors)) return GM_ERR_INVALID_ARG;
    if (n_scores != (2u * ap.max_station_shift + 1u) * (2u * ap.max_sector_shift + 1u)) return GM_ERR_INVALID_ARG;
    double Rm[3][3], tr[3];
    if (pose_split(pose, Rm, tr)) return GM_ERR_INVALID_ARG;
    DesignFrame d;
    design_frame_of(*wall, d);
    const double rel[3] = {tr[0] - d.o[0], tr[1] - d.o[1], tr[2] - d.o[2]};
    if (!(fabs(floor((dot(rel, d.a) - wall->t_min) / wall->station_length)) < 4.0e18)) return GM_ERR_INVALID_ARG;
    align_select(d, *wall, ap, Rm, tr, table, info);
    return GM_OK;
}

}  // extern "C"
