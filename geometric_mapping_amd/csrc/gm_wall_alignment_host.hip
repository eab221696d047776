// gm_wall_alignment_host.hip -- the part of the wall alignment's C ABI that needs no device (include/gm_hip.h states the
// rule): the chaining of the element maps, the joint planes, ownership, project, point, the chainage window, the plan
// of an add, and the windows and metrics of the objects and the regions on the global station grid.  Every element is a DesignAxis (gm_wall_map.hpp): its section, project, point and per-add frame are the
// element map's own, asked of the axis.  Like gm_wall_host.hip it links against libm and the C++ library alone;
// host/gm_wall_alignment_host_test.cpp runs it under the host sanitizers.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define GM_WALL_HOST_ONLY
#include "gm_wall_map.hpp"

using namespace gm;
using namespace gm::wall;

namespace gm {
namespace wall {

static_assert(GM_WALL_ELEMENT_STRAIGHT == kAxisStraight && GM_WALL_ELEMENT_ARC == kAxisArc && GM_WALL_ELEMENT_CLOTHOID == kAxisClothoid,
              "an element's kind is its axis' kind");

gm_status alignment_build(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, Alignment &A)
{
    A.el.clear();
    if (!params || !elements || n < 1u || n > GM_WALL_ALIGNMENT_MAX_ELEMENTS) return GM_ERR_INVALID_ARG;
    gm_wall_params t = *params;
    t.n_stations = 1u;
    if (check_params(&t) != GM_OK) return GM_ERR_INVALID_ARG;
    const double ds = params->station_length;
    try {
        A.el.resize(n);
    } catch (...) {
        return GM_ERR_OOM;
    }
    double s = params->t_min;
    for (uint32_t i = 0; i < n; ++i) {
        const gm_wall_element &e = elements[i];
        if (e.struct_size != sizeof(gm_wall_element) || e.reserved != 0u || e.kind > GM_WALL_ELEMENT_CLOTHOID || e.n_stations < 1u)
            return GM_ERR_INVALID_ARG;
        AlignElem &E = A.el[i];
        E.p = t;
        E.p.n_stations = e.n_stations;
        E.s_start = s;
        E.s_end = s + (double)e.n_stations * ds;
        memset(&E.arc, 0, sizeof(E.arc));
        memset(&E.cl, 0, sizeof(E.cl));
        if (!isfinite(E.s_end)) return GM_ERR_INVALID_ARG;
        if (i > 0u) {   // the frame at the end of the element before: its point, direction = forward, up
            const AlignElem &B = A.el[i - 1u];
            double v[3];
            B.ax.frame(B.p.t_min + (double)B.p.n_stations * B.p.station_length, E.p.point, E.p.direction, E.p.up, v);
            for (int k = 0; k < 3; ++k) E.p.forward[k] = E.p.direction[k];
            E.p.t_min = s;
        }
        if (check_params(&E.p) != GM_OK) return GM_ERR_INVALID_ARG;
        DesignFrame d;
        design_frame_of(E.p, d);
        if (e.kind != GM_WALL_ELEMENT_STRAIGHT) {
            const double tl = sqrt(e.turn[0] * e.turn[0] + e.turn[1] * e.turn[1]);
            if (!isfinite(tl) || !(tl > 0.0) || !isfinite(e.curvature)) return GM_ERR_INVALID_ARG;
            const double t0 = e.turn[0] / tl, t1 = e.turn[1] / tl;
            double m[3];
            for (int k = 0; k < 3; ++k) m[k] = t0 * d.u[k] + t1 * d.v[k];
            if (e.kind == GM_WALL_ELEMENT_ARC) {
                if (!(e.curvature > 0.0)) return GM_ERR_INVALID_ARG;
                E.arc.struct_size = (uint32_t)sizeof(gm_wall_arc);
                for (int k = 0; k < 3; ++k) E.arc.curvature[k] = e.curvature * m[k];
                E.arc.point_chainage = s;
            } else {
                E.cl.struct_size = (uint32_t)sizeof(gm_wall_clothoid);
                for (int k = 0; k < 3; ++k) E.cl.normal[k] = m[k];
                E.cl.curvature = e.curvature;
                E.cl.rate = e.rate;
                E.cl.point_chainage = s;
            }
        } else if (i > 0u) {   // the straight rule's own chainage of `point`
            E.p.t_min = dot(E.p.point, d.a);
        }
        const gm_status st = axis_check(&E.p, E.arc.struct_size ? &E.arc : nullptr, E.cl.struct_size ? &E.cl : nullptr, E.ax);
        if (st != GM_OK) return st == GM_ERR_OOM ? GM_ERR_OOM : GM_ERR_INVALID_ARG;
        E.ax.offset = s - E.p.t_min;   // (0 but on a straight element behind the first)
        s = E.s_end;
    }
    A.ds = ds;
    return GM_OK;
}

// d_i(x) < 0 for joint i (between elements i and i + 1)
static bool before_joint(const Alignment &A, uint32_t i, const double x[3])
{
    const AlignElem &N = A.el[i + 1u];
    const double r[3] = {x[0] - N.p.point[0], x[1] - N.p.point[1], x[2] - N.p.point[2]};
    return dot(r, N.ax.d.a) < 0.0;
}

// The owner looks at an element's OWN two joints only: element i is a candidate when x lies on its side of both (not before
// the joint at its start, before the joint at its end; the alignment's two ends are open).  There is always one: the element
// before the first joint x lies before, or the last.  An alignment that turns a quarter turn or more brings x between the
// joints of an element far away as well; of several candidates the owner is the one whose axis, cut to its span, is
// nearest to x (ties: the lowest index).
void alignment_project(const Alignment &A, const double x[3], uint32_t &element, double &chainage, double &angle, double &e)
{
    const uint32_t n = (uint32_t)A.el.size();
    double best = INFINITY;
    bool have = false;
    bool after_prev = true;   // x is not before the joint at this element's start
    for (uint32_t i = 0; i < n; ++i) {
        const bool before_next = i + 1u < n ? before_joint(A, i, x) : true;
        const bool candidate = after_prev && before_next;
        after_prev = !before_next;
        if (!candidate) continue;
        const AlignElem &E = A.el[i];
        double s, ph, ee;
        E.ax.project(x, s, ph, ee);   // the element's own rule, in the alignment's chainage
        const double over = s < E.s_start ? E.s_start - s : (s > E.s_end ? s - E.s_end : 0.0);
        const double rho = ee + E.ax.d.R;
        double dist = sqrt(rho * rho + over * over);
        if (!isfinite(dist)) dist = INFINITY;
        if (!have || dist < best) {
            have = true;
            best = dist;
            element = i;
            chainage = s;
            angle = ph;
            e = ee;
        }
    }
}

uint32_t alignment_owner(const Alignment &A, const double x[3])
{
    uint32_t el = 0;
    double s, ph, e;
    alignment_project(A, x, el, s, ph, e);
    return el;
}

void alignment_point(const Alignment &A, double chainage, double angle, double rho, double xyz[3])
{
    uint32_t i = 0;
    while (i + 1u < (uint32_t)A.el.size() && chainage >= A.el[i].s_end) ++i;
    A.el[i].ax.point(chainage, angle, rho, xyz);
}

gm_status alignment_add_plan(const Alignment &A, const double pose[12], double bound, gm_wall_alignment_add_info *info)
{
    double Rm[3][3], tr[3];
    if (!pose || !info || !isfinite(bound) || !(bound > 0.0) || pose_split(pose, Rm, tr)) return GM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_add_info);
    uint32_t el = 0;
    double s = 0.0, angle = 0.0, e = 0.0;
    alignment_project(A, tr, el, s, angle, e);
    if (!isfinite(s)) return GM_ERR_INVALID_ARG;
    const double L = 2.0 * bound * 1.7320508075688772 + A.ds;
    info->element = el;
    info->chainage = s;
    info->reach = L;
    info->offset = A.el[el].ax.offset;
    uint32_t lo = el, hi = el;
    while (lo > 0u && A.el[lo - 1u].s_end > s - L) --lo;
    while (hi + 1u < (uint32_t)A.el.size() && A.el[hi + 1u].s_start < s + L) ++hi;
    const uint32_t ns = hi - lo + 1u;
    if (ns > GM_WALL_JOINT_MAX_SIDES) return GM_ERR_UNSUPPORTED;
    info->n_sides = ns;
    for (uint32_t k = 0; k < ns; ++k) {
        const AlignElem &E = A.el[lo + k];
        info->side_element[k] = lo + k;
        info->status |= E.ax.d.status;
        AxisAddFrame f;   // of the element map's own add
        if (!E.ax.add_frame(E.p, Rm, tr, f)) return GM_ERR_INVALID_ARG;
        info->side_anchor[k] = f.anchor;
        if (k + 1u < ns) {
            const AlignElem &N = A.el[lo + k + 1u];
            const double r[3] = {N.p.point[0] - tr[0], N.p.point[1] - tr[1], N.p.point[2] - tr[2]};
            for (int c = 0; c < 3; ++c) {   // Rm^T x
                info->joint_o[k][c] = (float)(Rm[0][c] * r[0] + Rm[1][c] * r[1] + Rm[2][c] * r[2]);
                info->joint_a[k][c] = (float)(Rm[0][c] * N.ax.d.a[0] + Rm[1][c] * N.ax.d.a[1] + Rm[2][c] * N.ax.d.a[2]);
            }
        }
    }
    return GM_OK;
}

// The section of element E at its own add's anchor station in map coordinates, not rounded: S = o, a, n, b on a curved
// element (o, a, u, v on a straight one), (u, v) = u(s_f), v(s_f), and ax = kappa_f, rate, un, ub, vn, vb as the add rounds them.
static void element_anchor_section(const AlignElem &E, int64_t anchor, double S[4][3], double u[3], double v[3], float ax[6])
{
    const DesignAxis &X = E.ax;
    const bool straight = X.kind == kAxisStraight;
    const double kf = X.station_section(E.p, (double)anchor, S[1], S[2], S[0]);
    for (int k = 0; k < 3; ++k) {
        S[3][k] = straight ? X.d.v[k] : X.b[k];
        u[k] = straight ? S[2][k] : X.un * S[2][k] + X.ub * S[3][k];
        v[k] = straight ? S[3][k] : X.vn * S[2][k] + X.vb * S[3][k];
    }
    ax[0] = (float)kf; ax[1] = (float)X.cl.rate;   // (0 where the axis has none)
    ax[2] = (float)X.un; ax[3] = (float)X.ub; ax[4] = (float)X.vn; ax[5] = (float)X.vb;
}

gm_status alignment_locate_start(const Alignment &A, const double pose[12], double bound, gm_wall_alignment_locate_start *out)
{
    if (!out) return GM_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(gm_wall_alignment_locate_start);
    GMW_OK(alignment_add_plan(A, pose, bound, &out->add));
    double Rm[3][3], tr[3];
    (void)pose_split(pose, Rm, tr);   // (accepted by the plan)
    const gm_wall_alignment_add_info &pl = out->add;
    out->home = pl.element - pl.side_element[0];
    // the home section and the start
    double H[4][3], hu[3], hv[3];
    float ax[6];
    element_anchor_section(A.el[pl.element], pl.side_anchor[out->home], H, hu, hv, ax);
    const double *of = H[0], *ha = H[1];
    for (int c = 0; c < 3; ++c) {   // Rm^T x
        const double r[3] = {of[0] - tr[0], of[1] - tr[1], of[2] - tr[2]};
        out->c[c] = Rm[0][c] * r[0] + Rm[1][c] * r[1] + Rm[2][c] * r[2];
        out->d[c] = Rm[0][c] * ha[0] + Rm[1][c] * ha[1] + Rm[2][c] * ha[2];
        out->u[c] = Rm[0][c] * hu[0] + Rm[1][c] * hu[1] + Rm[2][c] * hu[2];
        out->v[c] = Rm[0][c] * hv[0] + Rm[1][c] * hv[1] + Rm[2][c] * hv[2];
        out->o_f[c] = of[c]; out->a[c] = ha[c]; out->fu[c] = hu[c]; out->fv[c] = hv[c];
    }
    out->s0 = -dot(out->c, out->d);
    auto coords = [&](const double *x, bool point, double *h) {
        const double r[3] = {point ? x[0] - of[0] : x[0], point ? x[1] - of[1] : x[1], point ? x[2] - of[2] : x[2]};
        h[0] = dot(r, ha); h[1] = dot(r, hu); h[2] = dot(r, hv);
    };
    for (uint32_t k = 0; k < pl.n_sides; ++k) {
        const AlignElem &E = A.el[pl.side_element[k]];
        double S[4][3], su[3], sv[3];
        element_anchor_section(E, pl.side_anchor[k], S, su, sv, out->side_axis[k]);
        out->side_kind[k] = (uint32_t)E.ax.kind;
        for (int q = 0; q < 4; ++q) coords(S[q], q == 0, &out->side[k][3 * q]);
        if (k == out->home) {   // exactly itself
            const bool straight = E.ax.kind == kAxisStraight;
            for (int q = 0; q < (straight ? 4 : 2); ++q)
                for (int c = 0; c < 3; ++c) out->side[k][3 * q + c] = q > 0 && c == q - 1 ? 1.0 : 0.0;
        }
        if (k + 1u < pl.n_sides) {
            const AlignElem &N = A.el[pl.side_element[k] + 1u];
            coords(N.p.point, true, &out->joint[k][0]);
            coords(N.ax.d.a, false, &out->joint[k][3]);
        }
    }
    return GM_OK;
}

// F(x) of include/gm_hip.h's align rule: the design frame at alignment chainage x, on the element the point rule picks
void alignment_frame(const Alignment &A, double x, double o[3], double a[3], double u[3], double v[3])
{
    uint32_t i = 0;
    while (i + 1u < (uint32_t)A.el.size() && x >= A.el[i].s_end) ++i;
    const DesignAxis &X = A.el[i].ax;
    X.frame(x - X.offset, o, a, u, v);   // (the offset is 0 but on a straight element behind the first)
}

gm_status alignment_align_plan(const Alignment &A, const double pose[12], double bound, const gm_wall_align_params &ap,
                               gm_wall_alignment_align_plan_info *out)
{
    if (!out) return GM_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(gm_wall_alignment_align_plan_info);
    if (A.el.empty() || !align_prm_ok(ap, A.el[0].p.n_sectors)) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_add_plan(A, pose, bound, &out->add));
    const gm_wall_alignment_add_info &pl = out->add;
    const int64_t P = (int64_t)ap.half_patch_stations, Ash = (int64_t)ap.max_station_shift;
    std::vector<int64_t> base;
    try {
        base.resize(A.el.size() + 1u);
    } catch (...) {
        return GM_ERR_OOM;
    }
    base[0] = 0;
    for (size_t i = 0; i < A.el.size(); ++i) base[i + 1u] = base[i] + (int64_t)A.el[i].p.n_stations;
    out->total = base[A.el.size()];
    out->home = pl.element - pl.side_element[0];
    const int64_t Gf = base[pl.element] + pl.side_anchor[out->home];   // (|anchor| < 4e18, base < 2^40: no overflow)
    out->anchor_global = Gf;
    for (uint32_t k = 0; k < pl.n_sides; ++k) {
        const int64_t r0 = ((base[pl.side_element[k]] + pl.side_anchor[k]) - Gf) + P;
        if (r0 < -2147483647ll - 1 || r0 > 2147483647ll) return GM_ERR_INVALID_ARG;
        out->row0[k] = (int32_t)r0;
    }
    // the pieces: the elements the image rows [G_f - P - A, G_f + P + A) meet, ascending
    const int64_t g0 = (Gf - P) - Ash, g1 = (Gf + P) + Ash;
    uint32_t np = 0;
    for (size_t i = 0; i < A.el.size(); ++i) {
        if (!(base[i] < g1 && base[i + 1u] > g0)) continue;
        if (np == GM_WALL_ALIGN_MAX_PIECES) {
            out->n_pieces = 0;
            memset(out->piece, 0, sizeof(out->piece));
            return GM_ERR_UNSUPPORTED;
        }
        out->piece[np].element = (uint32_t)i;
        out->piece[np].n_stations = A.el[i].p.n_stations;
        out->piece[np].first_row = base[i];
        ++np;
    }
    out->n_pieces = np;
    out->own = (pl.n_sides == 1u && A.el[pl.element].ax.kind == kAxisStraight && (np == 0u || (np == 1u && out->piece[0].element == pl.element)))
                   ? 1u : 0u;
    return GM_OK;
}

// the selection of `table` and the pose of include/gm_hip.h's align rule; everything of info but the device's counts
gm_status alignment_align_select(const Alignment &A, const double pose[12], const gm_wall_align_params &ap,
                                 const gm_wall_alignment_align_plan_info &plan, const gm_wall_align_score *table,
                                 gm_wall_alignment_align_info *info)
{
    double Rm[3][3], tr[3];
    if (!table || !info || pose_split(pose, Rm, tr)) return GM_ERR_INVALID_ARG;
    static_assert(offsetof(gm_wall_alignment_align_info, element) == sizeof(gm_wall_align_info), "the shared head");
    memset(info, 0, sizeof(*info));
    const gm_wall_params &wp = A.el[plan.add.element].p;
    gm_wall_align_info head;
    const bool ok = align_select_table(ap, wp.station_length, wp.n_sectors, table, &head);
    head.anchor_station = plan.add.side_anchor[plan.home];
    if (ok) {
        const double s = plan.add.chainage, s2 = s + head.shift_m;
        double o1[3], a1[3], u1[3], v1[3], o2[3], a2[3], u2[3], v2[3];
        alignment_frame(A, s, o1, a1, u1, v1);
        alignment_frame(A, s2, o2, a2, u2, v2);
        const double cs = cos(head.roll), sn = sin(head.roll);
        double M[3][3];   // F(s') Q F(s)^T
        for (int r = 0; r < 3; ++r) {
            const double qu = cs * u2[r] + sn * v2[r], qv = cs * v2[r] - sn * u2[r];
            for (int c = 0; c < 3; ++c) M[r][c] = (a2[r] * a1[c] + qu * u1[c]) + qv * v1[c];
        }
        const double rel[3] = {tr[0] - o1[0], tr[1] - o1[1], tr[2] - o1[2]};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) head.pose[4 * r + c] = (M[r][0] * Rm[0][c] + M[r][1] * Rm[1][c]) + M[r][2] * Rm[2][c];
            head.pose[4 * r + 3] = o2[r] + ((M[r][0] * rel[0] + M[r][1] * rel[1]) + M[r][2] * rel[2]);
        }
    }
    memcpy(info, &head, sizeof(head));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_align_info);
    info->element = plan.add.element;
    info->n_sides = plan.add.n_sides;
    info->chainage = plan.add.chainage;
    info->anchor_global = plan.anchor_global;
    info->plan = plan.add;
    return GM_OK;
}

gm_status alignment_window(const Alignment &A, double s_from, double s_to, gm_wall_alignment_piece *pieces, uint32_t capacity,
                           uint32_t *n_out)
{
    if (!n_out || !isfinite(s_from) || !isfinite(s_to) || s_from > s_to || (capacity && !pieces)) return GM_ERR_INVALID_ARG;
    uint32_t got = 0;
    for (uint32_t i = 0; i < (uint32_t)A.el.size(); ++i) {
        const AlignElem &E = A.el[i];
        const double lo = std::max(s_from, E.s_start), hi = std::min(s_to, E.s_end);
        if (!(lo < hi)) continue;
        const double nst = (double)E.p.n_stations;
        const double j0 = std::min(std::max(floor((lo - E.s_start) / A.ds), 0.0), nst);
        const double j1 = std::min(std::max(ceil((hi - E.s_start) / A.ds), 0.0), nst);
        if (!(j0 < j1)) continue;
        if (got < capacity) {
            pieces[got].element = i;
            pieces[got].station0 = (uint32_t)j0;
            pieces[got].n_stations = (uint32_t)(j1 - j0);
            pieces[got].reserved = 0u;
        }
        ++got;
    }
    *n_out = got;
    return got > capacity ? GM_ERR_CAPACITY : GM_OK;
}

// gm_wall_alignment_check_objects' host half (include/gm_hip.h states the rule): the size rule, the plan's sides on the
// global station grid, G_f and the window around it
gm_status alignment_object_window(const Alignment &A, const gm_wall_alignment_add_info &plan, const gm_wall_object_params &op,
                                  ObjectWindow &w, gm_wall_alignment_objects_info *info)
{
    static_assert(sizeof(gm_wall_alignment_objects_info) == 136 && offsetof(gm_wall_alignment_objects_info, element) == sizeof(gm_wall_objects_info),
                  "the shared head");
    if (!info) return GM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_objects_info);
    if (A.el.empty() || !object_prm_ok(op)) return GM_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)A.el.size(), nsec = A.el[0].p.n_sectors;
    uint64_t total = 0;
    for (const AlignElem &E : A.el) total += E.p.n_stations;   // (<= 256 * 2^32)
    const uint64_t NK = (nsec + op.block_sectors - 1u) / op.block_sectors;
    const uint64_t rows_of_blocks = (total + op.block_stations - 1u) / op.block_stations;
    if (total > 0xFFFFFFFFull || rows_of_blocks * NK > 0xFFFFFFFFull) return GM_ERR_UNSUPPORTED;   // (both factors < 2^32)
    if (plan.struct_size != sizeof(gm_wall_alignment_add_info) || plan.n_sides < 1u || plan.n_sides > GM_WALL_JOINT_MAX_SIDES)
        return GM_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < plan.n_sides; ++k)
        if (plan.side_element[k] >= n || (k && plan.side_element[k] != plan.side_element[k - 1u] + 1u)) return GM_ERR_INVALID_ARG;
    if (plan.element < plan.side_element[0] || plan.element > plan.side_element[plan.n_sides - 1u]) return GM_ERR_INVALID_ARG;
    const uint32_t home = plan.element - plan.side_element[0];
    uint64_t base = 0;
    for (uint32_t i = 0; i < plan.side_element[0]; ++i) base += A.el[i].p.n_stations;
    info->element = plan.element;
    info->n_sides = plan.n_sides;
    info->total = (int64_t)total;
    for (uint32_t k = 0; k < plan.n_sides; ++k) {
        info->side_element[k] = plan.side_element[k];
        info->side_first[k] = (uint32_t)base;
        base += A.el[plan.side_element[k]].p.n_stations;
    }
    // G_f in int64: an anchor the add accepts is < 4e18 in size and a base < 2^32; anything else saturates, far outside
    const int64_t bf = (int64_t)info->side_first[home], an = plan.side_anchor[home];
    const int64_t Gf = an > INT64_MAX - bf ? INT64_MAX : bf + an;
    info->anchor_global = Gf;
    if (!object_window(total, nsec, op, Gf, w)) return GM_ERR_INVALID_ARG;
    info->station0 = w.station0;
    info->n_stations = w.n_stations;
    info->blocks_stations = w.nJ;
    info->blocks_sectors = w.NK;
    return GM_OK;
}

// gm_wall_alignment_regions' host half (include/gm_hip.h states the rule): the size rule, the window on the global station
// grid and the elements it meets
gm_status alignment_region_window(const Alignment &A, uint32_t station0, uint32_t n, gm_wall_alignment_regions_info *info)
{
    static_assert(sizeof(gm_wall_alignment_regions_info) == 112 && offsetof(gm_wall_alignment_regions_info, total) == sizeof(gm_wall_regions_info),
                  "the shared head");
    if (!info) return GM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    info->struct_size = (uint32_t)sizeof(gm_wall_alignment_regions_info);
    if (A.el.empty()) return GM_ERR_INVALID_ARG;
    const gm_wall_params &t = A.el[0].p;
    const uint32_t nsec = t.n_sectors;
    uint64_t total = 0;
    for (const AlignElem &E : A.el) total += E.p.n_stations;   // (<= 256 * 2^32)
    if (total * nsec > 0x7FFFFFFFull) return GM_ERR_UNSUPPORTED;   // (nsec <= 4096: no overflow)
    if ((uint64_t)station0 + n > total) return GM_ERR_INVALID_ARG;
    if ((uint64_t)n * nsec > GM_WALL_ALIGNMENT_REGION_MAX_CELLS) return GM_ERR_UNSUPPORTED;
    info->station0 = station0;
    info->n_stations = n;
    info->n_sectors = nsec;
    // (one operation per statement, as gm_wall_region_metrics derives it)
    const double sr = t.station_length * t.radius;
    const double ring = sr * kTwoPi;
    info->cell_area = ring / (double)nsec;
    info->total = (int64_t)total;
    if (!n) return GM_OK;
    const uint64_t last = (uint64_t)station0 + n - 1u;
    uint64_t base = 0;
    for (uint32_t i = 0; i < (uint32_t)A.el.size(); ++i) {
        const uint64_t next = base + A.el[i].p.n_stations;
        if (station0 >= base && station0 < next) {
            info->element_from = i;
            info->station_from = (uint32_t)(station0 - base);
        }
        if (last >= base && last < next) {
            info->element_to = i;
            info->station_to = (uint32_t)(last - base);
        }
        base = next;
    }
    info->n_pieces = info->element_to - info->element_from + 1u;
    return GM_OK;
}

}  // namespace wall
}  // namespace gm

extern "C" {

gm_status gm_wall_alignment_check(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n)
{
    Alignment A;
    return alignment_build(params, elements, n, A);
}

gm_status gm_wall_alignment_element_params(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, uint32_t i,
                                           gm_wall_params *out, gm_wall_arc *arc, gm_wall_clothoid *clothoid)
{
    Alignment A;
    if (!out) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    if (i >= n) return GM_ERR_INVALID_ARG;
    *out = A.el[i].p;
    if (arc) *arc = A.el[i].arc;
    if (clothoid) *clothoid = A.el[i].cl;
    return GM_OK;
}

gm_status gm_wall_alignment_project(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, const double xyz[3],
                                    uint32_t *element, double *chainage, double *angle, double *e)
{
    Alignment A;
    if (!xyz || !element || !chainage || !angle || !e) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    if (!isfinite(xyz[0]) || !isfinite(xyz[1]) || !isfinite(xyz[2])) return GM_ERR_INVALID_ARG;
    alignment_project(A, xyz, *element, *chainage, *angle, *e);
    return GM_OK;
}

gm_status gm_wall_alignment_point(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, double chainage,
                                  double angle, double rho, double xyz[3])
{
    Alignment A;
    if (!xyz || !isfinite(chainage) || !isfinite(angle) || !isfinite(rho)) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    alignment_point(A, chainage, angle, rho, xyz);
    return GM_OK;
}

gm_status gm_wall_alignment_add_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                     const double pose[12], double bound, gm_wall_alignment_add_info *info)
{
    Alignment A;
    GMW_OK(alignment_build(params, elements, n, A));
    return alignment_add_plan(A, pose, bound, info);
}

gm_status gm_wall_alignment_locate_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                        const double pose[12], double bound, gm_wall_alignment_locate_start *start)
{
    Alignment A;
    GMW_OK(alignment_build(params, elements, n, A));
    return alignment_locate_start(A, pose, bound, start);
}

gm_status gm_wall_alignment_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, double s_from,
                                   double s_to, gm_wall_alignment_piece *pieces, uint32_t capacity, uint32_t *n_out)
{
    Alignment A;
    GMW_OK(alignment_build(params, elements, n, A));
    return alignment_window(A, s_from, s_to, pieces, capacity, n_out);
}

gm_status gm_wall_alignment_align_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                       const double pose[12], double bound, const gm_wall_align_params *prm,
                                       gm_wall_alignment_align_plan_info *plan)
{
    Alignment A;
    GMW_OK(alignment_build(params, elements, n, A));
    return alignment_align_plan(A, pose, bound, params_or(prm, gm_wall_align_default_params), plan);
}

gm_status gm_wall_alignment_align_select(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                         const double pose[12], double bound, const gm_wall_align_params *prm,
                                         const gm_wall_align_score *table, uint32_t n_scores, gm_wall_alignment_align_info *info)
{
    Alignment A;
    if (!table || !info) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    const gm_wall_align_params ap = params_or(prm, gm_wall_align_default_params);
    gm_wall_alignment_align_plan_info plan;
    GMW_OK(alignment_align_plan(A, pose, bound, ap, &plan));
    if (n_scores != (2u * ap.max_station_shift + 1u) * (2u * ap.max_sector_shift + 1u)) return GM_ERR_INVALID_ARG;
    return alignment_align_select(A, pose, ap, plan, table, info);
}

gm_status gm_wall_alignment_object_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                          const gm_wall_alignment_add_info *plan, const gm_wall_object_params *prm,
                                          gm_wall_alignment_objects_info *info)
{
    Alignment A;
    if (!plan || !info) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    ObjectWindow w;
    return alignment_object_window(A, *plan, params_or(prm, gm_wall_object_default_params), w, info);
}

gm_status gm_wall_alignment_object_metrics(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                           const gm_wall_object_params *op, const gm_wall_object *o,
                                           struct gm_wall_alignment_object_metrics *out)
{
    static_assert(sizeof(struct gm_wall_alignment_object_metrics) == 112 &&
                      offsetof(struct gm_wall_alignment_object_metrics, element_from) == sizeof(struct gm_wall_object_metrics),
                  "the shared head");
    Alignment A;
    if (!o || !out) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n, A));
    struct gm_wall_object_metrics head;
    GMW_OK(gm_wall_object_metrics(params, op, o, &head));   // (the template's t_min, station_length and n_sectors)
    uint64_t total = 0;
    for (const AlignElem &E : A.el) total += E.p.n_stations;
    if ((uint64_t)o->station_max >= total) return GM_ERR_INVALID_ARG;   // (station_min <= station_max: the head's refusal)
    memset(out, 0, sizeof(*out));
    memcpy(out, &head, sizeof(head));
    uint64_t base = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t next = base + A.el[i].p.n_stations;
        if (o->station_min >= base && o->station_min < next) {
            out->element_from = i;
            out->station_from = (uint32_t)(o->station_min - base);
        }
        if (o->station_max >= base && o->station_max < next) {
            out->element_to = i;
            out->station_to = (uint32_t)(o->station_max - base);
        }
        base = next;
    }
    return GM_OK;
}

gm_status gm_wall_alignment_region_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n_el,
                                          uint32_t station0, uint32_t n, gm_wall_alignment_regions_info *info)
{
    Alignment A;
    if (!info) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n_el, A));
    return alignment_region_window(A, station0, n, info);
}

gm_status gm_wall_alignment_region_metrics(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n_el,
                                           const gm_wall_region *r, struct gm_wall_alignment_region_metrics *out)
{
    static_assert(sizeof(struct gm_wall_alignment_region_metrics) == 120 &&
                      offsetof(struct gm_wall_alignment_region_metrics, element_from) == sizeof(struct gm_wall_region_metrics),
                  "the shared head");
    Alignment A;
    if (!r || !out) return GM_ERR_INVALID_ARG;
    GMW_OK(alignment_build(params, elements, n_el, A));
    struct gm_wall_region_metrics head;
    GMW_OK(gm_wall_region_metrics(params, r, &head));   // (the template's t_min, station_length, radius and n_sectors)
    const uint32_t nsec = params->n_sectors;
    uint64_t total = 0;
    for (const AlignElem &E : A.el) total += E.p.n_stations;
    const uint64_t Gp = r->peak_cell / nsec;
    const uint32_t kp = r->peak_cell % nsec;
    if ((uint64_t)r->station_max >= total || Gp >= total) return GM_ERR_INVALID_ARG;   // (station_min <= station_max: the head's refusal)
    memset(out, 0, sizeof(*out));
    memcpy(out, &head, sizeof(head));
    uint64_t base = 0;
    for (uint32_t i = 0; i < n_el; ++i) {
        const uint64_t next = base + A.el[i].p.n_stations;
        if (r->station_min >= base && r->station_min < next) {
            out->element_from = i;
            out->station_from = (uint32_t)(r->station_min - base);
        }
        if (r->station_max >= base && r->station_max < next) {
            out->element_to = i;
            out->station_to = (uint32_t)(r->station_max - base);
        }
        if (Gp >= base && Gp < next) {
            out->peak_element = i;
            out->peak_station = (uint32_t)(Gp - base);
        }
        base = next;
    }
    out->peak_sector = kp;
    // (one operation per statement: the same roundings as the twin's, whatever the compiler may contract)
    const double gc = (double)Gp + 0.5;
    const double along = gc * params->station_length;
    const double chainage = params->t_min + along;
    const double kc = (double)kp + 0.5;
    const double turn = kTwoPi * kc;
    const double angle = turn / (double)nsec;
    const double peak_m = (double)r->peak * 0x1p-20;
    const double rho = params->radius + peak_m;
    alignment_point(A, chainage, angle, rho, out->peak_point);
    return GM_OK;
}

}  // extern "C"
