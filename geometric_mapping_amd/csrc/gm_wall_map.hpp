// gm_wall_map.hpp -- what the four wall-map files share: the map, the state of one (map, slot), the pure rules.
//   gm_wall_host.hip  every entry point that needs no device, and the rules the others share with them
//   gm_wall.hip       the map itself and the window calls
//   gm_wall_slot.hip  the per-(map, slot) calls: check, locate, align, objects
//   gm_wall_add_checked.hip  the add less the check's changed rows: a slot's check and the map's add in one call
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gm_internal.hpp"
#ifndef GM_WALL_HOST_ONLY   // (gm_wall_host.hip defines it)
#include "gm_compact.hpp"
#endif

#define GMW_HIP(ctx, call)                                                           \
    do {                                                                             \
        hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) {                                                     \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);         \
            return (e__ == hipErrorOutOfMemory) ? GM_ERR_OOM : GM_ERR_DEVICE;        \
        }                                                                            \
    } while (0)
#define GMW_OK(call)                       \
    do {                                   \
        const gm_status s__ = (call);      \
        if (s__ != GM_OK) return s__;      \
    } while (0)

namespace gm {
namespace wall {

constexpr double kTwoPi = 6.283185307179586476925286766559;

inline double dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// ---- gm_wall_host.hip: no device, no context, no map ----

// the design frame of include/gm_hip.h: k_surface.hip's surf_frame on fp64 inputs, kept in fp64
struct DesignFrame { double o[3], a[3], u[3], v[3], R; uint32_t status; };
void design_frame_of(const gm_wall_params &p, DesignFrame &d);
gm_status check_params(const gm_wall_params *p);
// The arc's own part of a design axis (fp64, not rounded): kappa > 0, the centre C, s0 = point_chainage.
struct ArcFrame { double kappa, inv_kappa, s0, C[3]; };
// The clothoid's own part.  tab: (X, Y) at the n_stations + 1 station starts.
struct ClothoidFrame {
    double k0 = 0.0, rate = 0.0, s0 = 0.0, tau0 = 0.0, ds = 0.0, pt[3] = {};
    uint32_t nst = 0;
    std::vector<double> tab;
    double kappa(double tau) const { return k0 + rate * tau; }
    double psi(double tau) const { return tau * (k0 + (0.5 * rate) * tau); }
};
// DesignAxis::add_frame's result, the per-add frame of include/gm_hip.h: the anchor station, the sensor's and the anchor's
// chainage, the anchor section's origin P in map coordinates; in sensor coordinates (o', a', n', b') rounded to fp32 once
// (u', v' in n, b on a straight axis), the same four and u', v' = Rm^T u(s_f), Rm^T v(s_f) before the rounding, |a'|_1;
// kappa_f, rate and un .. vb rounded to fp32 once (0 on a straight axis).
struct AxisAddFrame {
    int64_t anchor;
    double s, sf, P[3], o64[3], a64[3], u64[3], v64[3], a1;
    float o[3], a[3], n[3], b[3], kappa, rate, un, ub, vn, vb;
};
// The design axis of a map, straight (gm_device.hpp: kAxisStraight), arc or clothoid: the DesignFrame at params.point, the
// curved kinds' n, b and un = u.n, ub = u.b, vn = v.n, vb = v.b there, and the kind's own frame.  Every rule of
// include/gm_hip.h that sees the axis is written here once; where the kinds differ each keeps its own arithmetic,
// operation for operation.  Chainages are the map's own; offset (a straight element of an alignment: alignment chainage =
// map chainage + offset) enters project and point alone.
struct DesignAxis {
    int kind = kAxisStraight;
    DesignFrame d;
    double n[3] = {}, b[3] = {}, un = 0.0, ub = 0.0, vn = 0.0, vb = 0.0, offset = 0.0;
    ArcFrame arc = {};
    ClothoidFrame cl;
    bool is_arc() const { return kind == kAxisArc; }
    bool is_clothoid() const { return kind == kAxisClothoid; }
    // the section at chainage s: a(s), n(s) (u on a straight axis), P(s); returns kappa(s)
    double section(double s, double as[3], double ns[3], double P[3]) const;
    // ... at the start of station j, as an add evaluates its anchor section (a clothoid in tau_0 + j ds: the chainage's
    // size does not enter)
    double station_section(const gm_wall_params &p, double j, double as[3], double ns[3], double P[3]) const;
    // the design frame at s: o = P(s), a(s), u(s), v(s); n(s) to n_out (may be NULL); returns kappa(s)
    double frame(double s, double o[3], double a[3], double u[3], double v[3], double *n_out = nullptr) const;
    // the foot of the perpendicular of a map point: returns its chainage; (yc, zb): the point in the section there, along
    // n(s) and b (u and v on a straight axis)
    double foot(const double x[3], double &yc, double &zb) const;
    void project(const double x[3], double &chainage, double &angle, double &e) const;
    void point(double chainage, double angle, double rho, double xyz[3]) const;
    // the per-add frame of an accepted (Rm, tr); false: the anchor is out of range
    bool add_frame(const gm_wall_params &p, const double Rm[3][3], const double tr[3], AxisAddFrame &out) const;
    // the reach in stations of an add's LDS window under the crop bound B, a1 = |a'|_1
    double reach(const gm_wall_params &p, double B, double a1) const;
    // the position rule's values of a cloud or mesh block row centred at chainage tc, less the anchor: row_width() doubles
    uint32_t row_width() const { return kind == kAxisClothoid ? 5u : (kind == kAxisArc ? 2u : 0u); }
    void row(double tc, const double anchor[3], double *row) const;
};
// The refusals of gm_wall_map_create (arc and cl NULL), _create_arc and _create_clothoid, each kind's own; the axis of an
// accepted call (a clothoid's table included: GM_ERR_OOM).
gm_status axis_check(const gm_wall_params *p, const gm_wall_arc *arc, const gm_wall_clothoid *cl, DesignAxis &ax);
// ---- gm_wall_alignment_host.hip: a wall alignment (include/gm_hip.h: gm_wall_alignment_create), no device either ----
// One element: its derived structs (what its map is created from), its axis (a straight element's offset in it) and its
// chainage span in the alignment.
struct AlignElem {
    gm_wall_params p;
    gm_wall_arc arc;
    gm_wall_clothoid cl;
    DesignAxis ax;
    double s_start = 0.0, s_end = 0.0;
};
struct Alignment {
    std::vector<AlignElem> el;
    double ds = 0.0;
};
// the chaining and every refusal of it; GM_ERR_OOM or GM_ERR_INVALID_ARG
gm_status alignment_build(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, Alignment &A);
uint32_t alignment_owner(const Alignment &A, const double x[3]);
void alignment_project(const Alignment &A, const double x[3], uint32_t &element, double &chainage, double &angle, double &e);
void alignment_point(const Alignment &A, double chainage, double angle, double rho, double xyz[3]);
// the plan of an add: everything of info; GM_ERR_UNSUPPORTED: too many sides
gm_status alignment_add_plan(const Alignment &A, const double pose[12], double bound, gm_wall_alignment_add_info *info);
gm_status alignment_window(const Alignment &A, double s_from, double s_to, gm_wall_alignment_piece *pieces, uint32_t capacity,
                           uint32_t *n_out);
// what a locate on the alignment starts from: the plan, the home section, the state, the attached vectors
gm_status alignment_locate_start(const Alignment &A, const double pose[12], double bound, gm_wall_alignment_locate_start *out);
// gm_wall_alignment_align_*: F(x), the design frame at alignment chainage x on the element the point rule picks; the plan
// of an align (the add's plan, G_f, row0 per side, the pieces; GM_ERR_UNSUPPORTED: too many sides or pieces); the selection
// and the pose from a table
void alignment_frame(const Alignment &A, double x, double o[3], double a[3], double u[3], double v[3]);
gm_status alignment_align_plan(const Alignment &A, const double pose[12], double bound, const gm_wall_align_params &ap,
                               gm_wall_alignment_align_plan_info *out);
gm_status alignment_align_select(const Alignment &A, const double pose[12], const gm_wall_align_params &ap,
                                 const gm_wall_alignment_align_plan_info &plan, const gm_wall_align_score *table,
                                 gm_wall_alignment_align_info *info);
// the library's pose check: 0 the pose is accepted (Rm, tr filled), 1 an entry is not finite, 2 Rm is not a rotation
int pose_split(const double pose[12], double Rm[3][3], double tr[3]);
// the direction table of include/gm_hip.h: NK pairs (one operation per statement, as stated there)
void cloud_directions(uint32_t nsec, uint32_t bk, double *cos_sin);
// gm_wall_clearance_check_params' rule; T and R_q of an accepted call
bool clearance_ok(const gm_wall_params *p, const gm_wall_clearance_params &c, const int32_t *gauge_q, uint32_t n_gauges,
                  const uint8_t *station_gauge, uint32_t n, long long &T, long long &Rq);
// gm_wall_section_check_params' rule; Tr of an accepted block
bool section_prm_ok(const gm_wall_section_params &p, long long &Tr);
// the basis table of include/gm_hip.h: B[nsec][1 + 2 H] (one operation per statement, as stated there)
void section_basis(uint32_t nsec, uint32_t H, int32_t *B);
// the solve of include/gm_hip.h on one record of sums: the status, and c_q[9] (0 unless the status is GM_SECTION_OK)
uint32_t section_solve(const gm_wall_section_sums &s, uint32_t H, uint32_t min_columns, int64_t cq[9]);
// gm_wall_quantity_check_params' rule; R_q of an accepted call
bool quantity_ok(const gm_wall_params *p, const gm_wall_quantity_params &q, const int32_t *lo_q, const int32_t *hi_q,
                 uint32_t n_profiles, const uint8_t *section_profile, uint32_t n, const uint8_t *zone, uint32_t n_zones,
                 long long &Rq);
bool check_prm_ok(const gm_wall_check_params &c, long long &T);
bool locate_prm_ok(const gm_wall_locate_params &p);
bool align_prm_ok(const gm_wall_align_params &p, uint32_t nsec);
bool object_prm_ok(const gm_wall_object_params &p);
// The window of the object rule around the anchor station jf on a grid of n_stations x n_sectors -- a map's own, or an
// alignment's global stations (n_stations = total <= 2^32 - 1).  false: more than GM_WALL_OBJECT_MAX_BLOCKS blocks.
struct ObjectWindow {
    uint32_t J0 = 0, nJ = 0, NK = 0;         // block rows [J0, J0 + nJ) (nJ 0: empty), blocks per block row
    uint32_t station0 = 0, n_stations = 0;   // the block rows' stations, clipped to the grid
};
bool object_window(uint64_t n_stations, uint32_t n_sectors, const gm_wall_object_params &op, int64_t jf, ObjectWindow &w);
// gm_wall_alignment_check_objects: the plan's sides on the global station grid.  Refusals in their order: GM_ERR_UNSUPPORTED
// (total or the block count beyond 32 bits), GM_ERR_INVALID_ARG (the plan's sides, its element, a window above
// GM_WALL_OBJECT_MAX_BLOCKS blocks).  info: struct_size, the window fields, element, n_sides, anchor_global, total,
// side_element, side_first; everything else 0.
gm_status alignment_object_window(const Alignment &A, const gm_wall_alignment_add_info &plan, const gm_wall_object_params &op,
                                  ObjectWindow &w, gm_wall_alignment_objects_info *info);
// gm_wall_alignment_regions: the window [station0, station0 + n) on the global station grid.  Refusals in their order:
// GM_ERR_UNSUPPORTED (total n_sectors beyond 2^31 - 1), GM_ERR_INVALID_ARG (a window outside [0, total]), GM_ERR_UNSUPPORTED
// (more than GM_WALL_ALIGNMENT_REGION_MAX_CELLS cells).  info: struct_size, the window fields, cell_area, total, n_pieces
// and the element and station fields; everything else 0.  The pieces are the consecutive elements element_from ..
// element_to, whole but for the first station of the first and the last of the last.
gm_status alignment_region_window(const Alignment &A, uint32_t station0, uint32_t n, gm_wall_alignment_regions_info *info);
bool add_checked_prm_ok(const gm_wall_add_checked_params &p, long long &S);   // S of an accepted block
// The selection half of the align rule of include/gm_hip.h from a table of (2A + 1)(2B + 1) records on a grid of station
// length ds and nsec sectors: everything of info but the device's counts, anchor_station and the pose (NaN when it returns
// false: GM_ALIGN_NO_OVERLAP; zero otherwise).
bool align_select_table(const gm_wall_align_params &ap, double ds, uint32_t nsec, const gm_wall_align_score *t, gm_wall_align_info *info);
// The selection and the pose of include/gm_hip.h from a table of (2A + 1)(2B + 1) records.  Fills everything but the
// device's counts.
void align_select(const DesignFrame &d, const gm_wall_params &wp, const gm_wall_align_params &ap, const double Rm[3][3],
                  const double tr[3], const gm_wall_align_score *t, gm_wall_align_info *info);

// the mesh rule of include/gm_hip.h: its two scalar parameters, and the quad grid over NJ x NK blocks
inline bool mesh_rule_ok(uint32_t flags, double max_step)
{
    return !(flags & ~(uint32_t)(GM_WALL_MESH_OUTWARD | GM_WALL_MESH_NO_WRAP)) && isfinite(max_step) && max_step >= 0.0;
}
struct MeshGrid { uint32_t wrapped, NKq; uint64_t quads; };
inline MeshGrid mesh_grid(uint32_t NJ, uint32_t NK, uint32_t flags)
{
    MeshGrid g;
    g.wrapped = (NK >= 3u && !(flags & GM_WALL_MESH_NO_WRAP)) ? 1u : 0u;
    g.NKq = g.wrapped ? NK : (NK ? NK - 1u : 0u);
    g.quads = NJ ? (uint64_t)(NJ - 1u) * g.NKq : 0u;
    return g;
}

// the caller's parameters, or the defaults for NULL
template <class P>
P params_or(const P *prm, void (*defaults)(P *))
{
    P p;
    defaults(&p);
    if (prm) p = *prm;
    return p;
}

// ---- the map: from here to the end not for gm_wall_host.hip, which so sees nothing that calls the device ----
#ifndef GM_WALL_HOST_ONLY

constexpr uint64_t kStageCells = 1u << 20;   // cells per chunk of a window call (24 MiB of raw records)
constexpr uint32_t kSectionChunk = 1u << 16; // sections per chunk of gm_wall_map_sections (37 MiB of scratch)
constexpr uint64_t kStageBytes = kStageCells * 24u;   // the staging of a chunk of gm_wall_map_quantities: what the other window calls use

// The records of a chained scan (gm_compact.hpp) that is not a frame's -- a slot's own belong to the frame that may be in
// flight on it: the record array with the ticket word behind it, and the epoch of the launches on it so far.  The rule is
// next_scan's (gm_internal.hpp): epochs run 1 .. 2^29-2 and never 0, and the records are cleared when the counter wraps,
// behind every launch that wrote them.
struct ScanRecords {
    DevArray<unsigned long long> rec;   // [n] tile records | the ticket word
    uint32_t n = 0;
    uint32_t epoch = 0;
    bool holds(uint32_t points) const { return n >= compact_records(points); }
    // for launches over up to `points` inputs; a new block is zeroed on s.  Nothing may be in flight on the old one.
    gm_status reserve(gm_ctx *ctx, uint32_t points, hipStream_t s)
    {
        if (holds(points)) return GM_OK;
        n = 0;
        const uint32_t want = compact_records(points);
        GMW_HIP(ctx, rec.reserve((uint64_t)want + 1));
        GMW_HIP(ctx, hipMemsetAsync(rec.p, 0, sizeof(unsigned long long) * ((size_t)want + 1), s));
        n = want;
        return GM_OK;
    }
    // the state of the next k_compact launch on s
    ScanState next(hipStream_t s)
    {
        if (epoch >= 0x1FFFFFFEu) {
            (void)hipMemsetAsync(rec.p, 0, sizeof(unsigned long long) * ((size_t)n + 1), s);
            epoch = 0;
        }
        epoch += 1u;
        ScanState st;
        st.status = rec.p;
        st.ticket = reinterpret_cast<uint32_t *>(rec.p + n);
        st.epoch = epoch;
        st.frame_ptr = nullptr;
        return st;
    }
};

// The result of one per-slot call (a check, a locate, an align) of one (map, slot): enqueued on the slot's stream, read by
// the host later.  Every reader of the result, every add on another slot and the map's sync and release go through here.
struct PendingResult {
    hipEvent_t done = nullptr;   // recorded behind the call and the copy of its result
    bool have = false;           // a call was enqueued: a result is (or will be) readable
    bool outstanding = false;    // the host has not waited for `done` yet
    gm_status ensure(gm_ctx *ctx)
    {
        if (!done) GMW_HIP(ctx, hipEventCreateWithFlags(&done, hipEventDisableTiming));
        return GM_OK;
    }
    hipError_t done_passed() { return outstanding ? hipEventSynchronize(done) : hipSuccess; }   // the one host block on `done`
    gm_status wait(gm_ctx *ctx)
    {
        GMW_HIP(ctx, done_passed());
        outstanding = false;
        return GM_OK;
    }
    gm_status record(gm_ctx *ctx, hipStream_t s)
    {
        GMW_HIP(ctx, hipEventRecord(done, s));
        have = outstanding = true;
        return GM_OK;
    }
    // the map is going: nothing may still be writing its blocks (an error has nowhere to go, as at any release)
    void release() { (void)done_passed(); if (done) (void)hipEventDestroy(done); }
};

// gm_wall_map_check_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallCheckSlot {
    DevArray<gm_wall_check_point> stage;    // the changed rows of the last check, in order
    ScanRecords scan;                       // the check's own chained scan
    DevArray<unsigned long long> ctr;       // device [kWallCheckCounters]
    HostArray<unsigned long long> h_ctr;    // pinned copy, valid once the result has been waited for
    PendingResult res;
    uint32_t status = 0;
    long long T = 0;
    int64_t anchor = 0;                     // the check's j_f (gm_wall_map_check_objects anchors its window on it)
    uint64_t cloud_seq = 0;                 // the slot's cloud_seq at the enqueue: the cloud whose indices the rows carry
};

// gm_wall_map_add_frame_checked: the state of one (map, slot), allocated on first use, freed with the map
struct WallAddCheckedSlot {
    DevArray<unsigned long long> blk;       // device [kWallAddCheckedCounters] | the mask: one bit per point of the slot's
                                            // frame in whole 64-bit words (one block: one fill zeroes both per call)
    HostArray<unsigned long long> h_ctr;    // pinned copy, valid once the result has been waited for
    PendingResult res;                      // (also what check_prepare waits for before it frees the rows the mark reads)
    uint32_t status = 0;
    long long S = 0;
};

// gm_wall_map_locate_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallLocateSlot {
    DevArray<WallLocateWork> work;          // the state between the passes, the result behind them
    DevArray<double> partial;               // [kFitBlocks][kFitRowLen] partial rows of a pass
    DevArray<uint32_t> ticket;              // last-block ticket of the passes (0 between launches)
    HostArray<WallLocateWork> h_work;       // pinned copy, valid once the result has been waited for
    PendingResult res;
    int64_t anchor = 0;                     // the locate's j_f
    double of[3] = {0.0, 0.0, 0.0};         // its o_f, map coordinates
};

// gm_wall_map_align_*: the state of one (map, slot), allocated on first use, freed with the map
struct WallAlignSlot {
    DevArray<uint8_t> zeroed;               // counters | score table | patch sums | patch counts: one zero-fill per align
    DevArray<int32_t> f, m;                 // the two value images
    HostArray<uint8_t> h_res;               // pinned copy of counters | score table, valid once the result has been waited for
    PendingResult res;
    gm_wall_align_params prm;               // of that align
    double pose[12];                        // the caller's pose of that align
    uint32_t n_shifts = 0;                  // (2A + 1)(2B + 1)
};

// The per-point outputs of a stage call, device side: the one owner of their buffers (a map's, an alignment's) and the one
// path a call's wanted ones take -- reserved ahead of the launch, handed to the kernel, copied back behind it.
enum : uint32_t { kPtRes = 1u, kPtCell = 2u, kPtDelta = 4u, kPtCls = 8u, kPtElement = 16u };
struct PointOutputs {
    DevArray<float> res;
    DevArray<int32_t> cell, delta, element;
    DevArray<uint8_t> cls;
    uint32_t wanted = 0;   // kPt* bits of the call in progress: the outputs its kernel writes
    // n points of every output in `hold` (which includes `want`); the kernel is to write those in `want`
    gm_status reserve(gm_ctx *ctx, uint64_t n, uint32_t want, uint32_t hold);
    // the kernel's pointers: nullptr for an output that is not wanted
    float *dev_res() const { return (wanted & kPtRes) ? res.p : nullptr; }
    int32_t *dev_cell() const { return (wanted & kPtCell) ? cell.p : nullptr; }
    int32_t *dev_delta() const { return (wanted & kPtDelta) ? delta.p : nullptr; }
    uint8_t *dev_cls() const { return (wanted & kPtCls) ? cls.p : nullptr; }
    int32_t *dev_element() const { return (wanted & kPtElement) ? element.p : nullptr; }
    // n points of each output the caller gave a pointer for, onto `s` behind the launch
    gm_status copy_back(gm_ctx *ctx, hipStream_t s, uint32_t n, float *h_res, int32_t *h_cell, int32_t *h_delta, uint8_t *h_cls,
                        int32_t *h_element) const;
};

// gm_wall_map_check_objects / gm_wall_check_objects and gm_wall_alignment_check_objects / _rows: the tile in blocks
// (GM_WALL_OBJECT_TILE: tests, measurements) and the scratch of their owner, a map or an alignment; allocated on first use
struct ObjectScratch {
    uint32_t tr = GM_WALL_OBJECT_TILE_ROWS, tc = GM_WALL_OBJECT_TILE_COLS;
    DevArray<uint32_t> blocks;               // per window block and plane: cnt | parent | slot
    DevArray<unsigned long long> ctr;        // [kWallObjectCounters]
    DevArray<uint8_t> recs;                  // per component: WallObjectAcc | gm_wall_object | out_slot u32 | pos i32
    DevArray<gm_wall_check_point> rows;      // the stage call's rows
    DevArray<int32_t> of_row;                // object_of_row
    std::vector<gm_wall_object> host;        // the unsorted list, its slots, the sorting permutation, slot -> position
    std::vector<uint32_t> host_slot, order;
    std::vector<int32_t> pos;
    void read_tile_env();                    // GM_WALL_OBJECT_TILE=<block rows>x<block columns>; anything else: the default
};
// The grid a call's rows are decoded on: a map's (sides.n_sides 0) or an alignment's sides on its global stations.
struct ObjectGrid {
    uint32_t nsec = 0, cells = 0;
    WallObjectSides sides = {};
};
// The object call on n_rows device rows (32-byte aligned), on stream `s`, blocking.  rejected_if_empty and
// side_rows_if_empty (may be NULL): the rejected rows and each side's rows that are not, used when nothing is launched
// (zero rows or an empty window).  info: the fields gm_wall_objects_info and gm_wall_alignment_objects_info share, from
// n_rows on (struct_size and what lies behind `reserved` are the caller's); side_rows (may be NULL): counter words
// 9 .. 12.  objects / object_of_row may be NULL; the capacities were checked by the caller but for the record count.
gm_status objects_run(gm_ctx *ctx, hipStream_t s, ObjectScratch &ob, const ObjectGrid &grid, const gm_wall_check_point *d_rows,
                      uint32_t n_rows, uint32_t rejected_if_empty, const uint32_t *side_rows_if_empty, const gm_wall_object_params &op,
                      const ObjectWindow &win, gm_wall_objects_info *info, uint32_t *side_rows, gm_wall_object *objects,
                      uint32_t capacity, uint32_t *n_out, int32_t *object_of_row, const char *who);

// gm_wall_map_regions and gm_wall_alignment_regions: the tile (GM_WALL_REGION_TILE: tests, measurements) and the scratch of
// their owner, a map or an alignment; allocated on first use
struct RegionScratch {
    uint32_t ts = GM_WALL_REGION_TILE_STATIONS, tk = GM_WALL_REGION_TILE_SECTORS;
    DevArray<uint8_t> cells;                 // per window cell: d i64 | parent u32 | slot u32
    DevArray<unsigned long long> ctr;        // [kWallRegionCounters]
    DevArray<uint8_t> recs;                  // per component: WallRegionAcc | gm_wall_region
    DevArray<WallRegionPiece> pieces;        // an alignment's call: the window's pieces
};
// The region call on a window of a.n stations (>= 1), on stream `s`, blocking.  a: the window, the grid, the parameters
// and what the cells are read from (the map's tables, or an alignment's pieces, already on the device); the tile, the
// scratch and the counts are filled in here.  stage: device room for stage_labels labels, a chunk of cell_labels.  info:
// the fields gm_wall_regions_info and gm_wall_alignment_regions_info share; the classes, components and regions are
// written, the rest is the caller's.  regions / cell_labels may be NULL; `who`: the failure of a list that does not fit.
gm_status regions_run(gm_ctx *ctx, hipStream_t s, RegionScratch &rg, WallRegionArgs &a, int32_t *stage, uint64_t stage_labels,
                      gm_wall_regions_info *info, gm_wall_region *regions, uint32_t capacity, uint32_t *n_out, int32_t *cell_labels,
                      const char *who);
// gm_wall_map_regions' parameter rule: NULL and T of an accepted block, or why it is refused (to follow the call's name)
const char *region_prm_refusal(const gm_wall_region_params &p, long long &T);

}  // namespace wall
}  // namespace gm

struct gm_wall_map {
    gm_ctx *ctx = nullptr;
    gm_wall_params prm;
    uint64_t ncell = 0;
    gm::DevArray<uint8_t> base;    // the device table (zeroed at creation)
    gm::WallTable table;
    gm::wall::DesignAxis axis;     // fp64, not rounded
    gm_wall_arc arc;               // gm_wall_map_create_arc's (zero on a straight map)
    gm_wall_clothoid clothoid;     // gm_wall_map_create_clothoid's (zero on other maps)
    uint64_t frames = 0;
    hipStream_t stream = nullptr;  // the small kernels (read / merge / clear / count) and their copies
    std::vector<uint8_t> pending;  // per slot of ctx: an add was enqueued on its stream since the last sync
    std::vector<hipEvent_t> adds;  // per slot of ctx: recorded on its stream for a reader on another slot: the adds so far
    gm::DevArray<uint8_t> stage;   // device staging of the window calls, kStageCells records
    gm::wall::PointOutputs pt;     // the stage calls' per-point outputs: gm_wall_map_add_points', gm_wall_map_check_points'
    uint32_t points_per_block = 0; // 0: the kernel's default (GM_WALL_POINTS_PER_BLOCK: measurements)
    // gm_wall_map_regions: the tile (read at the create) and the scratch
    gm::wall::RegionScratch rg;
    // gm_wall_map_cloud: the chunk (GM_WALL_CLOUD_CHUNK: tests, measurements; 0: kStageCells blocks) and the scratch
    uint32_t cloud_chunk = 0;
    gm::DevArray<uint8_t> cl_acc;      // merged accumulators of a chunk, kWallCloudAccBytes per block (a merging call only)
    gm::DevArray<gm_wall_cloud_point> cl_stage;   // a chunk's records
    gm::wall::ScanRecords cl_scan;     // the map's own chained scan
    gm::DevArray<unsigned long long> cl_ctr;      // [kWallCloudCounters]
    gm::DevArray<double> cl_dirs;      // [GM_WALL_MAX_SECTORS][2]
    std::vector<double> cl_dirs_host;          // the table of the call in progress
    gm::DevArray<double> cl_rows;      // an arc map: [block rows of a chunk][2] cos psi, sin psi; a clothoid map: [..][5]
    std::vector<double> cl_rows_host;
    // gm_wall_map_mesh: its vertex pass runs on the cloud's scratch above; its own
    gm::DevArray<uint32_t> ms_rank;    // [NJ * NK] of the window: a block's vertex index, kWallMeshDead otherwise
    gm::DevArray<float> ms_mean;       // [NJ * NK]: the vertices' means (a call with a step cut only)
    gm::DevArray<gm_wall_mesh_triangle> ms_stage;   // a chunk's triangles
    gm::wall::ScanRecords ms_scan;     // the triangle pass's own chained scan
    gm::DevArray<unsigned long long> ms_ctr;      // [kWallMeshCounters]
    // gm_wall_map_clearance: the chunk (GM_WALL_CLEAR_CHUNK: tests, measurements; 0: kStageCells cells) and the scratch
    uint32_t clear_chunk = 0;
    gm::DevArray<int32_t> cr_gauge;    // the uploaded tables [n_gauges][n_sectors]
    gm::DevArray<uint8_t> cr_station_gauge;        // [n]
    gm::DevArray<gm_wall_clearance_station> cr_stations;   // [n]
    gm::DevArray<gm_wall_clearance_cell> cr_stage; // a chunk's list rows
    gm::wall::ScanRecords cr_scan;     // the list's own chained scan
    gm::DevArray<unsigned long long> cr_ctr;       // [kWallClearCounters]
    // gm_wall_map_sections: the chunk (GM_WALL_SECTION_CHUNK: tests; 0: kSectionChunk sections) and the scratch
    uint32_t section_chunk = 0;
    gm::DevArray<int32_t> sc_basis;    // the uploaded table [n_sectors][P]
    gm::DevArray<uint8_t> sc_chunk;    // per section of a chunk: WallSectionModel | WallSectionOut
    std::vector<int32_t> sc_basis_host;            // the tables of the call in progress
    std::vector<gm::WallSectionModel> sc_model_host;
    std::vector<gm::WallSectionOut> sc_out_host;
    // gm_wall_map_quantities: the chunk (GM_WALL_QUANTITY_CHUNK: tests, measurements; 0: what kStageBytes holds) and the scratch
    uint32_t quantity_chunk = 0;
    gm::DevArray<int32_t> qt_lines;    // the uploaded tables lo [n_profiles][n_sectors] | hi [n_profiles][n_sectors]
    gm::DevArray<uint8_t> qt_index;    // section_profile [NS] | zone [n_sectors]
    gm::DevArray<uint8_t> qt_stage;    // a chunk's records [cs][n_zones] | its profile rows [cs][n_sectors]
    gm::DevArray<unsigned long long> qt_ctr;       // [kWallQuantityCounters]
    // gm_wall_map_check_*, _locate_*, _align_*: per slot of ctx
    std::vector<gm::wall::WallCheckSlot> checks;
    std::vector<gm::wall::WallLocateSlot> locates;
    std::vector<gm::wall::WallAlignSlot> aligns;
    // gm_wall_alignment_locate_*: the pending locates, per slot, of the alignment this map is an element of (they read the
    // map as its own locates do); nullptr on any other map
    std::vector<gm::wall::PendingResult> *al_locates = nullptr;
    // gm_wall_alignment_check_*: the same for that alignment's pending checks
    std::vector<gm::wall::PendingResult> *al_checks = nullptr;
    // gm_wall_alignment_align_*: the same for that alignment's pending aligns
    std::vector<gm::wall::PendingResult> *al_aligns = nullptr;
    // gm_wall_map_add_frame_checked: per slot of ctx; gm_wall_map_add_points_checked: the stage call's own rows and block
    std::vector<gm::wall::WallAddCheckedSlot> add_checks;
    gm::DevArray<gm_wall_check_point> ac_rows;
    gm::DevArray<unsigned long long> ac_blk;
    uint32_t align_rows = 0;  // the patch rows per score block (GM_WALL_ALIGN_ROWS: tests, measurements; 0: the default rule)
    // gm_wall_map_check_objects / gm_wall_check_objects
    gm::wall::ObjectScratch ob;
};

// ---- gm_wall.hip: what the per-slot calls share with the map's own ----

namespace gm {
namespace wall {

inline gm_status set_device(gm_ctx *ctx)
{
    return hipSetDevice(ctx->device) == hipSuccess ? GM_OK : gm_fail(ctx, GM_ERR_DEVICE, "hipSetDevice failed");
}

// The head of a frame call `who`, its refusals in their order: NULL map or context, a foreign context, the slot's range,
// the call's own parameters (prm_ok: run once the three before it hold), a slot without a frame.
template <class PrmOk>
gm_status frame_call_head(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const char *who, PrmOk prm_ok, Slot *&sl)
{
    if (!map || !ctx) return GM_ERR_INVALID_ARG;
    auto refuse = [&](gm_status st, const char *why) { return gm_fail(ctx, st, (std::string(who) + why).c_str()); };
    if (ctx != map->ctx) return refuse(GM_ERR_INVALID_ARG, ": the map belongs to another context");
    if (slot >= ctx->n_slots) return gm_fail(ctx, GM_ERR_INVALID_ARG, "slot out of range");
    if (!prm_ok()) return refuse(GM_ERR_INVALID_ARG, ": struct_size mismatch or a parameter outside its limits");
    sl = &ctx->slots[slot];
    return sl->submitted ? GM_OK : refuse(GM_ERR_NOT_READY, ": the slot holds no frame");
}

// the point fields of a frame call's launch: the frame the slot holds
inline void frame_points(const gm_ctx *ctx, const Slot &sl, WallArgs &w)
{
    w.pts = sl.crop4;
    w.labels = (ctx->cfg.flags & GM_CFG_RANSAC_PLANE) ? sl.labels : nullptr;   // (label 1 exists with the plane RANSAC only)
    w.n_ptr = &sl.ctr->n_valid;
    w.n_host = sl.n_in;
}

// The per-add frame: pose check, anchor, (o', a', u', v') in sensor coordinates, and the kernel's arguments but for the
// buffers.  The context's crop bound (a cube around the sensor) sizes the LDS window.
// f64 (a locate's start): the same vectors before the rounding, and o_f in map coordinates.
struct WallFrame64 { double c[3], d[3], u[3], v[3], of[3]; };
// ax: the map's kind and what the arc and the clothoid kernels take beside w (gm_internal.hpp: WallAxis).  An arc or a
// clothoid map refuses a caller without one (a locate, an align) with GM_ERR_UNSUPPORTED.
gm_status add_frame_args(gm_wall_map *m, const double pose[12], gm_wall_add_info *info, WallArgs &w, WallFrame64 *f64 = nullptr,
                         WallAxis *ax = nullptr);
// An add on `s` (the stream of `slot`) must not be seen by a reader -- a check, a locate, an align -- enqueued before it
// on another slot: `s` waits for every result outstanding there (nothing to wait for on a map without readers).
gm_status add_wait_readers(gm_wall_map *m, uint32_t slot, hipStream_t s);
// The other way round, for a reader on `s` (the stream of `slot`): it waits for the adds enqueued so far on every other
// slot's stream -- an event, no host block.
gm_status wait_adds(gm_wall_map *m, uint32_t slot, hipStream_t s);

// gm_wall_add_checked.hip, shared with the alignment's checked add: the 64-bit words of a call's block -- the counters, then
// one mask bit per point of n_cap (the masked add loads one word per wave and trip) -- and the info of a block's counters
uint64_t add_checked_block_words(uint32_t n_cap);
void add_checked_fill_info(gm_wall_add_checked_info *info, uint32_t status, long long S, const unsigned long long *h);

// A stage call's points (gm_wall_map_add_points, gm_wall_map_check_points, gm_wall_alignment_add_points, ...) on the staging
// slot: open, whatever the call enqueues ahead of its points, upload, the call's launch, close.
struct StageCall {
    gm_wall_map *map;
    uint32_t n;
    PointOutputs &out;   // where the per-point outputs are staged: the map's owner, or that of the alignment map is side 0 of
    float *residual;     // the caller's per-point outputs (NULL: not wanted)
    int32_t *cell, *delta;
    uint8_t *cls;
    int32_t *element;
    Slot *sl = nullptr;
    gm_status open();    // the slot, its capacity and the device side of the per-point outputs; nothing is enqueued
    gm_status upload(const float *xyz, const uint8_t *labels, WallArgs &w);   // points and labels onto the slot's stream; w: the point fields of the launch
    gm_status close();   // the per-point outputs back, behind the launch; blocks until the slot's stream has drained
};

#endif  // GM_WALL_HOST_ONLY
}  // namespace wall
}  // namespace gm
