// gm_internal.hpp -- host-side context and the launch functions each kernel
// file exports.  Nothing here is visible through the C ABI (include/gm_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/gm_hip.h"
#include "gm_dev_array.hpp"
#include "gm_device.hpp"

namespace gm {

// How x,y,z are pulled out of sensor_msgs/PointCloud2 rows
// (pcl::fromROSMsg, /root/reference src/geometric_mapping.cpp:55).
struct RowLayout {
    const uint8_t *data;
    // When set, the rows start at *data_at instead (a device word): a captured launch chain reads device-resident rows through
    // it, so that a frame handed over at another address replays the same graph (the pointer travels like the point count).
    const uint8_t *const *data_at;
    uint32_t step, ox, oy, oz;
    uint32_t mode;  // 0: 16-byte rows x,y,z at 0/4/8 (one dwordx4 load)  1: 4-byte aligned  2: byte loads
    uint32_t bswap; // PointCloud2.is_bigendian
};

struct SortScratch {
    DevArray<uint32_t> totals;            // [kRsMaxPasses][2048] digit totals of every pass (zero-filled when a frame opens)
    DevArray<uint32_t> rec;               // [pass][tile][digit] records of the passes' chained scans (k_sort.hip), cleared per sort
    size_t rec_words = 0;
    DevArray<uint32_t> ticket;            // ticket word of the passes (0 between launches); [1]: the tile cutter's
};

// passes x bits of the radix sort for a key width (k_sort.hip); the crop counts the digit totals of exactly this plan
struct SortPlan { int passes, bits; };

// One in-flight frame: its stream, staging and device buffers (grow-only).  Every DevArray / HostArray member owns its
// block and frees it with the slot; a plain pointer is an alias into memory owned elsewhere.
struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[GM_N_STAGES + 1] = {};
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;  // around the normals kernel alone
    uint32_t cap = 0;          // point capacity of the buffers below
    size_t raw_cap = 0;        // bytes
    HostArray<uint8_t> h_raw;  // pinned staging for the incoming rows
    DevArray<uint8_t> d_raw;
    DevArray<float4> crop4;   // cropped cloud: x,y,z, bits(input row); behind the NaN-normal compaction, which works in place
                              // (k_frame.hip), the valid cloud: rows [0, n_valid)
    DevArray<uint32_t> keys_a, keys_b, vals_a, vals_b;
    DevArray<float4> spts4;   // cropped cloud in cell-sorted order: x,y,z, bits(cropped index)
    uint32_t *skeys = nullptr; // == whichever of keys_a/keys_b holds the sorted keys
    DevArray<float4> normals4;   // per cropped point: nx,ny,nz,curvature (NaN when <3 neighbours); behind the compaction the
                                 // valid cloud's normals, row for row
    DevArray<int32_t> counts;    // per cropped point neighbour count (GM_CFG_KEEP_COUNTS)
    DevArray<uint2> tiles;
    uint32_t tiles_cap = 0;   // entries of the tile list's last class (every tile of a frame fits)
    uint32_t tile_seg = 0;    // entries of each of its other kTileListClasses - 1 classes
    DevArray<uint2> row_bounds;  // [1024*1024] first / one-past-last sorted position per x-row of the search grid
    DevArray<unsigned long long> blk;  // tile records of the single-pass compactions 
    uint32_t blk_cap = 0;
    uint32_t scan_epoch = 0;            // launches of k_compact on this slot so far (see gm_compact.hpp)
    uint32_t scan_seq = 0;              // index of the next k_compact launch inside the frame being captured
    uint64_t cloud_seq = 0;             // counts the clouds the slot has held: every submit and every stage call takes the next
    uint32_t frames_enqueued = 0;       // host mirror of the device-side frame counter (frame_in[1]) that replayed scans take their epochs from
    // graph replay (GM_CFG_GRAPH): the frame's launch chain is captured once per (sizes, layout, configuration) and replayed
    bool capturing = false;             // the launches being enqueued go into a stream capture
    bool kernel_timed = false;          // ev_k0 / ev_k1 bracket the last frame's k_normals (not in a replayed frame)
    DevArray<uint32_t> frame_in;       // device: [0] = points of the frame, [2..3] = address of device-resident rows, [4] = frames replayed so far (epochs)
    HostArray<uint32_t> h_frame_in;     // pinned: words [0..3] of frame_in (copied by a node of the graph)
    static constexpr int kGraphs = 4;   // cached captures (a caller that rotates a few device buffers keeps them all)
    hipGraphExec_t graph_exec[kGraphs] = {};
    unsigned char graph_key[kGraphs][512] = {};  // everything the captured launches froze
    uint32_t graph_key_len[kGraphs] = {};
    uint64_t graph_used[kGraphs] = {};  // last use (least recently used is replaced)
    uint64_t graph_clock = 0;
    uint32_t graph_captures = 0;        // launch chains captured on this slot so far (gm_debug_graph_captures: tests)
    uint32_t alloc_gen = 0;             // counts the (re)allocations of the slot's device buffers (every reserve is handed this word)
    SortScratch sort;
    DevArray<unsigned long long> tile_rec;   // [cutter blocks + 1][kTileListClasses] records of the tile cutter's chained scan
    size_t tile_rec_words = 0;
    DevArray<uint32_t> seg_start;
    DevArray<float4> vox4;       // voxel centroids: x,y,z,count
    DevArray<VoxCell> vox_table; // dense voxel table (fast path)
    DevArray<int32_t> vox_nn;
    DevArray<double> partials;   // [kScatterBlocks][6]  (gm_get_local_frame on caller-supplied normals)
    DevArray<double> tile_partials;  // [compact_records(cap)][6]  scatter rows left by the NaN-normal compaction
    DevArray<uint8_t> labels;
    DevArray<uint8_t> inl_mask;   // per valid point: which of the last RANSAC stage's hypotheses it is an inlier of
    DevArray<DevCounters> ctr;
    DevArray<VoxelParams> voxp;
    DevArray<FrameOut> d_out;
    HostArray<FrameOut> h_out;    // pinned
    // extension scratch (allocated on first use)
    uint32_t ext_H = 0, ext_cap = 0;
    DevArray<float> hyp_plane, hyp_cyl;   // [H][8]
    DevArray<float2> band;                           // [H]
    DevArray<uint32_t> score_partial;                // [score_blocks][H]
    DevArray<int32_t> cnt_plane, cnt_cyl; // [H]
    DevArray<uint32_t> best_plane, best_cyl; // [2]
    DevArray<double> mom_partial;                    // [kScatterBlocks][16]
    DevArray<double> mom_plane, mom_cyl;  // [16]
    DevArray<unsigned long long> nn_best;            // [cap]
    DevArray<float4> vox_nrm4;                       // [cap] normal of each voxel centroid's nearest point (GM_CFG_NEAREST)
    // cylinder regression (k_cylfit.hip)
    DevArray<double> fit_partial;                    // [kFitBlocks][24] partial rows of a pass
    DevArray<uint32_t> fit_ticket;                   // last-block ticket of the passes (0 between launches)
    DevArray<CylFitWork> fit_work;                   // model between the passes
    DevArray<float> fit_init;                        // [8] gm_fit_cylinder's starting row
    DevArray<gm_cylinder_fit> fit_stage;             // gm_fit_cylinder's result record
    gm_cylinder_fit last_fit = {};                    // the fit of the slot's last completed frame (GM_CFG_CYLINDER_FIT)
    // wall deviation map (k_surface.hip; GM_CFG_SURFACE_MAP or gm_surface_map, allocated on first use)
    DevArray<SurfParams> surf_prm;                   // [2]: the frames' parameters, the stage call's
    DevArray<uint8_t> surf_table;                    // global cell table + class counters + ticket (zero between launches)
    DevArray<gm_surface_cell> surf_cells;            // [GM_SURF_MAX_CELLS]
    DevArray<gm_surface_info> surf_info;
    DevArray<gm_cylinder_fit> surf_fit;              // the stage call's model row
    DevArray<float> surf_res;                        // [surf_cap] per valid point
    DevArray<int32_t> surf_cell;                     // [surf_cap]
    uint32_t surf_cap = 0;
    // /choppedCloud output (gm_set_cloud_output): caller-owned page-locked rows, copied on a stream of their own
    float4 *cloud_out = nullptr;
    float4 *cloud_out_dev = nullptr;   // the same rows as the device sees them (mapped page-locked memory)
    uint32_t cloud_out_cap = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_crop = nullptr, ev_valid = nullptr, ev_copied = nullptr;
    // state
    bool submitted = false, complete = false;
    bool pipelined = false;      // the context keeps several frames in flight (n_slots > 1): kernels choose block shapes that share the chip
    bool vox_sort_path = false;  // this frame's voxels came from the sort path (may report passthrough)
    uint32_t n_in = 0;
    gm_frame_result last = {};
};

// record array + ticket word + a fresh epoch for the next k_compact launch on this slot's stream
inline ScanState next_scan(Slot &sl)
{
    ScanState st;
    st.status = sl.blk;
    if (sl.capturing) {   // (replayed launches derive their epoch on the device)
        st.epoch = sl.scan_seq++ & 31u;
        st.frame_ptr = sl.frame_in + 4;
    } else {
        // 1 .. 2^29-2, never 0.  When the counter wraps, the records are cleared (on the slot's stream, behind every
        // launch that wrote them): a record left at a tile index that no launch of the last 2^29 has reached would
        // otherwise carry the epoch that is about to be reused and read as ready.
        if (sl.scan_epoch >= 0x1FFFFFFEu) {
            (void)hipMemsetAsync(sl.blk, 0, sizeof(unsigned long long) * (size_t)sl.blk_cap, sl.stream);
            if (sl.tile_rec) (void)hipMemsetAsync(sl.tile_rec, 0, sizeof(unsigned long long) * sl.tile_rec_words, sl.stream);
            sl.scan_epoch = 0;
        }
        sl.scan_epoch += 1u;
        st.epoch = sl.scan_epoch;
        st.frame_ptr = nullptr;
    }
    st.ticket = reinterpret_cast<uint32_t *>(sl.blk + sl.blk_cap);
    return st;
}

}  // namespace gm

struct gm_ctx {
    gm_config cfg;
    int device = 0;
    uint32_t n_slots = 1;
    gm::Slot *slots = nullptr;
    double own_lo, own_hi;
    bool force_voxel_sort = false;
    gm_surface_params surf;   // gm_set_surface_params (the frames' map parameters)
    std::vector<gm_wall_map *> walls;   // persistent wall maps created from this context (gm_wall.hip), freed with it
    std::vector<gm_wall_alignment *> alignments;   // wall alignments (gm_wall_alignment.hip): their element maps are in `walls`
    std::string err;
};

namespace gm {

constexpr int kScatterBlocks = 1024;

// ---- launchers (each enqueues on `s`, never synchronises) --------------------

// k_crop.hip
// count_digits: the emit step also counts the digit totals of the cell sort's passes into sl.sort.totals (which the
// caller has zeroed on this stream)
void launch_crop(const RowLayout &rows, uint32_t n, float lo, float hi, const GridParams &g, Slot &sl, hipStream_t s,
                 uint32_t n_size = 0, const uint32_t *n_dev = nullptr, bool count_digits = false);
// k_sort.hip : stable LSD radix sort of (key, index) pairs, one launch per pass; n is device-resident.
// Returns 0 if the sorted keys (and values) end in (keys_a, vals_a), 1 if in (keys_b, vals_b).
size_t radix_totals_bytes();
size_t radix_record_words(uint32_t n_cap, int key_bits);   // record words a sort of n_cap positions uses (cleared before it)
size_t radix_record_words_max(uint32_t n_cap);
SortPlan radix_plan(int key_bits);
int cell_key_bits(const GridParams &g);
int launch_radix_sort(uint32_t *keys_a, uint32_t *vals_a, uint32_t *keys_b, uint32_t *vals_b,
                      const uint32_t *n_ptr, uint32_t n_cap, int key_bits, Slot &sl, bool prepared,
                      hipStream_t s, const float4 *rows_in = nullptr, float4 *rows_out = nullptr);
// k_normals.hip
// scratch_cleared: the frame's opening zero-fill cleared the per-row table AND the crop counted the sort's digit totals
void launch_grid_and_normals(const GridParams &g, const VoxDense &vd, Slot &sl, uint32_t n_cap, bool keep_counts,
                             bool scratch_cleared, hipStream_t s);
// one launch that zero-fills up to four 8-byte-granular regions (the frame's counters and scratch tables)
struct ZeroJobs { void *ptr[6]; uint64_t words8[6]; uint32_t *frame_counter; };   // (+1 on the counter: one frame more)
void launch_zero_fill(const ZeroJobs &jobs, hipStream_t s);
uint32_t max_tiles(uint32_t n_cap, const GridParams &g);
uint32_t tile_cutter_blocks(uint32_t n_cap);   // blocks (= chained-scan records per class) of k_rows_and_tiles
// k_frame.hip
// NaN-normal compaction, in place: crop4 / normals4 [0, n_valid) become the valid cloud and its normals (two launches:
// k_valid_scan, then the move of the rows behind the first dropped point); also leaves the scatter-matrix partial rows of
// the survivors in sl.tile_partials (one per *row_tile cropped points); returns the number of rows launched
uint32_t launch_compact_valid(Slot &sl, uint32_t n_cap, double weightingFactor, hipStream_t s, uint32_t *row_tile = nullptr);
// scatter partials over nrm4[0..n); returns the number of partial rows written
uint32_t launch_scatter_partials(const float4 *nrm4, const uint32_t *n_ptr, uint32_t n_cap, double wf, Slot &sl,
                                 hipStream_t s);
void launch_rows_to_host(const float4 *src, float4 *dst_mapped, const uint32_t *begin_enc, const uint32_t *end_ptr, hipStream_t s);
void launch_frame_finalize(const double *partials, uint32_t n_partials, uint32_t row_tile, Slot &sl, hipStream_t s);
// k_voxel.hip
void launch_voxel_grid(Slot &sl, uint32_t n_cap, float leaf, int key_bits, hipStream_t s);
void launch_voxel_dense_finalize(const VoxDense &vd, Slot &sl, hipStream_t s);
constexpr uint32_t kVoxDenseMaxCells = 1u << 18;
// k_ransac.hip (extensions)
constexpr uint32_t kMaxHypotheses = 8192;
uint32_t score_blocks(uint32_t n_cap);
void launch_plane_hypotheses(const float4 *pts, const uint8_t *labels, uint32_t want, const uint32_t *n_ptr,
                             uint32_t n_host, uint64_t seed, uint32_t H, float *hyp8, int32_t *zero_counts,
                             hipStream_t s);
void launch_cylinder_hypotheses(const float4 *pts, const float4 *nrm, const uint8_t *labels, uint32_t want,
                                const uint32_t *n_ptr, uint32_t n_host, uint64_t seed, uint32_t H, float *hyp8,
                                int32_t *zero_counts, float2 *band, double tau, hipStream_t s);
void launch_score(int model, const float4 *pts, const uint8_t *labels, uint32_t want, const uint32_t *n_ptr,
                  uint32_t n_cap, const float *hyp8, float2 *band, uint32_t H, double tau, uint32_t *partial,
                  int32_t *counts, uint32_t *best, hipStream_t s);
bool launch_score_preemptive(int model, const float4 *pts, const uint8_t *labels, uint32_t want,
                             const uint32_t *n_ptr, uint32_t n_cap, const float *hyp8, float2 *band, uint32_t H,
                             double tau, uint32_t *scratch, int32_t *counts, uint32_t *best, bool prepared,
                             const uint32_t **sel_out, const int32_t **cnt_out, uint32_t *k_out, hipStream_t s,
                             uint8_t *masks = nullptr, bool *masks_written = nullptr, bool *replicated_counts = nullptr);
                             // masks != nullptr: the last stage streams (k_score_stream; its counters are then kept in copies) and may leave inlier masks
uint32_t launch_label(int model, const float4 *pts, uint8_t *labels, uint32_t want, uint32_t label, const uint32_t *n_ptr,
                      uint32_t n_cap, const float *hyp8, const float2 *band, uint32_t *best, double tau, int init,
                      const uint32_t *sel, const int32_t *counts_k, uint32_t K, hipStream_t s,
                      const float4 *nrm = nullptr, double *mom_partial = nullptr,
                      const uint8_t *masks = nullptr, bool replicated_counts = false);  // returns the grid size (= partial rows); masks: of the K hypotheses in sel
void launch_segment_moments(const float4 *pts, const float4 *nrm, const uint8_t *labels, uint32_t label,
                            const uint32_t *n_ptr, uint32_t n_cap, double *partial, double *mom16, hipStream_t s);
void launch_ext_finalize(const float *hyp_plane, const uint32_t *best_plane, const float *hyp_cyl,
                         const uint32_t *best_cyl, double *mom_plane, double *mom_cyl, FrameExt *ext,
                         const double *partial32, uint32_t mom_rows, hipStream_t s,
                         const double *scatter_partials = nullptr, uint32_t scatter_rows = 0, uint32_t row_tile = 0,
                         const DevCounters *ctr = nullptr, const VoxelParams *voxp = nullptr, FrameOut *frame_out = nullptr);
// k_cylfit.hip (cylinder regression, GM_CFG_CYLINDER_FIT): 3 Gauss-Newton passes + 1 label pass on a fixed grid
constexpr uint32_t kFitBlocks = 512;
constexpr int kFitRowLen = 24;   // doubles in a partial row of a pass (22 Gauss-Newton sums or 3 label sums, zero padded)
struct CylFitArgs {
    const float4 *pts;
    const uint8_t *labels;     // eligibility: labels == nullptr, or labels[i] == want or want2
    uint8_t *out;              // mask_mode 0: the label array to rewrite (eligible points: 2 inlier / 0); 1: 0/1 per point
    uint32_t want, want2, mask_mode;
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    const float *init;         // starting row = init + 8 * best[0] (best == nullptr: row 0); point, direction, radius
    const uint32_t *best;
    CylFitWork *work;
    gm_cylinder_fit *fit;      // result record (device)
    double *partial;           // [kFitBlocks][kFitRowLen]
    uint32_t *ticket;
    double tau;
    double *rank_row = nullptr;   // group: the last block writes the rank's reduced 24-double row here instead of solving
};
void launch_cylinder_fit(const CylFitArgs &a, hipStream_t s);
// group (gm_group_fit_cylinder): one pass (0..2 Gauss-Newton, 3 label) with a.rank_row set, then, after the rows of every
// rank are gathered into rows[n_ranks][24] on this rank, the merge that solves / publishes
void launch_cylinder_fit_pass(const CylFitArgs &a, int pass, hipStream_t s);
void launch_cylinder_fit_merge(const CylFitArgs &a, int pass, const double *rows, uint32_t n_ranks, hipStream_t s);
gm_status gm_enqueue_ransac(gm_ctx *ctx, Slot &sl, uint32_t n_cap, uint32_t scatter_rows, uint32_t row_tile);
// k_surface.hip (wall deviation map, GM_CFG_SURFACE_MAP): one launch per frame
struct SurfArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    const gm_cylinder_fit *fit;   // status + fp32 model row
    const SurfParams *prm;
    uint8_t *table;            // Slot::surf_table
    gm_surface_cell *cells;
    gm_surface_info *info;
    float *res;
    int32_t *cell;
};
size_t surface_table_bytes();
// n_cap: the most points the launch can see (the grid is sized by it)
void launch_surface_map(const SurfArgs &a, uint32_t n_cap, hipStream_t s);
SurfParams surface_device_params(const gm_surface_params &p);
gm_status gm_check_surface_params(const gm_surface_params *p);
gm_status gm_ensure_surface(gm_ctx *ctx, Slot &sl);
// k_wall.hip (persistent wall map, gm_wall_*): one launch per add, small kernels for read / merge / clear
constexpr int kWallTotals = 8;   // u64 words behind the cells: mapped, outside, beyond_gate, plane, cells_hit scratch, pad
constexpr uint32_t kWallPointsPerBlock = 8192, kWallMinPointsPerBlock = 2048, kWallSmallBlocks = 48;
struct WallTable {   // SoA over the map's cells
    unsigned long long *sum;
    uint32_t *cnt, *lo, *hi;       // count, ~ordered(min e), ordered(max e)
    unsigned long long *totals;    // [kWallTotals]
};
struct WallArgs {
    const float4 *pts;
    const uint8_t *labels;     // nullptr: no point is plane
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t n_stations, n_sectors;
    int32_t win_first;         // the LDS window: stations [anchor + win_first, anchor + win_first + win_stations)
    uint32_t win_stations;     // win_stations * n_sectors <= GM_SURF_MAX_CELLS
    int64_t anchor;            // j_f
    float o[3], a[3], u[3], v[3];   // the frame-local map frame in sensor coordinates
    float R, station_length, gate, sector_angle, two_pi;
    WallTable table;
    float *res;                // stage call only (nullptr in the frame path)
    int32_t *cell;
};
// the arrays of a table of ncell cells at base: sum i64 | count u32 | lo u32 | hi u32 | totals u64 [kWallTotals]
__host__ __device__ inline WallTable wall_table(uint8_t *base, uint64_t ncell)
{
    WallTable t;
    t.sum = reinterpret_cast<unsigned long long *>(base);
    t.cnt = reinterpret_cast<uint32_t *>(base + 8 * ncell);
    t.lo = t.cnt + ncell;
    t.hi = t.lo + ncell;
    t.totals = reinterpret_cast<unsigned long long *>(base + ((20 * ncell + 7) & ~(uint64_t)7));
    return t;
}
size_t wall_table_bytes(uint64_t ncell);
// The design axis of a launch, host side: the kind (gm_device.hpp: kAxis*) and what the arc and the clothoid kernels take
// beside the arguments (an arc reads ax.arc alone, a straight axis nothing).  One launch front per kernel family takes it
// and launches the instantiation of its kind.
struct WallAxis {
    int kind;
    WallClothoid ax;
};
// n_cap: the most points the launch can see (the grid is sized by it); points_per_block 0: the default rule.  mask (NULL:
// none): k_wall_add over the points whose mask bit is clear; the five point classes also go to ctr[4 .. 8].
void launch_wall_add(const WallArgs &a, const WallAxis &axis, const unsigned long long *mask, unsigned long long *ctr, uint32_t n_cap,
                     uint32_t points_per_block, hipStream_t s);
// k_wall_add_checked.hip (gm_wall_map_add_*_checked): mark the selected rows' points in a bit mask, then k_wall_add's masked
// instantiation.  u64 words of the call's counter block: rows_neg, rows_pos, rows_kept, rows_rejected | skipped, mapped,
// outside, beyond_gate, plane | n_rows, n_points, pad
constexpr int kWallAddCheckedCounters = 12;
struct WallMarkArgs {
    const gm_wall_check_point *rows;
    const unsigned long long *n_rows_ptr;   // the check's counter word (low 32 bits); nullptr: n_rows_host
    uint32_t n_rows_host;
    uint32_t rows_cap;         // rows the buffer holds: the count is clamped to it
    const uint32_t *n_ptr;     // device point count (nullptr: n_host)
    uint32_t n_host;
    uint32_t skip;             // GM_WALL_SKIP_* bits
    long long S;
    uint32_t *mask;            // one bit per point, >= n_points bits rounded up to whole 64-bit words   } zeroed by the caller
    unsigned long long *ctr;   // [kWallAddCheckedCounters]                                              } on the same stream
};
// n_cap: the most rows the launch can see (the grid is sized by it)
void launch_wall_mark(const WallMarkArgs &a, uint32_t n_cap, hipStream_t s);
// the class of one row: 0 selected negative, 1 selected positive, 2 kept, 3 rejected (delta_bits: the row's delta)
__host__ __device__ inline uint32_t wall_mark_class(uint32_t delta_bits, long long dq, uint32_t index, uint32_t n_points,
                                                    uint32_t skip, long long S)
{
    if (dq == 0 || (delta_bits & 0x7F800000u) == 0x7F800000u || index >= n_points) return 3u;
    if (dq < 0) return ((skip & GM_WALL_SKIP_NEG) && -dq >= S) ? 0u : 2u;
    return ((skip & GM_WALL_SKIP_POS) && dq >= S) ? 1u : 2u;
}
void launch_wall_read(const WallTable &T, uint64_t first, uint64_t n, gm_surface_cell *out, hipStream_t s);
void launch_wall_read_raw(const WallTable &T, uint64_t first, uint64_t n, gm_wall_raw_cell *out, hipStream_t s);
void launch_wall_merge_raw(const WallTable &T, uint64_t first, uint64_t n, const gm_wall_raw_cell *in, hipStream_t s);
void launch_wall_clear(const WallTable &T, uint64_t first, uint64_t n, bool totals_too, hipStream_t s);
void launch_wall_count(const WallTable &T, uint64_t n, hipStream_t s);
void gm_wall_free_all(gm_ctx *ctx);   // gm_destroy: the maps still alive
void gm_wall_alignment_free_all(gm_ctx *ctx);   // ... and, ahead of them, the alignments (their maps go with the maps)
// k_wall_regions.hip (gm_wall_map_regions): tiles -> seams -> flatten | reduce -> select | labels
constexpr uint32_t kWallRegionTileCells = 4096;    // the most cells of a tile (its LDS tables)
constexpr int kWallRegionCounters = 8;             // u64: flagged_pos, flagged_neg, unusable, empty, components, regions, pad
struct WallRegionAcc {   // 64 B, zero = empty: minima are kept inverted so that every extent is an integer maximum
    uint32_t cells, label;
    uint32_t st_min_inv, st_max, k_min_inv, k_max, t_min_inv, t_max;
    unsigned long long sum_d, points, peak_key;   // peak_key = min(|d|, 2^32 - 1) << 32 | ~cell
    unsigned long long pad;
};
// one element's share of an alignment's window: window rows [row0, row0 + rows) are stations [station0, station0 + rows) of
// the element map `map` (and of the baseline's map of that element, `base`)
struct WallRegionPiece {
    uint32_t row0, station0, rows, pad;
    WallTable map, base;
};
struct WallRegionArgs {
    WallTable map, base;       // base: the baseline's table when has_base
    uint32_t has_base;
    uint32_t n, nsec;          // the window's stations, the map's sectors
    uint64_t first;            // station0 * nsec: map-wide index of window cell 0
    uint32_t ts, tk, tiles_s, tiles_k;   // the tile and the tiles of the window
    uint32_t conn8, min_count, min_cells;
    long long T;
    uint32_t *parent, *slot;   // [n * nsec] window-local parent (kCcNone, gm_gridcc.hpp: not flagged); a root's region slot
    long long *d;              // [n * nsec] d of the flagged cells
    unsigned long long *ctr;   // [kWallRegionCounters]
    WallRegionAcc *acc;        // [components]
    gm_wall_region *out;       // [components]: the regions, in the order their slots were taken
    uint32_t ncomp;
    // gm_wall_alignment_regions (k_wall_regions_joint.hip): the window's pieces in device memory, ascending and gapless over
    // its rows; n_pieces 0: a map's call (map, base and first are then the map's own).  On an alignment map and base are
    // not read and first = station0 * nsec is the GLOBAL index of window cell 0.
    uint32_t n_pieces;
    const WallRegionPiece *pieces;
};
void launch_wall_region_label(const WallRegionArgs &a, hipStream_t s);    // three launches, up to the component count
void launch_wall_region_reduce(const WallRegionArgs &a, hipStream_t s);   // two launches, up to the region list
void launch_wall_region_labels(const WallRegionArgs &a, uint64_t first, uint64_t n, int32_t *out, hipStream_t s);
// k_wall_regions_joint.hip: the two kernels that read a cell, on the pieces (launch_wall_region_label and _reduce launch
// them in place of the map's when a.n_pieces is not 0)
void launch_wall_region_tiles_joint(const WallRegionArgs &a, hipStream_t s);
void launch_wall_region_reduce_joint(const WallRegionArgs &a, hipStream_t s);
// k_wall_cloud.hip (gm_wall_map_cloud): per chunk of whole block rows merge (unless bs = bk = 1) -> compact + emit
constexpr int kWallCloudCounters = 4;              // u64: empty, below_min_count, the chunk's points (low word), pad
constexpr uint32_t kWallCloudAccBytes = 28;        // merged accumulators per block: sum u64 | count u64 | lo, hi, cells u32
struct WallCloudArgs {
    WallTable map;
    uint64_t first;            // station0 * nsec: map-wide index of window cell 0
    uint32_t station0, n, nsec;
    uint32_t bs, bk, NK;       // the block (clamped to the window and the ring), blocks per block row
    uint32_t merged;           // 0: bs = bk = 1, the table is the source
    uint32_t min_count;
    uint32_t J0, nJ;           // the chunk: block rows [J0, J0 + nJ)
    unsigned long long *acc_sum, *acc_cnt;      // [nJ * NK] merged accumulators of the chunk (zeroed by the caller)
    uint32_t *acc_lo, *acc_hi, *acc_cells;
    const double *dirs;        // [NK][2] cos, sin
    double oa[3], a[3], u[3], v[3];   // o - anchor, and the design frame (fp64, not rounded)
    double R, g, t_min, ds;
    gm_wall_cloud_point *out;  // the chunk's staging
    unsigned long long *ctr;   // [kWallCloudCounters]
};
// the arc position rule beside WallCloudArgs, whose oa, u, v are then not read (a: the design direction at params.point)
struct WallCloudArc {
    const double *rows;        // [nJ][2] cos psi, sin psi of the chunk's block rows (host-computed)
    double ca[3], n[3], b[3];  // C - anchor, n, b
    double inv_kappa, un, ub, vn, vb;
};
// the clothoid position rule beside WallCloudArgs (oa, u, v not read either)
struct WallCloudClothoid {
    const double *rows;        // [nJ][5] (P(tc) - anchor)[3], cos psi, sin psi of the chunk's block rows (host-computed)
    double n[3], b[3];
    double un, ub, vn, vb;
};
// The position rule's axis of a cloud or mesh launch, host side: the kind and the arc's struct, of which a clothoid takes
// rows ([nJ][5] then), n, b and un .. vb, a straight axis nothing.
struct WallCloudAxis {
    int kind;
    WallCloudArc arc;
};
void launch_wall_cloud_merge(const WallCloudArgs &a, hipStream_t s);
void launch_wall_cloud_compact(const WallCloudArgs &a, const WallCloudAxis &axis, const ScanState &st, hipStream_t s);
// k_wall_mesh.hip (gm_wall_map_mesh): the cloud's compaction with an emit step that also stores the survivor's index
// (rank_base + its rank in the chunk) into rank[block of the window] and, for a step cut, its mean into mean[block]; then
// per chunk of whole quad rows one k_compact over the chunk's 2 * quads slots
constexpr int kWallMeshCounters = 6;               // u64: quads_two, quads_one, quads_none, cut_by_step, the chunk's triangles (low word), pad
constexpr uint32_t kWallMeshDead = 0xFFFFFFFFu;    // rank of a block that did not become a point
struct WallMeshArgs {
    const uint32_t *rank;      // [NJ * NK] vertex index per block of the window, kWallMeshDead: not alive
    const float *mean;         // [NJ * NK] the vertex's mean, written for alive blocks only; nullptr: no step cut
    uint32_t NK, NKq;          // blocks and quads per row (NKq = NK: the last column wraps onto the first)
    uint32_t Q0, nq;           // the chunk: quads [Q0, Q0 + nq), whole quad rows
    uint32_t outward;
    float max_step;
    gm_wall_mesh_triangle *out;   // the chunk's staging, 2 * nq records
    unsigned long long *ctr;   // [kWallMeshCounters]
};
void launch_wall_mesh_vertices(const WallCloudArgs &a, const WallCloudAxis &axis, uint32_t *rank, float *mean, uint32_t rank_base,
                               const ScanState &st, hipStream_t s);
void launch_wall_mesh_triangles(const WallMeshArgs &a, const ScanState &st, hipStream_t s);
// k_wall_check.hip (gm_wall_map_check_*): one k_compact launch per check
// u64 words: the seven classes (GM_WALL_CHECK_CLS_* order), peak_pos, -peak_neg, the changed points (low word), n_points, pad
constexpr int kWallCheckCounters = 12;
struct WallCheckArgs {
    WallArgs w;                // the add's arguments (its window fields unused); gate is the check's; res / cell: stage call only
    uint32_t reference, min_count;
    long long T;
    uint32_t row_is_index;     // stage call: row = index (the frame path takes the valid cloud's pad word)
    gm_wall_check_point *out;  // staging, >= n_cap rows
    unsigned long long *ctr;   // [kWallCheckCounters], zeroed by the caller on the same stream
    int32_t *delta;            // stage call only (nullptr in the frame path)
    uint8_t *cls;
};
// n_cap: the most points the launch can see (the grid is sized by it)
void launch_wall_check(const WallCheckArgs &a, const WallAxis &axis, uint32_t n_cap, const ScanState &st, hipStream_t s);
// the rule's integers, shared by the kernel and gm_wall_check_classify
__host__ __device__ inline long long wall_check_fix(float e)   // (int64) rint(e 2^20), saturating at int32, 0 for a NaN
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (long long)__float2int_rn(__fmul_rn(e, 1048576.0f));
#else
    const volatile float p = e * 1048576.0f;
    if (p != p) return 0;
    if (p >= 2147483648.0f) return 2147483647ll;
    if (p <= -2147483648.0f) return -2147483647ll - 1;
    return (long long)__builtin_rintf(p);
#endif
}
// delta and class of a point with residual e (inside the gate) in a cell (sum, count, lo = ~ordered(min), hi = ordered(max))
__host__ __device__ inline uint32_t wall_check_rule(uint32_t reference, uint32_t min_count, long long T, long long sum, uint32_t count,
                                                    uint32_t lo, uint32_t hi, float e, long long &delta)
{
    delta = 0;
    if (count < min_count) return GM_WALL_CHECK_CLS_UNSURVEYED;
    const long long eq = wall_check_fix(e);
    if (reference == GM_WALL_CHECK_ENVELOPE) {
        const long long lq = wall_check_fix(ordered_to_float(~lo)), hq = wall_check_fix(ordered_to_float(hi));
        delta = eq > hq ? eq - hq : (eq < lq ? eq - lq : 0);
    } else {
        const long long q = sum / (long long)count;
        delta = (long long)((unsigned long long)eq - (unsigned long long)q);   // (wraps instead of overflowing on a merged cell of no survey)
    }
    return delta >= T ? GM_WALL_CHECK_CLS_CHANGED_POS : (delta <= -T ? GM_WALL_CHECK_CLS_CHANGED_NEG : GM_WALL_CHECK_CLS_UNCHANGED);
}
// k_wall_locate.hip (gm_wall_map_locate_*): one launch per pass on the cylinder regression's fixed grid
// the state between the passes and the result: written by the last block of each pass, copied to the host behind pass 2
struct WallLocateWork {
    double c[3], d[3], u[3], v[3];   // the state in sensor coordinates, fp64
    double lateral[2], tilt[2];      // the summed steps
    double last_step;                // |x| of the last completed pass
    uint32_t status, passes, n_points, pad;
    gm_wall_locate_pass pass[GM_LOCATE_PASSES];
};
struct WallLocateArgs {
    WallArgs w;                // the add's arguments: its o, a, u, v, gate and window fields unused; res / cell: stage call only
    uint32_t reference, min_count;
    double gate;               // of pass 0
    double c0[3], d0[3], u0[3], v0[3], s0;   // the start, fp64, not rounded
    WallLocateWork *work;
    double *partial;           // [kFitBlocks][kFitRowLen]
    uint32_t *ticket;          // 0 between launches
};
void launch_wall_locate(const WallLocateArgs &a, hipStream_t s);   // the three passes
// k_wall_align.hip (gm_wall_map_align_*): bin -> values -> score
constexpr int kWallAlignCounters = 8;   // u64: plane, beyond_gate, outside_patch, binned, n_points, patch_cells_usable, pad
constexpr int32_t kWallAlignNone = -2147483647 - 1;   // the value of an unusable cell in both int32 images
constexpr int32_t kWallAlignSat = 1 << 30;            // |m| saturates here: far beyond every clamp C <= 2^23
struct WallAlignArgs {
    WallArgs w;                // the add's arguments (its window and table-totals fields unused); gate is the align's
    uint32_t P, A, B;          // half_patch_stations, max_station_shift, max_sector_shift
    uint32_t min_count, min_frame_count;
    uint32_t rows;             // patch rows per block of k_wall_align_score, 1 .. 2P
    long long C;               // the clamp, 1 .. 2^23
    unsigned long long *ctr;   // [kWallAlignCounters]       } one block, zeroed by the caller on the same stream:
    gm_wall_align_score *table;   // [(2A + 1)(2B + 1)]      }   ctr | table | p_sum | p_cnt
    unsigned long long *p_sum; // [2P n_sectors] the patch   }
    uint32_t *p_cnt;           // [2P n_sectors]             }
    int32_t *f;                // [2P n_sectors] the patch's values
    int32_t *m;                // [(2P + 2A) n_sectors] the map's values of stations j_f - P - A ...
};
uint32_t wall_blocks(uint32_t n_cap, uint32_t points_per_block);   // k_wall.hip: the add's grid
// n_cap: the most points the launch can see (the grid is sized by it)
void launch_wall_align_bin(const WallAlignArgs &a, uint32_t n_cap, hipStream_t s);
void launch_wall_align_values(const WallAlignArgs &a, hipStream_t s);   // behind the wait on the adds
void launch_wall_align_score(const WallAlignArgs &a, hipStream_t s);
uint32_t wall_align_default_rows(uint32_t n_sectors);
// k_wall_clearance.hip (gm_wall_map_clearance): stations -> per chunk of whole stations compact + emit
// u64 words 0 .. 5: the six classes (kWallClear* order); 6 stations_tight; 7 stations_infringed; 8 ~key of the least
// clearance (0: none), key = (c + 2^34) << 24 | cell; 9 the chunk's list cells (low word); 10, 11 pad
constexpr int kWallClearCounters = 12;
constexpr uint32_t kWallClearUngauged = 0u, kWallClearEmpty = 1u, kWallClearUnusable = 2u, kWallClearInfringed = 3u,
                   kWallClearTight = 4u, kWallClearClear = 5u;
constexpr long long kWallClearBias = 1ll << 34;   // |c| < 2^34: R_q <= 2^32, |w| <= 2^31, 0 <= G < 2^31
struct WallClearArgs {
    WallTable map;
    uint64_t first;            // station0 * nsec: map-wide index of window cell 0
    uint32_t n, nsec;          // the window's stations, the map's sectors
    uint32_t reference, min_count;
    long long T, Rq;
    const int32_t *gauge;      // [n_gauges][nsec]
    const uint8_t *station_gauge;   // [n], nullptr: table 0
    gm_wall_clearance_station *stations;   // [n]
    unsigned long long *ctr;   // [kWallClearCounters], zeroed by the caller on the same stream
    uint32_t j0, nj;           // the list's chunk: window stations [j0, j0 + nj)
    gm_wall_clearance_cell *out;   // the chunk's staging
};
void launch_wall_clear_stations(const WallClearArgs &a, hipStream_t s);
void launch_wall_clear_list(const WallClearArgs &a, const ScanState &st, hipStream_t s);
// the rule's integers, shared by the kernels and the host
__host__ __device__ inline long long wall_clear_value(uint32_t reference, long long sum, uint32_t count, uint32_t lo)   // count >= 1
{
    if (reference == GM_WALL_CLEAR_MEAN) {
        const long long q = sum / (long long)count;
        return q > kWallAlignSat ? (long long)kWallAlignSat : (q < -kWallAlignSat ? -(long long)kWallAlignSat : q);
    }
    return wall_check_fix(ordered_to_float(~lo));
}
// the class of a usable gauged cell of clearance c
__host__ __device__ inline uint32_t wall_clear_class(long long c, long long T)
{
    return c < 0 ? kWallClearInfringed : (c < T ? kWallClearTight : kWallClearClear);
}
// k_wall_sections.hip (gm_wall_map_sections): one kernel, launched once per fitting pass and once more for the evaluation
constexpr uint32_t kWallSectionCoefs = 9;                   // P <= 1 + 2 GM_WALL_SECTION_MAX_HARMONICS
constexpr long long kWallSectionSat = 1ll << 24;            // |m| and |c_q| end here
constexpr long long kWallSectionBias = 1ll << 29;           // |rho| < 2^29: |m| <= 2^24, |M| <= 9 2^24 + 1
struct WallSectionModel {   // 80 B per section, host -> device before every launch
    long long c[kWallSectionCoefs];   // c_q of the pass before (0 before pass 1)
    long long alive;                  // 0: the section has failed, the launch leaves its record alone
};
struct WallSectionOut {     // 512 B per section, device -> host behind every launch
    gm_wall_section_sums sums;        // over the SELECTED columns (N and r: fitting launches only)
    unsigned long long rss;           // sum rho^2 over the selected columns (meaningful with a threshold <= 2^23)
    long long peak_out, peak_in;      // over the usable columns; 0 without one
    uint32_t peak_out_sector, peak_in_sector;   // 0xFFFFFFFF without one
    uint32_t empty, unusable, usable, pad0;
    unsigned long long pad1[2];
};
struct WallSectionArgs {
    WallTable map, base;       // base: the baseline's table when has_base
    uint32_t has_base;
    uint32_t n, nsec;          // the window's stations, the map's sectors
    uint64_t first;            // station0 * nsec: map-wide index of window cell 0
    uint32_t S, P;             // section_stations, 1 + 2 harmonics
    uint32_t sec0, nsect;      // the chunk: sections [sec0, sec0 + nsect)
    uint32_t min_count, fit;   // fit 1: N and r are summed (a fitting pass); 0: the evaluation
    long long thr;             // selected: usable and |rho| <= thr (pass 1: above every |rho|)
    const int32_t *basis;      // [nsec][P]
    const WallSectionModel *model;   // [nsect]
    WallSectionOut *out;       // [nsect]
};
void launch_wall_sections(const WallSectionArgs &a, hipStream_t s);
// the rule's integers, shared by the kernel and the host
__host__ __device__ inline long long wall_section_value(long long sum, unsigned long long count)   // count >= 1
{
    return sum / (long long)count;
}
__host__ __device__ inline long long wall_section_sat(long long m)
{
    return m > kWallSectionSat ? kWallSectionSat : (m < -kWallSectionSat ? -kWallSectionSat : m);
}
// k_wall_quantities.hip (gm_wall_map_quantities): one kernel per chunk of whole sections
// u64 words 0 .. 5: the six classes (GM_WALL_QUANTITY_CLASS_* order); 6 sections_under; 7 sections_over
constexpr int kWallQuantityCounters = 8;
constexpr int32_t kWallQuantityNoValue = -2147483647 - 1;   // the profile entry of a column that is not usable
struct WallQuantityArgs {
    WallTable map, base;       // base: the baseline's table when has_base
    uint32_t has_base;
    uint32_t n, nsec;          // the window's stations, the map's sectors
    uint64_t first;            // station0 * nsec: map-wide index of window cell 0
    uint32_t station0, S;      // the window's first station, section_stations
    uint32_t sec0, nsect;      // the chunk: sections [sec0, sec0 + nsect)
    uint32_t min_count, n_zones;
    long long Rq;
    const int32_t *lo, *hi;    // [n_profiles][nsec]
    const uint8_t *section_profile;   // [NS], nullptr: table 0
    const uint8_t *zone;       // [nsec], nullptr: zone 0
    gm_wall_quantity *records; // [nsect][n_zones]: the chunk's staging
    int32_t *rows;             // [nsect][nsec] or nullptr
    unsigned long long *ctr;   // [kWallQuantityCounters], zeroed by the caller on the same stream
};
void launch_wall_quantities(const WallQuantityArgs &a, hipStream_t s);
// the rule's integers of one column, shared by the kernel and the host (gm_wall_quantity_column)
struct WallQuantityColumn {
    uint32_t cls;
    bool usable;
    long long v;               // x - b0 of a usable column
    long long line;            // x - L of a usable column
    long long under, over, excess;   // the three area terms
};
__host__ __device__ inline long long wall_quantity_ann(long long a, long long b)   // b >= a >= 0
{
    return ((b - a) * (b + a)) >> 20;
}
__host__ __device__ inline WallQuantityColumn wall_quantity_column(long long Rq, unsigned long long cn, long long sm, bool has_base,
                                                                   unsigned long long bcn, long long bsm, uint32_t min_count,
                                                                   long long lo, long long hi, bool unmeasured)
{
    WallQuantityColumn c;
    c.v = c.line = c.under = c.over = c.excess = 0;
    c.usable = cn >= (unsigned long long)min_count && (!has_base || bcn >= (unsigned long long)min_count);
    const bool empty = cn == 0ull && (!has_base || bcn == 0ull);
    c.cls = unmeasured ? GM_WALL_QUANTITY_CLASS_UNMEASURED : (empty ? GM_WALL_QUANTITY_CLASS_EMPTY : GM_WALL_QUANTITY_CLASS_UNUSABLE);
    if (!c.usable) return c;
    const long long b0 = Rq + (has_base ? wall_section_sat(wall_section_value(bsm, bcn)) : 0ll);
    const long long x = Rq + wall_section_sat(wall_section_value(sm, cn));
    const long long L = b0 + lo, H = b0 + hi;
    c.v = x - b0;
    c.line = x - L;
    if (unmeasured) return c;   // (its value is drawn, its areas are nobody's)
    const long long xc = x < 0 ? 0 : x, Lc = L < 0 ? 0 : L, Hc = H < 0 ? 0 : H;
    const bool under = c.v < lo, over = c.v > hi;
    c.cls = under ? GM_WALL_QUANTITY_CLASS_UNDER : (over ? GM_WALL_QUANTITY_CLASS_OVER : GM_WALL_QUANTITY_CLASS_WITHIN);
    if (under) c.under = wall_quantity_ann(xc, Lc);
    if (c.line > 0) c.over = wall_quantity_ann(Lc, xc);
    if (over) c.excess = wall_quantity_ann(Hc, xc);
    return c;
}
// k_wall_objects.hip (gm_wall_map_check_objects, gm_wall_check_objects): bin -> tiles -> seams -> flatten | blocks ->
// reduce -> select | rows; k_wall_objects_joint.hip (gm_wall_alignment_check_objects): bin, reduce and rows behind the
// alignment's row decode (gm_wall_objects.hpp)
constexpr uint32_t kWallObjectTileBlocks = 4096;      // the most window blocks of a tile (its LDS tables)
// (two index spaces that never meet: kCcNone (gm_gridcc.hpp) is a value of parent[], kWallObjectRejected /
// kWallObjectOutside are values of a row's decoded block index; both are above every real index, 2 NB <= 2^21)
constexpr uint32_t kWallObjectRejected = 0xFFFFFFFFu, kWallObjectOutside = 0xFFFFFFFEu;   // a row without a window block
// u64 words 0 .. 8: rejected, outside_window, sparse, small, in_object, flagged_neg, flagged_pos, components, objects;
// words 9 .. 12: the rows of each side that are not rejected (the joint kernels only; 0 on a map); words 13 .. 15 unused:
// the block is 128 bytes so that its zero-fill and its copy are whole multiples of 16 bytes
constexpr int kWallObjectCounters = 16;
constexpr int kWallObjectSideRows = 9;
// gm_wall_alignment_check_objects: a row's cell is side << 24 | cell; side k's stations start at global station first[k]
// and its map holds cells[k] cells.  n_sides 0: a map's rows (cell is the map's cell), the table is not read.
struct WallObjectSides {
    uint32_t n_sides;
    uint32_t first[4], cells[4];
};
struct WallObjectAcc {   // 128 B, zero = empty: minima are kept inverted so that every extent is an integer maximum
    uint32_t label, blocks;
    uint32_t st_min_inv, st_max, k_min_inv, k_max, t_min_inv, t_max;
    unsigned long long points, peak_key, sum_delta, sum_x, sum_y, sum_z;   // peak_key = min(|dq|, 2^32 - 1) << 32 | ~index
    uint32_t box_min_inv[3], box_max[3], e_min_inv, e_max;                 // ordered() keys
    uint32_t plane, pad0;                                                  // 0 the negative rows', 1 the positive rows'
    unsigned long long pad1;
};
struct WallObjectArgs {
    const gm_wall_check_point *rows;   // device rows, 32-byte aligned
    uint32_t n_rows;
    uint32_t nsec, cells;      // the map's sectors and cells
    uint32_t bs, bk, NK;       // the block, blocks per block row
    uint32_t J0, nJ, NB;       // the window: block rows [J0, J0 + nJ), NB = nJ * NK window blocks
    uint32_t ts, tk, tiles_s, tiles_k;   // the tile (in blocks) and the tiles of the window
    uint32_t conn8, min_block_points, min_points;
    uint32_t *cnt, *parent, *slot;       // [2 NB]: plane p's block w at p * NB + w; parents index the same space
    unsigned long long *ctr;   // [kWallObjectCounters]
    WallObjectAcc *acc;        // [components]
    gm_wall_object *out;       // [components]: the objects, in the order select took them
    uint32_t *out_slot;        // [components]: the slot of each of them
    const int32_t *pos;        // [components]: slot -> position in the sorted list, -1 for a small component
    uint32_t ncomp;
    int32_t *object_of_row;    // [n_rows]
    WallObjectSides sides;     // by value, behind everything the map's kernels read
};
static_assert(GM_WALL_JOINT_MAX_SIDES == 4, "WallObjectSides, counter words 9 .. 12");
void launch_wall_object_label(const WallObjectArgs &a, hipStream_t s);    // four launches, up to the component count
void launch_wall_object_reduce(const WallObjectArgs &a, hipStream_t s);   // three launches, up to the object list
void launch_wall_object_rows(const WallObjectArgs &a, hipStream_t s);     // object_of_row
// the rule's per-row pieces, shared by the kernels and the host
__host__ __device__ inline long long wall_object_fix16(float x)   // (int64) rint(x 2^16), saturating at int32, 0 for a NaN
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (long long)__float2int_rn(__fmul_rn(x, 65536.0f));
#else
    const volatile float p = x * 65536.0f;
    if (p != p) return 0;
    if (p >= 2147483648.0f) return 2147483647ll;
    if (p <= -2147483648.0f) return -2147483647ll - 1;
    return (long long)__builtin_rintf(p);
#endif
}
// xb .. eb: the bits of x, y, z, e; dq = wall_check_fix(delta)
__host__ __device__ inline bool wall_object_rejected(uint32_t xb, uint32_t yb, uint32_t zb, uint32_t eb, int32_t cell, long long dq,
                                                     uint32_t cells)
{
    const uint32_t inf = 0x7F800000u;
    return cell < 0 || (uint32_t)cell >= cells || dq == 0 || (xb & inf) == inf || (yb & inf) == inf || (zb & inf) == inf ||
           (eb & inf) == inf;
}

// k_nearest.hip
void launch_nearest(const float4 *pts, const uint32_t *n_ptr, uint32_t n_cap, const float4 *queries,
                    const uint32_t *nq_ptr, uint32_t nq_cap, unsigned long long *best, int32_t *idx, hipStream_t s,
                    const float4 *attr = nullptr, float4 *attr_out = nullptr);  // attr_out[q] = attr[idx[q]]

// gm_api.hip helpers shared with gm_ext.hip
gm_status gm_fail(gm_ctx *ctx, gm_status st, const char *msg);
VoxDense gm_make_vox_dense(const gm_ctx *ctx, uint32_t n_cap);   // the dense voxel table a frame of this context uses (enabled = 0: sort path)
gm_status gm_ensure_capacity(gm_ctx *ctx, Slot &sl, uint32_t n, size_t raw_bytes, bool need_raw);
gm_status gm_ensure_ext(gm_ctx *ctx, Slot &sl, uint32_t H);
gm_status gm_begin_stage(gm_ctx *ctx, Slot *&sl);
gm_status gm_check_slot(gm_ctx *ctx, uint32_t slot);
gm_status gm_upload_xyz(gm_ctx *ctx, Slot &sl, const float *xyz, uint32_t n, float4 *dst);   // gm_ext.hip: rows of 3 floats through the slot's staging
void launch_minmax(const float4 *pts, const uint32_t *n_ptr, uint32_t n_cap, DevCounters *ctr, hipStream_t s);

}  // namespace gm
