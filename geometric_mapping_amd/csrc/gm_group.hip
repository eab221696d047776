// gm_group.hip -- one host thread driving every local GPU: spatial sharding of ONE frame across the devices of a node
// with an in-library RCCL all-gather of the fitted records, and round-robin streaming of whole frames over the same
// devices (SURVEY.md par. 8b "Threading", par. 8e; north_star: "Frames shard spatially across the 8 GPUs of one node
// with an RCCL all-gather of fitted primitives over xGMI only when a scan exceeds single-GPU capacity"; BASELINE
// configs[3] and configs[4]).
//
// Replaces the single-threaded ros::spin() consumer of /root/reference src/geometric_mapping.cpp:146,169; the reference
// has no counterpart (no parallelism of any kind, SURVEY.md par. 2).
//
// Sharded frame.  The path shards because every per-point stage depends only on points within neighborRadius and the
// final fit is a SUM (M = sum w^2 n n^T) followed by a 3x3 solve.  Rank g owns the points with x in [edge[g], edge[g+1])
// and also receives halo points within 1.01 r of its edges -- neighbours only, never outputs (gm_set_owned_range).
//   * The cut is made on the host before H2D (no device-to-device halo exchange), by the device-free gm_group_cut.hpp:
//     edges on planes of the VoxelGrid lattice, every row scattered once into per-rank page-locked buffers.
//   * The only exchange step of the path is one all-gather (all_gather below, also behind gm_group_fit_cylinder) of a
//     24-double record per rank (scatter partials, counts, the rank's fitted plane / cylinder): latency bound, a few
//     hundred bytes over xGMI.  RCCL is loaded at run time (dlopen) so that a single-GPU host needs no librccl.
//   * Voxel outputs of the group (centroids, and the normal of every centroid's nearest point: the /surfaceNormals
//     markers, src/tunnel_processing.cpp:237-252) are the ranks' own, merged into ascending pcl key order; the nearest
//     point of a centroid is searched on every rank (it may lie across an edge) and the closest wins.
// Streaming.  Frames that fit one GPU are independent: gm_group_submit_frame hands each to the next device's next free
// slot, gm_group_wait_frame returns them in submission order; no collective.
#include <dlfcn.h>
#include <math.h>
#include <rccl/rccl.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "gm_group_cut.hpp"
#include "gm_internal.hpp"

using namespace gm;

namespace {

constexpr int kRecLen = 24;  // doubles per rank: scatter[6] | n_in n_cropped n_valid n_voxels | plane[4] cyl[7] inliers[2] | pad

struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string &err)
    {
        // ONE RCCL per process.  A Python process with PyTorch-ROCm must use the copy PyTorch bundles (it has no SONAME in
        // common with /opt/rocm's, so the loader would happily map both, and the two tear each other down at exit):
        // geometric_mapping_amd/_lib.py names it in GM_RCCL_PATH.  A host that already has an RCCL mapped (it links one,
        // or loaded one before us) gets THAT copy: RTLD_NOLOAD finds it without mapping a second one.
        const char *names[] = {getenv("GM_RCCL_PATH"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            if (!n || !*n) continue;
            handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
            if (handle) break;
        }
        for (const char *n : names) {
            if (handle) break;
            if (!n || !*n) continue;
            handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!handle) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(handle, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
        AllGather = (decltype(AllGather))dlsym(handle, "ncclAllGather");
        GroupStart = (decltype(GroupStart))dlsym(handle, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(handle, "ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))dlsym(handle, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !AllGather || !GroupStart || !GroupEnd || !GetErrorString) {
            err = "librccl lacks a required symbol";
            return false;
        }
        return true;
    }
};

// FrameOut of a finished frame -> the rank's record, on the device, on the frame's own stream
__global__ void k_pack_record(const FrameOut *__restrict__ o, uint32_t n_in, double *__restrict__ rec)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < 6; ++k) rec[k] = o->scatter[k];
    rec[6] = (double)n_in; rec[7] = (double)o->ctr.n_cropped; rec[8] = (double)o->ctr.n_valid; rec[9] = (double)o->ctr.n_voxels;
    for (int k = 0; k < 4; ++k) rec[10 + k] = (double)o->ext.plane[k];
    for (int k = 0; k < 7; ++k) rec[14 + k] = (double)o->ext.cylinder[k];
    rec[21] = (double)o->ext.plane_inliers; rec[22] = (double)o->ext.cylinder_inliers; rec[23] = 0.0;
}

// the normal AND the point (x, y, z, bits(local input row)) behind every nearest-point index
__global__ __launch_bounds__(256) void k_gather_nearest(const int32_t *__restrict__ idx, uint32_t nq, const float4 *__restrict__ pts,
                                                        float4 *__restrict__ pts_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int32_t j = idx[i];
    pts_out[i] = j >= 0 ? pts[j] : make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct gm_group {
    gm_config cfg;
    uint32_t n = 0;
    bool loopback = false;           // ranks share a device: records travel by device copies, no communicator
    bool dead = false;               // a collective failed half-way: the ranks' streams can no longer be trusted
    // everything one rank owns.  Lives and dies with its device current (gm_group_create, release).
    struct Rank {
        int device = 0;
        gm_ctx *ctx = nullptr;
        DevArray<double> d_rec;           // this rank's record
        DevArray<double> d_all;           // every rank's record (the all-gather's receive buffer)
        hipEvent_t ev = nullptr;          // loopback: "what this rank sends is written"
        HostArray<uint8_t> prow;          // page-locked row buffer of the slab cut (grow-only)
        std::vector<uint32_t> row_ids;    // input row of every row sent
        uint32_t next_slot = 0;           // streaming
        // cylinder regression of the sharded frame (gm_group_fit_cylinder): allocated on first use
        DevArray<double> partial;         // [kFitBlocks][24] the rank's partial rows of a pass
        DevArray<uint32_t> ticket;        // last-block ticket (0 between launches)
        DevArray<CylFitWork> work;        // the model between the passes (every rank writes the same bits)
        DevArray<gm_cylinder_fit> fit;    // the rank's copy of the result record
        DevArray<float> rows8;            // [0..8) starting row, [8..16) published plane row
        DevArray<uint32_t> plane_best;    // 0: the plane row labels; 0xFFFFFFFF: no plane, every label 0
        DevArray<double> row;             // [4 passes][24] the rank's reduced row of each pass (exchange send buffer)
        DevArray<double> rows;            // [4 passes][n][24] every rank's row of each pass (receive buffer; allocated last)
        hipStream_t stream() const { return ctx->slots[0].stream; }   // of the sharded frame: slot 0
        void release()   // the event, the context (gm_destroy drains the rank's streams first), then the rank's blocks
        {
            if (ev) hipEventDestroy(ev);
            if (ctx) gm_destroy(ctx);
            d_rec.release(); d_all.release(); prow.release(); partial.release(); ticket.release(); work.release();
            fit.release(); rows8.release(); plane_best.release(); row.release(); rows.release();
        }
    };
    std::vector<Rank> rank;          // [n]
    std::vector<int> devices;        // [n] and
    std::vector<ncclComm_t> comms;   // [n], contiguous for ncclCommInitAll
    HostArray<double> h_all;         // pinned host copy of rank 0's gathered buffer
    Rccl rccl;
    std::vector<float> xs;           // x of every input row (scratch of the cut)
    std::vector<double> edges;       // of the last cut, and whether they lie on planes of the voxel lattice
    bool edges_on_lattice = false;
    gm_frame_result last = {};
    bool have_frame = false;         // `last`, row_ids and the ranks' slot 0 hold one sharded frame
    double timing[GM_GROUP_N_TIMINGS] = {};
    std::vector<float> vox_cen;      // merged voxel centroids of the last sharded frame: x, y, z, count per voxel
    std::vector<float> vox_nrm;      // ... and the normal of each centroid's nearest point (filled on demand)
    std::vector<int32_t> vox_near;   // ... and that point's index in the merged /choppedCloud
    bool vox_nrm_valid = false;
    HostArray<gm_cylinder_fit> h_fit;     // pinned: [n] the ranks' result records of gm_group_fit_cylinder
    gm_cylinder_fit last_fit = {};
    bool have_fit = false;                // last_fit belongs to the sharded frame in `last`
    // streaming: frames in flight in submission order
    struct Ticket { uint32_t rank, slot; };
    std::deque<Ticket> inflight;
    uint32_t next_rank = 0;
    std::string err;
};

namespace {
thread_local std::string g_group_create_err;

gm_status gfail(gm_group *g, gm_status st, const std::string &msg)
{
    if (g) g->err = msg; else g_group_create_err = msg;
    return st;
}

// a failure behind the first submit: nothing of the frame may still be in flight when we return
gm_status fail_drained(gm_group &G, gm_status st, const std::string &msg)
{
    for (gm_group::Rank &k : G.rank) {
        if (!k.ctx) continue;
        hipSetDevice(k.device);
        for (uint32_t s = 0; s < k.ctx->n_slots; ++s) hipStreamSynchronize(k.ctx->slots[s].stream);
    }
    (void)hipGetLastError();
    return gfail(&G, st, msg);
}

// The one exchange step: `count` doubles of every rank q, send(q), to recv(r) + q * count on every rank r, on the ranks'
// slot-0 streams.  RCCL, or between ranks on one device (tests on a 1-GPU box) device copies ordered by the ranks' events.
template <class Send, class Recv>
gm_status all_gather(gm_group &G, size_t count, Send send, Recv recv)
{
    if (!G.loopback) {
        ncclResult_t rc = G.rccl.GroupStart();
        for (uint32_t r = 0; r < G.n && rc == ncclSuccess; ++r) {
            hipSetDevice(G.rank[r].device);
            rc = G.rccl.AllGather(send(r), recv(r), count, ncclDouble, G.comms[r], G.rank[r].stream());
        }
        const ncclResult_t rc2 = G.rccl.GroupEnd();
        if (rc == ncclSuccess) rc = rc2;
        if (rc == ncclSuccess) return GM_OK;
        // some ranks may have posted their half of the collective: their streams can block for good.  No drain (it
        // could hang with them); the group refuses further work.
        G.dead = true;
        return gfail(&G, GM_ERR_COMM, std::string("ncclAllGather: ") + G.rccl.GetErrorString(rc));
    }
    for (gm_group::Rank &k : G.rank) {
        hipSetDevice(k.device);
        hipEventRecord(k.ev, k.stream());
    }
    for (uint32_t r = 0; r < G.n; ++r) {
        hipSetDevice(G.rank[r].device);
        for (uint32_t q = 0; q < G.n; ++q) {
            if (q != r) hipStreamWaitEvent(G.rank[r].stream(), G.rank[q].ev, 0);
            hipMemcpyAsync(recv(r) + q * count, send(q), sizeof(double) * count, hipMemcpyDeviceToDevice, G.rank[r].stream());
        }
    }
    return GM_OK;
}

// ---- the cut (gm_group_cut.hpp) with the ranks' page-locked buffers allocated between its two calls
gm_status cut_slabs(gm_group &G, const gm_cloud *cloud, CutPlan &plan)
{
    try {   // (the cut allocates and starts threads: nothing may leave through the C ABI)
        const uint32_t T = cut_threads(cloud->n_points);
        cut_plan(G.cfg, G.n, *cloud, T, G.xs, plan);
        std::vector<uint8_t *> rows(G.n);
        std::vector<uint32_t *> ids(G.n);
        for (uint32_t r = 0; r < G.n; ++r) {
            gm_group::Rank &k = G.rank[r];
            const size_t need = (size_t)plan.total[r] * cloud->point_step;
            if (need > k.prow.cap && (hipSetDevice(k.device) != hipSuccess || k.prow.reserve(need + need / 8 + 4096) != hipSuccess))
                return gfail(&G, GM_ERR_OOM, "gm_group: page-locked row buffer allocation failed");
            k.row_ids.resize(plan.total[r]);
            rows[r] = k.prow; ids[r] = k.row_ids.data();
        }
        cut_scatter(*cloud, T, G.xs, plan, rows.data(), ids.data());
    } catch (const std::bad_alloc &) {
        return gfail(&G, GM_ERR_OOM, "gm_group_process_frame: host allocation failed in the slab cut");
    } catch (const std::exception &e) {
        return gfail(&G, GM_ERR_DEVICE, std::string("gm_group_process_frame: the slab cut failed: ") + e.what());
    }
    return GM_OK;
}

// the input row behind the .w of a row of rank r's valid cloud (the bits of its index among the rows sent to r)
bool input_row(const gm_group &G, uint32_t r, const float *w, uint32_t *row)
{
    uint32_t local;
    memcpy(&local, w, 4);
    if (local < G.rank[r].row_ids.size()) *row = G.rank[r].row_ids[local];
    return local < G.rank[r].row_ids.size();
}

struct MergedRow { uint32_t id; float x, y, z; uint8_t label; };

// every rank's valid cloud (and, with_labels, the rank's labels of it) tagged with the input row of each point, in
// ascending input row: the single-GPU order of the sharded frame
gm_status merged_rows(gm_group &G, bool with_labels, std::vector<MergedRow> &all)
{
    all.clear();
    all.reserve(G.last.n_valid);
    std::vector<float> buf;
    std::vector<uint8_t> lab;
    for (uint32_t r = 0; r < G.n; ++r) {
        uint32_t m = G.rank[r].ctx->slots[0].last.n_valid;
        buf.resize((size_t)(m ? m : 1) * 4);
        const gm_status st = gm_get_cropped_xyz(G.rank[r].ctx, 0, buf.data(), m ? m : 1, &m);
        if (st != GM_OK) return gfail(&G, st, gm_last_error(G.rank[r].ctx));
        lab.assign(m ? m : 1, 0);
        if (with_labels && m) {
            Slot &sl = G.rank[r].ctx->slots[0];
            if (hipSetDevice(G.rank[r].device) != hipSuccess ||
                hipMemcpyAsync(lab.data(), sl.labels, m, hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
                hipStreamSynchronize(sl.stream) != hipSuccess)
                return gfail(&G, GM_ERR_DEVICE, "gm_group: D2H of a rank's labels failed");
        }
        for (uint32_t i = 0; i < m; ++i) {
            uint32_t row;
            if (!input_row(G, r, &buf[4 * (size_t)i + 3], &row)) return gfail(&G, GM_ERR_DEVICE, "gm_group: a rank's row index is out of range");
            all.push_back(MergedRow{row, buf[4 * (size_t)i], buf[4 * (size_t)i + 1], buf[4 * (size_t)i + 2], lab[i]});
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const MergedRow &a, const MergedRow &b) { return a.id < b.id; });
    return GM_OK;
}

struct VoxRow { long long kz, ky, kx; float v[4]; };

// Voxel centroids of the group in ascending pcl key order (z slowest, x fastest: the key's order for any box).  Edges on
// the lattice: every voxel belongs to one rank, the ranks' lists are concatenated and ordered.  Otherwise (a lattice too
// coarse to cut along, which always means the dense-table path) a voxel may hold points of two ranks: the ranks' exact
// fixed-point sums are added per cell and divided once, as one rank would have.
gm_status merge_voxels(gm_group &G, const std::vector<gm_frame_result> &rr)
{
    const float inv = 1.0f / (float)G.cfg.voxelGridLeafSize;
    std::vector<VoxRow> rows;
    if (G.edges_on_lattice || G.n == 1) {
        std::vector<float> cen;
        for (uint32_t r = 0; r < G.n; ++r) {
            uint32_t v = rr[r].n_voxels, got = 0;
            cen.resize((size_t)(v ? v : 1) * 4);
            const gm_status st = gm_get_voxel_centroids(G.rank[r].ctx, 0, cen.data(), v ? v : 1, &got);
            if (st != GM_OK) return gfail(&G, st, gm_last_error(G.rank[r].ctx));
            for (uint32_t i = 0; i < got; ++i) {
                VoxRow w;
                w.kx = lattice_cell(cen[4 * i], inv); w.ky = lattice_cell(cen[4 * i + 1], inv); w.kz = lattice_cell(cen[4 * i + 2], inv);
                memcpy(w.v, &cen[4 * (size_t)i], 16);
                rows.push_back(w);
            }
        }
    } else {
        const VoxDense vd = gm_make_vox_dense(G.rank[0].ctx, G.rank[0].ctx->slots[0].cap);
        if (!vd.enabled) return gfail(&G, GM_ERR_UNSUPPORTED, "gm_group: voxel lattice neither cuttable nor dense");
        const size_t cells = (size_t)vd.dim * vd.dim * vd.dim;
        std::vector<VoxCell> sum(cells), part(cells);
        memset(sum.data(), 0, cells * sizeof(VoxCell));
        for (uint32_t r = 0; r < G.n; ++r) {
            Slot &sl = G.rank[r].ctx->slots[0];
            if (hipSetDevice(G.rank[r].device) != hipSuccess ||
                hipMemcpy(part.data(), sl.vox_table, cells * sizeof(VoxCell), hipMemcpyDeviceToHost) != hipSuccess)
                return gfail(&G, GM_ERR_DEVICE, "gm_group: D2H of a rank's voxel table failed");
            for (size_t c = 0; c < cells; ++c) { sum[c].sx += part[c].sx; sum[c].sy += part[c].sy; sum[c].sz += part[c].sz; sum[c].cnt += part[c].cnt; }
        }
        for (size_t c = 0; c < cells; ++c) {
            if (!sum[c].cnt) continue;
            // DenseEmit of k_voxel.hip, operation for operation (the device contracts lo + s * inv into one fma)
            const double q = vd.inv_scale / (double)sum[c].cnt, l = (double)vd.lo;
            VoxRow w;
            w.kx = (long long)(c % vd.dim); w.ky = (long long)((c / vd.dim) % vd.dim); w.kz = (long long)(c / ((size_t)vd.dim * vd.dim));
            w.v[0] = (float)fma((double)sum[c].sx, q, l); w.v[1] = (float)fma((double)sum[c].sy, q, l);
            w.v[2] = (float)fma((double)sum[c].sz, q, l); w.v[3] = (float)sum[c].cnt;
            rows.push_back(w);
        }
    }
    std::stable_sort(rows.begin(), rows.end(), [](const VoxRow &a, const VoxRow &b) {
        return a.kz != b.kz ? a.kz < b.kz : (a.ky != b.ky ? a.ky < b.ky : a.kx < b.kx);
    });
    G.vox_cen.resize(rows.size() * 4);
    for (size_t i = 0; i < rows.size(); ++i) memcpy(&G.vox_cen[4 * i], rows[i].v, 16);
    G.last.n_voxels = (uint32_t)rows.size();
    return GM_OK;
}

// ---- the steps of gm_group_process_frame, in its order.  Reset (whatever happens to the new frame, the accessors must
// not pair its rows with an older frame's results), then what a sharded frame asks of its cloud
gm_status begin_frame(gm_group &G, const gm_cloud *cloud)
{
    G.have_frame = false;
    G.have_fit = false;
    G.last = gm_frame_result{};
    G.vox_cen.clear(); G.vox_nrm.clear(); G.vox_near.clear(); G.vox_nrm_valid = false;
    if (cloud->flags & GM_CLOUD_DEVICE) return gfail(&G, GM_ERR_UNSUPPORTED, "gm_group_process_frame cuts the slabs on the host: pass host rows");
    // (the fit of a sharded frame is a stage call of its own on the resident slabs: gm_group_fit_cylinder)
    if (G.cfg.flags & GM_CFG_CYLINDER_FIT) return gfail(&G, GM_ERR_UNSUPPORTED, "gm_group_process_frame: GM_CFG_CYLINDER_FIT is not supported on sharded frames (call gm_group_fit_cylinder after the frame, or stream frames instead)");
    const uint64_t n = cloud->n_points, step = cloud->point_step;
    if (n && !cloud->data) return gfail(&G, GM_ERR_INVALID_ARG, "gm_cloud.data is NULL");
    if (n && (step < 12 || (uint64_t)cloud->off_x + 4 > step || (uint64_t)cloud->off_y + 4 > step || (uint64_t)cloud->off_z + 4 > step))
        return gfail(&G, GM_ERR_INVALID_ARG, "gm_cloud: x/y/z offsets do not fit in point_step");
    return GM_OK;
}

// every rank runs the unchanged single-GPU pipeline on its slab, asynchronously, and packs its record behind it
gm_status submit_slabs(gm_group &G, const gm_cloud *cloud, const CutPlan &plan)
{
    for (uint32_t r = 0; r < G.n; ++r) {
        gm_group::Rank &k = G.rank[r];
        gm_status st = gm_set_owned_range(k.ctx, G.edges[r], G.edges[r + 1]);
        if (st != GM_OK) return fail_drained(G, st, gm_last_error(k.ctx));
        gm_cloud c = *cloud;
        c.data = plan.total[r] ? k.prow.p : nullptr;
        c.n_points = plan.total[r];
        c.flags = (cloud->flags & GM_CLOUD_BIGENDIAN) | GM_CLOUD_PINNED;
        st = gm_submit_frame(k.ctx, 0, &c);
        if (st != GM_OK) return fail_drained(G, st, std::string("rank ") + std::to_string(r) + ": " + gm_last_error(k.ctx));
        hipLaunchKernelGGL(k_pack_record, dim3(1), dim3(64), 0, k.stream(), (const FrameOut *)k.ctx->slots[0].d_out, c.n_points, k.d_rec.p);
    }
    return GM_OK;
}

// the frame's exchange, rank 0's copy of the gathered records on the host, and every rank's frame done
gm_status gather_records(gm_group &G, std::vector<gm_frame_result> &rr)
{
    gm_status st;
    if ((st = all_gather(G, kRecLen, [&](uint32_t q) { return G.rank[q].d_rec.p; }, [&](uint32_t r) { return G.rank[r].d_all.p; })) != GM_OK) return st;
    hipSetDevice(G.rank[0].device);
    if (hipMemcpyAsync(G.h_all, G.rank[0].d_all, sizeof(double) * kRecLen * G.n, hipMemcpyDeviceToHost, G.rank[0].stream()) != hipSuccess)
        return fail_drained(G, GM_ERR_DEVICE, "D2H of the gathered records failed");
    for (uint32_t r = 0; r < G.n; ++r) {
        st = gm_wait_frame(G.rank[r].ctx, 0, &rr[r]);
        if (st != GM_OK) return fail_drained(G, st, std::string("rank ") + std::to_string(r) + ": " + gm_last_error(G.rank[r].ctx));
    }
    hipSetDevice(G.rank[0].device);
    if (hipStreamSynchronize(G.rank[0].stream()) != hipSuccess) return fail_drained(G, GM_ERR_DEVICE, "stream sync failed");
    return GM_OK;
}

// scatter summed in rank order (deterministic) and solved; every rank holds the same gathered records, rank 0's copy is read
gm_frame_result merge_records(const gm_group &G, uint32_t n_in, uint32_t n_inside)
{
    gm_frame_result out = {};
    out.n_in = n_in; out.n_cropped = n_inside;
    for (uint32_t r = 0; r < G.n; ++r) {
        const double *rec = G.h_all + (size_t)r * kRecLen;
        for (int k = 0; k < 6; ++k) out.scatter[k] += rec[k];
        out.n_valid += (uint32_t)rec[8];
    }
    double w[3], V[9];
    eig3_sym_eigen_signs(out.scatter, w, V);
    for (int k = 0; k < 3; ++k) { out.eigenvalues[k] = (float)w[k]; out.center_axis[k] = (float)V[k]; }
    for (int k = 0; k < 9; ++k) out.eigenvectors[k] = (float)V[k];
    return out;
}

// Fitted primitives (model 0: plane, 1: cylinder): every rank's fit is a candidate for the whole frame; each rank counts
// every candidate's inliers on its own resident valid cloud (owned points only: the counts add up to the count on the
// unsharded frame); the largest total wins, lowest rank on ties.  One process sees every rank: the counts are summed here.
gm_status vote(gm_group &G, int model, const std::vector<gm_frame_result> &rr, gm_frame_result &out)
{
    if (!(G.cfg.flags & (model == 0 ? GM_CFG_RANSAC_PLANE : GM_CFG_RANSAC_CYLINDER))) return GM_OK;
    const int w0 = model == 0 ? 10 : 14, wl = model == 0 ? 4 : 7;
    std::vector<float> cand;
    std::vector<uint32_t> owner;
    for (uint32_t r = 0; r < G.n; ++r) {
        const double *rec = G.h_all + (size_t)r * kRecLen;
        bool ok = rec[21 + model] > 0;
        for (int k = 0; k < wl; ++k) ok = ok && std::isfinite(rec[w0 + k]);
        if (!ok) continue;
        for (int k = 0; k < wl; ++k) cand.push_back((float)rec[w0 + k]);
        owner.push_back(r);
    }
    if (owner.empty()) return GM_OK;
    std::vector<long long> totalc(owner.size(), 0);
    std::vector<int32_t> cnt(owner.size());
    for (uint32_t r = 0; r < G.n; ++r) {
        const gm_status st = gm_score_frame(G.rank[r].ctx, 0, model, cand.data(), (uint32_t)owner.size(), G.cfg.ransac_threshold, 0, cnt.data());
        if (st != GM_OK) return gfail(&G, st, gm_last_error(G.rank[r].ctx));
        for (size_t k = 0; k < owner.size(); ++k) totalc[k] += cnt[k];
    }
    size_t best = 0;
    for (size_t k = 1; k < owner.size(); ++k) if (totalc[k] > totalc[best]) best = k;
    const gm_frame_result &src = rr[owner[best]];
    if (model == 0) {
        out.plane_inliers = (uint32_t)totalc[best];
        for (int k = 0; k < 4; ++k) { out.plane[k] = src.plane[k]; out.plane_refit[k] = src.plane_refit[k]; }
    } else {
        out.cylinder_inliers = (uint32_t)totalc[best];
        for (int k = 0; k < 7; ++k) out.cylinder[k] = src.cylinder[k];
        for (int k = 0; k < 3; ++k) out.cylinder_axis_refit[k] = src.cylinder_axis_refit[k];
    }
    return GM_OK;
}

// The head of the calls that write `count` rows of the sharded frame.  unmet: the message of the call's own precondition
// where it does not hold.  On GM_OK with a count there are rows to write and a buffer that takes them.
gm_status get_head(gm_group &G, const char *unmet, uint32_t count, const void *out, uint32_t capacity, uint32_t *n_out)
{
    if (!G.have_frame) { if (n_out) *n_out = 0; return gfail(&G, GM_ERR_NOT_READY, "gm_group: no completed sharded frame"); }
    if (unmet) return gfail(&G, GM_ERR_NOT_READY, unmet);
    if (n_out) *n_out = count;
    if (count > capacity) return gfail(&G, GM_ERR_CAPACITY, "output buffer too small");
    if (count && !out) return gfail(&G, GM_ERR_INVALID_ARG, "output pointer is NULL");
    return GM_OK;
}

}  // namespace

extern "C" {

const char *gm_group_last_error(const gm_group *grp) { return grp ? grp->err.c_str() : g_group_create_err.c_str(); }
uint32_t gm_group_size(const gm_group *grp) { return grp ? grp->n : 0u; }
gm_ctx *gm_group_ctx(gm_group *grp, uint32_t rank) { return (grp && rank < grp->n) ? grp->rank[rank].ctx : nullptr; }

void gm_group_destroy(gm_group *grp)
{
    if (!grp) return;
    // per rank: communicator (one exists only behind a loaded RCCL, so CommDestroy is set), event, context, blocks
    for (size_t r = 0; r < grp->rank.size(); ++r) {
        if (grp->rank[r].ctx) hipSetDevice(grp->rank[r].device);
        if (grp->comms[r]) grp->rccl.CommDestroy(grp->comms[r]);
        grp->rank[r].release();
    }
    delete grp;
}

gm_status gm_group_create(const gm_config *cfg, const int32_t *devices, uint32_t n_ranks, uint32_t flags, gm_group **out)
{
    if (!cfg || !out || !devices || n_ranks == 0 || n_ranks > 64)
        return gfail(nullptr, GM_ERR_INVALID_ARG, "gm_group_create: bad argument (1..64 ranks)");
    *out = nullptr;
    gm_group *g = new (std::nothrow) gm_group();
    if (!g) return gfail(nullptr, GM_ERR_OOM, "host allocation failed");
    g->cfg = *cfg; g->n = n_ranks;
    bool repeats = false;
    for (uint32_t a = 0; a < n_ranks; ++a)
        for (uint32_t b = a + 1; b < n_ranks; ++b) repeats |= devices[a] == devices[b];
    if (repeats && !(flags & GM_GROUP_LOOPBACK)) {
        delete g;
        return gfail(nullptr, GM_ERR_INVALID_ARG, "gm_group_create: a device is listed twice (pass GM_GROUP_LOOPBACK to allow it)");
    }
    g->loopback = repeats;
    g->rank.resize(n_ranks);
    g->devices.assign(devices, devices + n_ranks); g->comms.assign(n_ranks, nullptr);
    auto bail = [&](gm_status st, const std::string &msg) { g_group_create_err = msg; gm_group_destroy(g); return st; };
    for (uint32_t r = 0; r < n_ranks; ++r) {
        gm_group::Rank &k = g->rank[r];
        gm_config c = *cfg;
        c.device = k.device = devices[r];
        c.ransac_seed = cfg->ransac_seed + r;   // ranks draw different hypotheses: more candidates for the vote
        const gm_status st = gm_create(&c, &k.ctx);
        if (st != GM_OK) return bail(st, std::string("gm_group_create: rank ") + std::to_string(r) + ": " + gm_last_error(nullptr));
        if (hipSetDevice(k.device) != hipSuccess || k.d_rec.reserve(kRecLen) != hipSuccess ||
            k.d_all.reserve((size_t)kRecLen * n_ranks) != hipSuccess ||
            hipEventCreateWithFlags(&k.ev, hipEventDisableTiming) != hipSuccess)
            return bail(GM_ERR_DEVICE, "gm_group_create: device allocation failed");
    }
    if (g->h_all.reserve((size_t)kRecLen * n_ranks) != hipSuccess)
        return bail(GM_ERR_OOM, "gm_group_create: hipHostMalloc failed");
    if (!g->loopback) {
        std::string e;
        if (!g->rccl.load(e)) return bail(GM_ERR_COMM, e);
        const ncclResult_t rc = g->rccl.CommInitAll(g->comms.data(), (int)n_ranks, g->devices.data());
        if (rc != ncclSuccess) return bail(GM_ERR_COMM, std::string("ncclCommInitAll: ") + g->rccl.GetErrorString(rc));
    }
    *out = g;
    return GM_OK;
}

gm_status gm_group_process_frame(gm_group *grp, const gm_cloud *cloud, gm_frame_result *res)
{
    if (!grp || !cloud) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    if (G.dead) return gfail(grp, GM_ERR_COMM, "gm_group: an earlier collective failed; destroy the group");
    if (!G.inflight.empty()) return gfail(grp, GM_ERR_NOT_READY, "gm_group_process_frame: streamed frames are still in flight (gm_group_wait_frame)");
    gm_status st;
    if ((st = begin_frame(G, cloud)) != GM_OK) return st;
    for (int k = 0; k < GM_GROUP_N_TIMINGS; ++k) G.timing[k] = 0.0;
    const double t0 = now_ms();
    CutPlan plan;
    if ((st = cut_slabs(G, cloud, plan)) != GM_OK) return st;
    G.edges = plan.edges; G.edges_on_lattice = plan.on_lattice;
    const double t1 = now_ms();
    if ((st = submit_slabs(G, cloud, plan)) != GM_OK) return st;
    const double t2 = now_ms();
    std::vector<gm_frame_result> rr(G.n);
    if ((st = gather_records(G, rr)) != GM_OK) return st;
    const double t3 = now_ms();
    gm_frame_result out = merge_records(G, cloud->n_points, plan.n_inside);
    if (G.cfg.flags & GM_CFG_VOXEL_GRID) {
        st = merge_voxels(G, rr);
        if (st == GM_OK) out.n_voxels = G.last.n_voxels;
    }
    for (int model = 0; model < 2 && st == GM_OK; ++model) st = vote(G, model, rr, out);
    if (st != GM_OK) { G.last = gm_frame_result{}; return st; }
    for (uint32_t r = 0; r < G.n; ++r) out.normals_kernel_ms = fmaxf(out.normals_kernel_ms, rr[r].normals_kernel_ms);
    const double t4 = now_ms();
    G.timing[GM_GROUP_T_CUT] = t1 - t0; G.timing[GM_GROUP_T_SUBMIT] = t2 - t1; G.timing[GM_GROUP_T_DEVICE] = t3 - t2;
    G.timing[GM_GROUP_T_MERGE] = t4 - t3; G.timing[GM_GROUP_T_TOTAL] = t4 - t0;
    G.last = out;
    G.have_frame = true;
    if (res) *res = out;
    return GM_OK;
}

gm_status gm_group_get_timing(const gm_group *grp, double *ms, uint32_t capacity)
{
    if (!grp || !ms) return GM_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < capacity && k < (uint32_t)GM_GROUP_N_TIMINGS; ++k) ms[k] = grp->timing[k];
    return GM_OK;
}

gm_status gm_group_get_edges(const gm_group *grp, double *edges, uint32_t capacity, uint32_t *on_lattice)
{
    if (!grp || !edges) return GM_ERR_INVALID_ARG;
    if (capacity < grp->n + 1 || grp->edges.size() != (size_t)grp->n + 1) return GM_ERR_CAPACITY;
    for (uint32_t k = 0; k <= grp->n; ++k) edges[k] = grp->edges[k];
    if (on_lattice) *on_lattice = grp->edges_on_lattice ? 1u : 0u;
    return GM_OK;
}

// /choppedCloud of a sharded frame: every rank's valid cloud, merged back into the single-GPU order (ascending input
// row).  Rows x,y,z,pad with pad = the row index in the ORIGINAL cloud.
gm_status gm_group_get_cropped_xyz(gm_group *grp, float *xyzw, uint32_t capacity, uint32_t *n_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    gm_status st = get_head(*grp, nullptr, grp->last.n_valid, xyzw, capacity, n_out);
    if (st != GM_OK || !grp->last.n_valid) return st;
    std::vector<MergedRow> all;
    if ((st = merged_rows(*grp, false, all)) != GM_OK) return st;
    for (size_t i = 0; i < all.size() && i < capacity; ++i) {
        xyzw[4 * i] = all[i].x; xyzw[4 * i + 1] = all[i].y; xyzw[4 * i + 2] = all[i].z;
        memcpy(&xyzw[4 * i + 3], &all[i].id, 4);
    }
    return GM_OK;
}

// labels of a sharded frame, in the order of gm_group_get_cropped_xyz
gm_status gm_group_get_labels(gm_group *grp, uint8_t *labels, uint32_t capacity, uint32_t *n_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    const bool fitted = (grp->cfg.flags & (GM_CFG_RANSAC_PLANE | GM_CFG_RANSAC_CYLINDER)) || grp->have_fit;
    if (!fitted && n_out) *n_out = 0;
    gm_status st = get_head(*grp, fitted ? nullptr : "gm_group_get_labels: group created without a GM_CFG_RANSAC_* flag and no gm_group_fit_cylinder on this frame",
                            grp->last.n_valid, labels, capacity, n_out);
    if (st != GM_OK || !grp->last.n_valid) return st;
    std::vector<MergedRow> all;
    if ((st = merged_rows(*grp, true, all)) != GM_OK) return st;
    for (size_t i = 0; i < all.size() && i < capacity; ++i) labels[i] = all[i].label;
    return GM_OK;
}

gm_status gm_group_get_voxel_centroids(gm_group *grp, float *xyzc, uint32_t capacity, uint32_t *n_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    const char *unmet = (grp->cfg.flags & GM_CFG_VOXEL_GRID) ? nullptr : "group created without GM_CFG_VOXEL_GRID";
    const uint32_t V = (uint32_t)(grp->vox_cen.size() / 4);
    const gm_status st = get_head(*grp, unmet, V, xyzc, capacity, n_out);
    if (st == GM_OK && V) memcpy(xyzc, grp->vox_cen.data(), (size_t)V * 16);
    return st;
}

// The normal of every centroid's nearest valid point (normals->at(kIndices[0]) of the marker loop, src/tunnel_processing.cpp:
// 239-249).  The nearest point of a centroid next to a slab edge may belong to the neighbouring rank: every rank searches
// every centroid in its own valid cloud, the smallest (distance, input row) wins -- the 1-NN of the unsharded frame.
gm_status gm_group_get_voxel_normals(gm_group *grp, float *nxyzc, uint32_t capacity, uint32_t *n_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    const bool flags_ok = (G.cfg.flags & (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID)) == (GM_CFG_NEAREST | GM_CFG_VOXEL_GRID);
    const uint32_t V = (uint32_t)(G.vox_cen.size() / 4);
    gm_status st = get_head(G, flags_ok ? nullptr : "group created without GM_CFG_NEAREST | GM_CFG_VOXEL_GRID", V, nxyzc, capacity, n_out);
    if (st != GM_OK || !V) return st;
    if (!G.vox_nrm_valid) {
        G.vox_nrm.assign((size_t)V * 4, std::numeric_limits<float>::quiet_NaN());
        std::vector<unsigned long long> best_key(V, ~0ull);   // (distance bits << 32 | input row) of the winner so far
        std::vector<unsigned long long> keys;
        std::vector<float> nrm, pts;
        for (uint32_t r = 0; r < G.n; ++r) {
            Slot &sl = G.rank[r].ctx->slots[0];
            if (hipSetDevice(G.rank[r].device) != hipSuccess) return gfail(grp, GM_ERR_DEVICE, "hipSetDevice failed");
            if (sl.last.n_valid == 0) continue;
            // queries go through the rank's own centroid buffer in pieces of at most its capacity (its own centroids
            // were fetched by the merge already); results through its nearest-point scratch
            for (uint32_t q0 = 0; q0 < V; q0 += sl.cap) {
                const uint32_t nq = V - q0 < sl.cap ? V - q0 : sl.cap;
                if (hipMemcpyAsync(sl.vox4, &G.vox_cen[(size_t)q0 * 4], (size_t)nq * 16, hipMemcpyHostToDevice, sl.stream) != hipSuccess)
                    return gfail(grp, GM_ERR_DEVICE, "gm_group: upload of the merged centroids failed");
                launch_nearest(sl.crop4, &sl.ctr->n_valid, sl.cap, sl.vox4, nullptr, nq, sl.nn_best, sl.vox_nn, sl.stream, sl.normals4, sl.vox_nrm4);
                hipLaunchKernelGGL(k_gather_nearest, dim3((nq + 255) / 256), dim3(256), 0, sl.stream, (const int32_t *)sl.vox_nn, nq,
                                   (const float4 *)sl.crop4, sl.spts4);
                keys.resize(nq); nrm.resize((size_t)nq * 4); pts.resize((size_t)nq * 4);
                if (hipMemcpyAsync(keys.data(), sl.nn_best, (size_t)nq * 8, hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
                    hipMemcpyAsync(nrm.data(), sl.vox_nrm4, (size_t)nq * 16, hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
                    hipMemcpyAsync(pts.data(), sl.spts4, (size_t)nq * 16, hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
                    hipStreamSynchronize(sl.stream) != hipSuccess)
                    return gfail(grp, GM_ERR_DEVICE, "gm_group: nearest-point search failed");
                for (uint32_t i = 0; i < nq; ++i) {
                    if (keys[i] == ~0ull) continue;
                    uint32_t row;
                    if (!input_row(G, r, &pts[4 * (size_t)i + 3], &row)) return gfail(grp, GM_ERR_DEVICE, "gm_group: a rank's row index is out of range");
                    const unsigned long long k = (keys[i] & 0xFFFFFFFF00000000ull) | row;
                    if (k < best_key[q0 + i]) {
                        best_key[q0 + i] = k;
                        memcpy(&G.vox_nrm[4 * (size_t)(q0 + i)], &nrm[4 * (size_t)i], 16);
                    }
                }
            }
        }
        // the winners' positions in the merged /choppedCloud (gm_group_get_voxel_nearest): rank of their input row
        // among the valid rows, which merged_rows lists in ascending order
        std::vector<MergedRow> all;
        if ((st = merged_rows(G, false, all)) != GM_OK) return st;
        G.vox_near.assign(V, -1);
        for (uint32_t i = 0; i < V; ++i) {
            if (best_key[i] == ~0ull) continue;
            const uint32_t row = (uint32_t)(best_key[i] & 0xFFFFFFFFull);
            G.vox_near[i] = (int32_t)(std::lower_bound(all.begin(), all.end(), row, [](const MergedRow &a, uint32_t v) { return a.id < v; }) - all.begin());
        }
        G.vox_nrm_valid = true;
    }
    memcpy(nxyzc, G.vox_nrm.data(), (size_t)V * 16);
    return GM_OK;
}

gm_status gm_group_get_voxel_nearest(gm_group *grp, int32_t *idx, uint32_t capacity, uint32_t *n_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    const uint32_t V = (uint32_t)(grp->vox_cen.size() / 4);
    gm_status st = get_head(*grp, nullptr, V, idx, capacity, n_out);
    if (st != GM_OK || !V) return st;
    if (!grp->vox_nrm_valid) {
        std::vector<float> tmp((size_t)V * 4);
        if ((st = gm_group_get_voxel_normals(grp, tmp.data(), V, nullptr)) != GM_OK) return st;
    }
    memcpy(idx, grp->vox_near.data(), (size_t)V * 4);
    return GM_OK;
}

// ---- cylinder regression of the sharded frame (DESIGN.md par. 4 "Multi-device") ------------------------------------
// The fit is a sum followed by a 5x5 solve, so it shards like the scatter matrix: every rank runs the single-device
// launches (k_cylfit.hip) on its resident valid cloud -- owned points only, so the ranks' sums add up to the frame's --
// and writes its reduced 24-double row instead of solving; the rows are all-gathered (RCCL, or event-ordered device
// copies on a loopback group) and k_cylfit_merge, on every rank, sums them in rank order and runs the single-device
// solve.  4 exchange rounds per fit (3 Gauss-Newton passes, 1 label pass), everything enqueued, one wait at the end.
gm_status gm_group_fit_cylinder(gm_group *grp, const float init7[7], gm_cylinder_fit *out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    if (G.dead) return gfail(grp, GM_ERR_COMM, "gm_group: an earlier collective failed; destroy the group");
    if (!out) return gfail(grp, GM_ERR_INVALID_ARG, "gm_group_fit_cylinder: NULL argument");
    if (!G.have_frame) return gfail(grp, GM_ERR_NOT_READY, "gm_group: no completed sharded frame");
    G.have_fit = false;
    const uint32_t R = G.n;
    const double tau = G.cfg.ransac_threshold;
    if (!(tau > 0.0) || !std::isfinite(tau)) return gfail(grp, GM_ERR_INVALID_ARG, "gm_group_fit_cylinder: ransac_threshold must be > 0");
    // work buffers (first call; a context created without GM_CFG_CYLINDER_FIT has none of its own)
    for (gm_group::Rank &f : G.rank) {
        if (f.rows) continue;
        if (hipSetDevice(f.device) != hipSuccess) return gfail(grp, GM_ERR_DEVICE, "hipSetDevice failed");
        if (f.partial.reserve((size_t)kFitBlocks * kFitRowLen) != hipSuccess || f.ticket.reserve(1) != hipSuccess ||
            hipMemset(f.ticket, 0, sizeof(uint32_t)) != hipSuccess ||   // (k_cylfit resets it after every launch)
            f.work.reserve(1) != hipSuccess || f.fit.reserve(1) != hipSuccess || f.rows8.reserve(16) != hipSuccess ||
            f.plane_best.reserve(1) != hipSuccess || f.row.reserve((size_t)4 * kFitRowLen) != hipSuccess ||
            f.rows.reserve((size_t)4 * kFitRowLen * R) != hipSuccess)
            return gfail(grp, GM_ERR_OOM, "gm_group_fit_cylinder: device allocation failed");
    }
    if (G.h_fit.reserve(R) != hipSuccess) return gfail(grp, GM_ERR_OOM, "gm_group_fit_cylinder: hipHostMalloc failed");
    // the starting row (caller's, or the published cylinder: NaN when the frame has none) and the published plane
    const float nanf_ = std::numeric_limits<float>::quiet_NaN();
    float rows8[16];
    for (int k = 0; k < 16; ++k) rows8[k] = 0.f;
    const bool has_cyl = (G.cfg.flags & GM_CFG_RANSAC_CYLINDER) && G.last.cylinder_inliers > 0;
    for (int k = 0; k < 7; ++k) rows8[k] = init7 ? init7[k] : (has_cyl ? G.last.cylinder[k] : nanf_);
    bool has_plane = (G.cfg.flags & GM_CFG_RANSAC_PLANE) && G.last.plane_inliers > 0;
    for (int k = 0; k < 4; ++k) { rows8[8 + k] = G.last.plane[k]; has_plane = has_plane && std::isfinite(G.last.plane[k]); }
    const uint32_t plane_best = has_plane ? 0u : 0xFFFFFFFFu;
    std::vector<CylFitArgs> args(R);
    for (uint32_t r = 0; r < R; ++r) {
        gm_group::Rank &f = G.rank[r];
        Slot &sl = f.ctx->slots[0];
        if (hipSetDevice(f.device) != hipSuccess ||
            hipMemcpyAsync(f.rows8, rows8, sizeof(rows8), hipMemcpyHostToDevice, sl.stream) != hipSuccess ||
            hipMemcpyAsync(f.plane_best, &plane_best, sizeof(uint32_t), hipMemcpyHostToDevice, sl.stream) != hipSuccess)
            return fail_drained(G, GM_ERR_DEVICE, "gm_group_fit_cylinder: upload of the starting rows failed");
        // plane relabel: every valid point 1 if it is an inlier of the published plane (the RANSAC's fp32 predicate), else 0
        launch_label(0, sl.crop4, sl.labels, 0, 1, &sl.ctr->n_valid, sl.last.n_valid, f.rows8 + 8, nullptr, f.plane_best,
                     tau, 1, nullptr, nullptr, 0, sl.stream);
        CylFitArgs &a = args[r];
        a.pts = sl.crop4; a.labels = sl.labels; a.out = sl.labels;
        a.want = 0; a.want2 = 0; a.mask_mode = 0;   // eligible: what the published plane left
        a.n_ptr = &sl.ctr->n_valid; a.n_host = sl.last.n_valid;
        a.init = f.rows8; a.best = nullptr;
        a.work = f.work; a.fit = f.fit; a.partial = f.partial; a.ticket = f.ticket;
        a.tau = tau;
    }
    for (int pass = 0; pass < 4; ++pass) {
        // rank q's row -> rows[pass][q] on every rank (per-pass buffers: no rank overwrites a row still being copied)
        auto row = [&](uint32_t q) { return G.rank[q].row + (size_t)pass * kFitRowLen; };
        auto rows = [&](uint32_t r) { return G.rank[r].rows + (size_t)pass * kFitRowLen * R; };
        for (uint32_t r = 0; r < R; ++r) {
            hipSetDevice(G.rank[r].device);
            CylFitArgs a = args[r];
            a.rank_row = row(r);
            launch_cylinder_fit_pass(a, pass, G.rank[r].stream());
        }
        if (const gm_status st = all_gather(G, kFitRowLen, row, rows); st != GM_OK) return st;
        for (uint32_t r = 0; r < R; ++r) {
            hipSetDevice(G.rank[r].device);
            launch_cylinder_fit_merge(args[r], pass, rows(r), R, G.rank[r].stream());
        }
    }
    for (uint32_t r = 0; r < R; ++r) {
        hipSetDevice(G.rank[r].device);
        if (hipMemcpyAsync(&G.h_fit[r], G.rank[r].fit, sizeof(gm_cylinder_fit), hipMemcpyDeviceToHost, G.rank[r].stream()) != hipSuccess)
            return fail_drained(G, GM_ERR_DEVICE, "gm_group_fit_cylinder: D2H of a rank's fit failed");
    }
    for (uint32_t r = 0; r < R; ++r) {
        hipSetDevice(G.rank[r].device);
        if (hipStreamSynchronize(G.rank[r].stream()) != hipSuccess || hipGetLastError() != hipSuccess)
            return fail_drained(G, GM_ERR_DEVICE, std::string("gm_group_fit_cylinder: rank ") + std::to_string(r) + ": the fit's launches failed");
    }
    // every rank solved the same sums: the records must agree bit for bit (padding excluded)
    const size_t cmp = offsetof(gm_cylinder_fit, model) + sizeof(((gm_cylinder_fit *)nullptr)->model);
    for (uint32_t r = 1; r < R; ++r)
        if (memcmp(&G.h_fit[r], &G.h_fit[0], cmp) != 0)
            return gfail(grp, GM_ERR_DEVICE, std::string("gm_group_fit_cylinder: rank ") + std::to_string(r) + "'s fit differs from rank 0's");
    G.last_fit = G.h_fit[0];
    G.last_fit.struct_size = (uint32_t)sizeof(gm_cylinder_fit);
    G.have_fit = true;
    *out = G.last_fit;
    return GM_OK;
}

gm_status gm_group_get_cylinder_fit(const gm_group *grp, gm_cylinder_fit *out)
{
    if (!grp || !out) return GM_ERR_INVALID_ARG;
    if (!grp->have_frame || !grp->have_fit) return GM_ERR_NOT_READY;
    *out = grp->last_fit;
    return GM_OK;
}

// ---- streaming: whole frames, round-robin over the group's devices ---------------------------------------------------
// (BASELINE configs[4]; replaces the one-frame-at-a-time consumer of src/geometric_mapping.cpp:146,169.)

uint32_t gm_group_in_flight(const gm_group *grp) { return grp ? (uint32_t)grp->inflight.size() : 0u; }

gm_status gm_group_submit_frame(gm_group *grp, const gm_cloud *cloud)
{
    if (!grp || !cloud) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    if (G.dead) return gfail(grp, GM_ERR_COMM, "gm_group: an earlier collective failed; destroy the group");
    uint32_t cap = 0;
    for (uint32_t r = 0; r < G.n; ++r) cap += G.rank[r].ctx->n_slots;
    if (G.inflight.size() >= cap) return gfail(grp, GM_ERR_NOT_READY, "gm_group_submit_frame: every slot holds a frame (gm_group_wait_frame first)");
    // the next device in turn that has a free slot (slots of a rank are used in ring order, so the oldest frees first)
    for (uint32_t tries = 0; tries < G.n; ++tries) {
        const uint32_t r = (G.next_rank + tries) % G.n;
        uint32_t used = 0;
        for (const gm_group::Ticket &t : G.inflight) used += t.rank == r ? 1u : 0u;
        if (used >= G.rank[r].ctx->n_slots) continue;
        const uint32_t slot = G.rank[r].next_slot;
        // a sharded frame (also one that failed half-way) leaves the ranks with slab ranges: rank 0 owns (-inf, edge[1]),
        // so BOTH ends have to be looked at -- a streamed frame is a whole frame, every point of it is the rank's own
        if (G.rank[r].ctx->own_lo != -std::numeric_limits<double>::infinity() ||
            G.rank[r].ctx->own_hi != std::numeric_limits<double>::infinity()) {
            const gm_status st = gm_set_owned_range(G.rank[r].ctx, -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity());
            if (st != GM_OK) return gfail(grp, st, gm_last_error(G.rank[r].ctx));
        }
        const gm_status st = gm_submit_frame(G.rank[r].ctx, slot, cloud);
        if (st != GM_OK) return gfail(grp, st, std::string("rank ") + std::to_string(r) + ": " + gm_last_error(G.rank[r].ctx));
        G.have_frame = false;   // slot 0 of the ranks no longer holds a sharded frame
        G.inflight.push_back(gm_group::Ticket{r, slot});
        G.rank[r].next_slot = (slot + 1) % G.rank[r].ctx->n_slots;
        G.next_rank = (r + 1) % G.n;
        return GM_OK;
    }
    return gfail(grp, GM_ERR_NOT_READY, "gm_group_submit_frame: no free slot");
}

gm_status gm_group_poll_frame(gm_group *grp)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    if (G.inflight.empty()) return GM_ERR_NOT_READY;
    const gm_group::Ticket t = G.inflight.front();
    const gm_status st = gm_poll_frame(G.rank[t.rank].ctx, t.slot);
    if (st != GM_OK && st != GM_ERR_NOT_READY) return gfail(grp, st, std::string("rank ") + std::to_string(t.rank) + ": " + gm_last_error(G.rank[t.rank].ctx));
    return st;
}

gm_status gm_group_wait_frame(gm_group *grp, gm_frame_result *res, uint32_t *rank_out, uint32_t *slot_out)
{
    if (!grp) return GM_ERR_INVALID_ARG;
    gm_group &G = *grp;
    if (G.inflight.empty()) return gfail(grp, GM_ERR_NOT_READY, "gm_group_wait_frame: no frame in flight");
    const gm_group::Ticket t = G.inflight.front();
    G.inflight.pop_front();
    if (rank_out) *rank_out = t.rank;
    if (slot_out) *slot_out = t.slot;
    const gm_status st = gm_wait_frame(G.rank[t.rank].ctx, t.slot, res);
    if (st != GM_OK) return gfail(grp, st, std::string("rank ") + std::to_string(t.rank) + ": " + gm_last_error(G.rank[t.rank].ctx));
    return GM_OK;
}

}  // extern "C"
