/*
 * gm_hip.h -- C ABI of libgm_hip.so: the MI355X (gfx950) implementation of the
 * geometric_mapping per-frame point-cloud path.
 *
 * The reference exposes this path as plain C++ free functions linked into one
 * ROS executable (there is no plugin / FFI layer to bind to):
 *   /root/reference include/geometric_mapping/tunnel_processing.hpp:38-54,77-82
 *   called only from cloud_cb, /root/reference src/geometric_mapping.cpp:48-125.
 * This header is the boundary a catkin host links instead; every entry point
 * cites the reference interface it replaces.  No PCL / Eigen / ROS / torch
 * types cross it: plain pointers, sizes and POD structs only.  Nothing throws.
 *
 * Threading: a gm_ctx is NOT thread-safe (the reference's callback never
 * re-enters either: ros::spin(), src/geometric_mapping.cpp:169).  Use one
 * context per calling thread.  All device work of a context runs on HIP
 * streams it owns (one per slot).
 *
 * There is no CPU fallback behind this ABI: if no gfx950 device is usable,
 * gm_create fails with GM_ERR_DEVICE.
 */
#ifndef GM_HIP_H
#define GM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_ABI_VERSION 3u

typedef struct gm_ctx gm_ctx; /* opaque */

typedef enum gm_status {
    GM_OK = 0,
    GM_ERR_INVALID_ARG = 1,
    GM_ERR_TOO_FEW_POINTS = 2, /* reserved: stages accept empty clouds like the reference does */
    GM_ERR_DEVICE = 3,         /* a HIP call failed; gm_last_error() has the hipError string */
    GM_ERR_OOM = 4,
    GM_ERR_CAPACITY = 5,       /* caller buffer too small; *n_out holds the needed count */
    GM_ERR_NOT_READY = 6,      /* slot has no submitted / completed frame */
    GM_ERR_UNSUPPORTED = 7,
    GM_ERR_COMM = 8            /* RCCL could not be loaded or a collective failed (gm_group_*) */
} gm_status;

/* gm_config.flags */
#define GM_CFG_VOXEL_GRID      (1u << 0) /* run VoxelGrid every frame, as the reference does
                                            (src/geometric_mapping.cpp:70-75 is not gated) */
#define GM_CFG_NEAREST         (1u << 1) /* also 1-NN of every voxel centroid
                                            (src/tunnel_processing.cpp:237-239; only /surfaceNormals needs it) */
#define GM_CFG_RANSAC_PLANE    (1u << 2) /* extension, no reference counterpart */
#define GM_CFG_RANSAC_CYLINDER (1u << 3) /* extension, no reference counterpart */
#define GM_CFG_STAGE_TIMING    (1u << 4) /* bracket stages with hipEvents -> gm_frame_result.stage_ms */
#define GM_CFG_KEEP_COUNTS     (1u << 5) /* keep per-point neighbour counts (tests) */
#define GM_CFG_GRAPH           (1u << 6) /* capture the frame's launch chain as a hipGraph once and replay it for every
                                            frame of about the same size (launch-bound small frames; results are the
                                            same bit for bit; normals_kernel_ms / stage_ms are not measured) */
#define GM_CFG_CYLINDER_FIT    (1u << 7) /* least-squares regression of the RANSAC cylinder (needs GM_CFG_RANSAC_CYLINDER):
                                            gm_get_cylinder_fit, relabelled cylinder points, fitted map record */
#define GM_CFG_SURFACE_MAP     (1u << 8) /* wall deviation map against the fitted cylinder (needs GM_CFG_CYLINDER_FIT):
                                            gm_get_surface_map, gm_get_surface_points */
#define GM_CFG_DEFAULT         (GM_CFG_VOXEL_GRID)

/* The four numeric parameters are the reference's, with its types:
 * include/geometric_mapping/paramHandler.hpp:26-29 (all double). */
typedef struct gm_config {
    uint32_t struct_size;        /* = sizeof(gm_config) */
    uint32_t flags;              /* GM_CFG_* */
    double   boxFilterBound;     /* launch/mapping.launch:7  */
    double   voxelGridLeafSize;  /* launch/mapping.launch:8  */
    double   neighborRadius;     /* launch/mapping.launch:9  */
    double   weightingFactor;    /* launch/mapping.launch:10 */
    int32_t  device;             /* HIP device ordinal */
    uint32_t n_slots;            /* frames in flight (>=1); 2 overlaps H2D of frame i+1 with compute of i.  Every slot has its own
                                    HIP stream, created at the device's greatest stream priority: ROCm maps a process's streams onto
                                    GPU_MAX_HW_QUEUES hardware queues (default 4) per priority, so up to 4 slots have a queue each
                                    whatever other streams the process holds (measured: 4 slots 0.198 ms per 1 M-point frame, 3 slots
                                    0.210; more slots than queues share them and lose: DESIGN.md par. 7) */
    uint32_t max_points;         /* capacity hint; buffers grow on demand */
    uint32_t ransac_hypotheses;  /* H per model per frame (extension) */
    double   ransac_threshold;   /* tau, metres (extension) */
    uint64_t ransac_seed;        /* extension */
} gm_config;

/* gm_cloud.flags */
#define GM_CLOUD_DEVICE    (1u << 0) /* data is a device pointer valid on the context's device */
#define GM_CLOUD_BIGENDIAN (1u << 1) /* sensor_msgs/PointCloud2.is_bigendian */
#define GM_CLOUD_PINNED    (1u << 2) /* data is page-locked host memory from gm_host_alloc: it is copied to the device
                                        straight from there (no staging copy on the calling thread) and must stay
                                        untouched until gm_wait_frame / the blocking call returns */

/* One sensor_msgs/PointCloud2 worth of rows: what pcl::fromROSMsg reads at
 * src/geometric_mapping.cpp:55.  x,y,z are float32 at byte offsets off_* of
 * each point_step-byte row. */
typedef struct gm_cloud {
    const void *data;
    uint32_t n_points;
    uint32_t point_step;
    uint32_t off_x, off_y, off_z;
    uint32_t flags;
} gm_cloud;

enum { GM_STAGE_UPLOAD = 0, GM_STAGE_CROP, GM_STAGE_GRID, GM_STAGE_NORMALS, GM_STAGE_COMPACT,
       GM_STAGE_FRAME, GM_STAGE_VOXEL, GM_STAGE_RANSAC, GM_STAGE_TOTAL, GM_N_STAGES };

/* gm_frame_result.status_flags */
#define GM_RES_VOXEL_PASSTHROUGH (1u << 0) /* PCL "leaf size too small" guard: voxel output = input */

typedef struct gm_frame_result {
    uint32_t n_in;         /* points received */
    uint32_t n_cropped;    /* after chopCloud                          (src/geometric_mapping.cpp:57) */
    uint32_t n_valid;      /* after NaN-normal removal inside getNormals (:63)                       */
    uint32_t n_voxels;     /* VoxelGrid output size                    (src/tunnel_processing.cpp:220) */
    float    eigenvalues[3];   /* ascending, = *eigenVals              (src/tunnel_processing.cpp:132) */
    float    eigenvectors[9];  /* column-major like Eigen::Matrix3f    (src/tunnel_processing.cpp:136) */
    float    center_axis[3];   /* eigenvectors column 0                (src/geometric_mapping.cpp:92)  */
    uint32_t status_flags;
    double   scatter[6];       /* M = sum w^2 n n^T: xx,xy,xz,yy,yz,zz in fp64 (multi-GPU merge unit) */
    /* extensions (valid only with the GM_CFG_RANSAC_* flags) */
    uint32_t plane_inliers, cylinder_inliers;
    float    plane[4];         /* a,b,c,d  (unit normal)                */
    float    cylinder[7];      /* point on axis, unit axis direction, radius */
    double   plane_refit[4];   /* least-squares refit over the plane segment */
    double   cylinder_axis_refit[3]; /* min-eigenvector of sum nn^T over the cylinder segment */
    float    stage_ms[GM_N_STAGES];  /* device time per stage when GM_CFG_STAGE_TIMING; else 0 */
    float    normals_kernel_ms;      /* the neighbourhood-normals kernel alone (hipEvent bracketed) */
} gm_frame_result;

/* ---- lifetime ------------------------------------------------------------ */

/* Replaces the start-up half of main(): src/geometric_mapping.cpp:128-161
 * (parameters are read once; there is no dynamic reconfigure).  Picks the
 * device, creates one stream + pinned staging + device buffers per slot. */
gm_status gm_create(const gm_config *cfg, gm_ctx **out);
void gm_destroy(gm_ctx *ctx);

/* Page-locked host memory for GM_CLOUD_PINNED input (e.g. the buffer a driver or a custom ROS allocator fills with
 * PointCloud2 rows).  Owned by the caller until gm_host_free; outlives nothing: free it before gm_destroy. */
gm_status gm_host_alloc(gm_ctx *ctx, size_t bytes, void **out);
gm_status gm_host_free(gm_ctx *ctx, void *ptr);
/* The same for memory the caller already owns (e.g. the data vector of a pre-allocated sensor_msgs/PointCloud2 that a
 * node publishes from: gm_set_cloud_output then delivers /choppedCloud straight into the message): page-locks
 * [ptr, ptr + bytes) until gm_host_unregister.  Registered memory may be used wherever gm_host_alloc memory may. */
gm_status gm_host_register(gm_ctx *ctx, void *ptr, size_t bytes);
gm_status gm_host_unregister(gm_ctx *ctx, void *ptr);

/* Defaults = the launch file's values (launch/mapping.launch:7-10). */
void gm_default_config(gm_config *cfg);

uint32_t gm_abi_version(void);
/* Diagnostic (tests): device and page-locked blocks the library itself holds right now, process-wide.  Back at its
 * earlier value once every context, wall map and group created since has been destroyed (gm_host_alloc memory is the
 * caller's and is not counted). */
long long gm_debug_live_buffers(void);
const char *gm_status_string(gm_status s);
/* Message of the last failure on this context ("" if none).  ctx may be NULL
 * for a failure inside gm_create. */
const char *gm_last_error(const gm_ctx *ctx);

/* ---- the per-frame callback ------------------------------------------------ */

/* Replaces the processing half of cloud_cb, src/geometric_mapping.cpp:55-92:
 * fromROSMsg -> chopCloud -> getNormals -> VoxelGrid (inside rvizNormals) ->
 * getLocalFrame -> centerAxis.  Blocking; uses slot 0. */
gm_status gm_process_frame(gm_ctx *ctx, const gm_cloud *cloud, gm_frame_result *res);

/* Same work split for streaming (BASELINE config 5): submit returns once the
 * host buffer has been staged and all device work is enqueued on the slot's
 * stream; wait blocks until that frame's result is on the host.  The host
 * buffer may be reused as soon as submit returns. */
gm_status gm_submit_frame(gm_ctx *ctx, uint32_t slot, const gm_cloud *cloud);
gm_status gm_wait_frame(gm_ctx *ctx, uint32_t slot, gm_frame_result *res);
/* Completion query, never blocks: GM_OK when the slot's submitted frame has finished (gm_wait_frame will return at once),
 * GM_ERR_NOT_READY while it is still running or when the slot holds no submitted frame.  The reference publishes every
 * frame inside its own callback (src/geometric_mapping.cpp:100-117); a host that keeps frames in flight polls at the top
 * of each callback (and on a timer) and publishes what has finished, instead of waiting for the pipeline to fill. */
gm_status gm_poll_frame(gm_ctx *ctx, uint32_t slot);

/* /choppedCloud straight into host memory (the default launch has displayCloud = true: launch/mapping.launch:12,
 * src/geometric_mapping.cpp:100-107).  xyzw = page-locked memory from gm_host_alloc with room for capacity rows of
 * 4 floats (x, y, z, pad = input row index), owned by the caller, or NULL to switch the output off for the slot.  Every
 * later frame of the slot copies its valid cloud there -- the copy starts right behind the NaN-normal compaction, on a
 * stream of its own, and runs while the rest of the frame (voxel grid, RANSAC, eigen solve) executes -- and is complete
 * when gm_wait_frame returns; rows [0, n_valid) are the frame's, identical to gm_get_cropped_xyz's.  A frame with more
 * points than capacity is refused with GM_ERR_CAPACITY at submit. */
gm_status gm_set_cloud_output(gm_ctx *ctx, uint32_t slot, float *xyzw, uint32_t capacity);

/* Bulky per-frame outputs of a completed slot, fetched only when a display
 * flag needs them (src/geometric_mapping.cpp:100-117).  `capacity` counts
 * points; *n_out receives the available count (also on GM_ERR_CAPACITY).
 *   cropped xyz : /choppedCloud = cloudChopped AFTER the in-place NaN compaction
 *                 (src/tunnel_processing.cpp:81-85), rows of 4 floats x,y,z,pad
 *                 = pcl::PointXYZ; pad holds the point's row index in the input
 *                 cloud as int32 bits.
 *   normals     : rows nx,ny,nz,curvature (the meaningful fields of pcl::Normal)
 *   voxels      : VoxelGrid centroids in ascending voxel-key order, rows x,y,z,count
 *   nearest     : for each voxel centroid, index (into the cropped cloud) of its
 *                 nearest point (needs GM_CFG_NEAREST)
 *   voxel normals: normals->at(kIndices[0]) of rvizNormals' marker loop
 *                 (src/tunnel_processing.cpp:237-249): the normal (nx,ny,nz,curvature) of that nearest
 *                 point, one row per voxel centroid, gathered on the device (needs GM_CFG_NEAREST) --
 *                 with the centroids this is everything /surfaceNormals needs, a few KB instead of
 *                 the whole normals cloud */
gm_status gm_get_cropped_xyz(gm_ctx *ctx, uint32_t slot, float *xyzw, uint32_t capacity, uint32_t *n_out);
gm_status gm_get_normals(gm_ctx *ctx, uint32_t slot, float *nxyzc, uint32_t capacity, uint32_t *n_out);
gm_status gm_get_voxel_centroids(gm_ctx *ctx, uint32_t slot, float *xyzc, uint32_t capacity, uint32_t *n_out);
gm_status gm_get_voxel_nearest(gm_ctx *ctx, uint32_t slot, int32_t *idx, uint32_t capacity, uint32_t *n_out);
gm_status gm_get_voxel_normals(gm_ctx *ctx, uint32_t slot, float *nxyzc, uint32_t capacity, uint32_t *n_out);
/* per-point neighbour counts of the cropped cloud, pre-compaction order (GM_CFG_KEEP_COUNTS) */
gm_status gm_get_neighbor_counts(gm_ctx *ctx, uint32_t slot, int32_t *counts, uint32_t capacity, uint32_t *n_out);
/* extension: per-point segment label of the valid cloud: 0 none, 1 plane, 2 cylinder */
gm_status gm_get_labels(gm_ctx *ctx, uint32_t slot, uint8_t *labels, uint32_t capacity, uint32_t *n_out);

/* ---- the reference's stage functions, one call each ------------------------ */
/* Host buffers in, host buffers out (blocking, slot 0).  These exist so the
 * four signatures of tunnel_processing.hpp can be re-implemented one-to-one. */

/* chopCloud(bound, cloud): tunnel_processing.hpp:38, src/tunnel_processing.cpp:39-49.
 * Order-preserving.  out rows x,y,z,pad(=input row index). */
gm_status gm_chop_cloud(gm_ctx *ctx, const gm_cloud *cloud, double bound,
                        float *xyzw_out, uint32_t capacity, uint32_t *n_out);

/* getNormals(radius, cloud&, kdtree&): tunnel_processing.hpp:41-45,
 * src/tunnel_processing.cpp:52-89.  xyz rows of 3 floats in; compacted cloud
 * (rows x,y,z,pad(=input row)) and normals (nx,ny,nz,curvature) out, same
 * length and order, NaN-normal rows removed. */
gm_status gm_get_normals_stage(gm_ctx *ctx, const float *xyz, uint32_t n, double radius,
                               float *xyzw_out, float *nxyzc_out, uint32_t capacity, uint32_t *n_out);

/* getLocalFrame(n, wf, normals, vals*&, vecs*&): tunnel_processing.hpp:48-54,
 * src/tunnel_processing.cpp:92-148.  eigenvectors column-major. */
gm_status gm_get_local_frame(gm_ctx *ctx, const float *nxyzc, uint32_t n, double weighting_factor,
                             float eigenvalues[3], float eigenvectors[9], double scatter6[6]);

/* The second half of getNormals alone (removeNaNNormalsFromPointCloud + ExtractIndices,
 * src/tunnel_processing.cpp:74-85) with getLocalFrame's scatter sums: n cloud rows (x,y,z,pad)
 * and n normal rows (nx,ny,nz,curvature) in; the rows whose normal has three finite
 * components out, same order, bit for bit, and the six scatter sums of the survivors
 * (scatter6 may be NULL). */
gm_status gm_compact_valid_stage(gm_ctx *ctx, const float *xyzw, const float *nxyzc, uint32_t n,
                                 double weighting_factor, float *xyzw_out, float *nxyzc_out,
                                 uint32_t capacity, uint32_t *n_out, double scatter6[6]);

/* The pcl::VoxelGrid half of rvizNormals: tunnel_processing.hpp:77-82,
 * src/tunnel_processing.cpp:214-220.  out rows x,y,z,count. */
gm_status gm_voxel_grid(gm_ctx *ctx, const float *xyz, uint32_t n, double leaf,
                        float *xyzc_out, uint32_t capacity, uint32_t *n_out, uint32_t *status_flags);

/* kdtree->nearestKSearch(q, 1): src/tunnel_processing.cpp:237-239. */
gm_status gm_nearest(gm_ctx *ctx, const float *xyz, uint32_t n, const float *queries, uint32_t nq,
                     int32_t *idx_out);

/* ---- multi-GPU merge unit (SURVEY.md par. 8e) ------------------------------- */

/* Eigen-solve a merged scatter matrix (sum over shards of gm_frame_result.scatter).
 * Pure host arithmetic on 6 doubles; same Jacobi as the device epilogue. */
gm_status gm_solve_local_frame(const double scatter6[6], float eigenvalues[3], float eigenvectors[9]);

/* Restrict which cropped points act as QUERY points: only points whose x lies in
 * [own_lo, own_hi) get a normal (the rest are halo: neighbours only, dropped
 * from the outputs).  Defaults to (-inf, +inf).  Used by slab sharding. */
gm_status gm_set_owned_range(gm_ctx *ctx, double own_lo, double own_hi);

/* ---- extensions without a reference counterpart (SURVEY.md par. 8a-ext) ----- */
/* getCylinder is an empty stub in the reference (src/tunnel_processing.cpp:149-154);
 * these follow PCL's SampleConsensusModelPlane / SampleConsensusModelCylinder
 * conventions and are checked against oracle/gm_oracle_ext.c + analytic truth only.
 * With GM_CFG_RANSAC_PLANE / _CYLINDER a frame additionally runs, on its valid cloud:
 * seeded hypotheses -> batched scoring (preemptive, three stages: all H hypotheses on
 * every 64th point, the 128 best of them on every 16th point, the 8 best of those on
 * every point; order = count descending, hypothesis index ascending; H <= 128 starts at
 * the second stage, H <= 8 is exhaustive) -> best model -> inlier labels (1 plane,
 * 2 cylinder; the cylinder samples and scores only points the plane left) ->
 * per-segment moments -> refits, reported in gm_frame_result. */

int gm_ext_available(void); /* 1 when the extension kernels are built in */

/* labels (may be NULL): only points with labels[i]==want take part / are sampled. */

/* Score caller-supplied hypotheses against a host cloud (xyz rows of 3 floats).
 * plane rows a,b,c,d: inlier iff |a x + b y + c z + d| < tau  (fp32, fma chain).
 * cylinder rows px,py,pz,dx,dy,dz,r: inlier iff (r-tau)^2 < dist_axis^2 < (r+tau)^2. */
gm_status gm_score_planes(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                          const float *hyp4, uint32_t H, double tau, int32_t *counts);
gm_status gm_score_cylinders(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                             const float *hyp7, uint32_t H, double tau, int32_t *counts);
/* Seeded minimal-sample hypotheses generated on the device (splitmix64 counter PRNG). */
/* Score caller-supplied hypotheses against the valid cloud a completed frame left in `slot` (no upload of points).
 * model 0: plane rows a,b,c,d; 1: cylinder rows px,py,pz,dx,dy,dz,r.  unlabelled_only != 0 counts only points the
 * frame's own RANSAC left unlabelled.  With gm_set_owned_range the valid cloud holds owned points only, so the counts
 * of the ranks of a sharded frame add up to the count on the whole frame: the building block of the multi-GPU
 * primitive vote (geometric_mapping_amd/sharding.py, DESIGN.md par. 6). */
gm_status gm_score_frame(gm_ctx *ctx, uint32_t slot, int model, const float *hyp, uint32_t H, double tau,
                         uint32_t unlabelled_only, int32_t *counts);
gm_status gm_plane_hypotheses(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                              uint64_t seed, uint32_t H, float *hyp4);
gm_status gm_cylinder_hypotheses(gm_ctx *ctx, const float *xyz, const float *nxyzc, uint32_t n,
                                 const uint8_t *labels, uint32_t want, uint64_t seed, uint32_t H, float *hyp7);
/* Per-segment moments over points with labels[i]==label (labels NULL: all points):
 * mom16 = count, sum p (3), sum pp^T (xx,xy,xz,yy,yz,zz), sum nn^T (same order); fp64. */
gm_status gm_segment_moments(gm_ctx *ctx, const float *xyz, const float *nxyzc, const uint8_t *labels,
                             uint32_t n, uint32_t label, double mom16[16]);

/* ---- cylinder regression (GM_CFG_CYLINDER_FIT) -------------------------------------------------------------------
 * The reference's getCylinder is declared (include/geometric_mapping/tunnel_processing.hpp:56-59) with an empty body
 * under "//Regression function" (src/tunnel_processing.cpp:149-154); its cylinderPub / displayCylinder exist only to
 * publish that regression.  This is that regression, run on the device after the cylinder RANSAC:
 *   parameters  unit axis direction d, axis point c, radius r; residual of p: |(p-c) - ((p-c).d) d| - r.
 *   start       the frame's winning hypothesis row (gm_frame_result.cylinder), as published.
 *   points      those the plane did not take (label 0 or 2 after the RANSAC label passes).
 *   3 passes    Gauss-Newton, gates 4 tau, 2 tau, tau (tau = ransac_threshold): the points with |residual| < gate sum
 *               J^T J, J^T res, sum res^2, count and sum t = (p-c).d in fp64; J is taken in a frame e1, e2 perpendicular
 *               to d over (shift of c along e1, e2; tilt of d along e1, e2; r); c is moved to the foot of the gated
 *               points' mean t before each update; the 5x5 system is solved by fp64 Cholesky.
 *   label pass  at tau with the fp32 row `model` (point, unit direction, radius) and the RANSAC's own inlier predicate:
 *               label 2 = inlier of the fitted cylinder, former label-2 points outside go back to 0, label 1 untouched.
 *   point       the foot on the axis of the final inliers' centroid; axis sign: positive dot with the hypothesis axis.
 * On failure (no hypothesis, fewer than 5 gated points, a singular / non-positive pivot) the parameters are NaN and the
 * labels stay those of the RANSAC.  A last step above GM_FIT_STEP_BOUND sets GM_FIT_NOT_CONVERGED; values are kept. */
#define GM_FIT_OK            0u         /* fitted */
#define GM_FIT_NO_MODEL      1u         /* no cylinder hypothesis to start from */
#define GM_FIT_DEGENERATE    2u         /* fewer than 5 points inside a pass's gate */
#define GM_FIT_SINGULAR      3u         /* the 5x5 normal matrix has a non-positive (or non-finite) Cholesky pivot */
#define GM_FIT_FAILED_MASK   0xFFu      /* status & mask != 0: parameters are NaN */
#define GM_FIT_NOT_CONVERGED (1u << 8)  /* last_step > GM_FIT_STEP_BOUND (the parameters are still published) */
#define GM_FIT_STEP_BOUND    1e-2       /* Euclidean norm of the last 5-vector step (metres and radians): a third of tau */

typedef struct gm_cylinder_fit {
    uint32_t struct_size; /* = sizeof(gm_cylinder_fit), filled by the library */
    uint32_t status;      /* GM_FIT_* */
    uint32_t inliers;     /* points labelled 2 by the final pass (points with inlier_out = 1 for gm_fit_cylinder) */
    uint32_t passes;      /* Gauss-Newton passes completed (3 on success) */
    double   point[3];    /* foot on the axis of the final inliers' centroid */
    double   axis[3];     /* unit axis direction, positive dot with the hypothesis axis */
    double   radius;      /* metres */
    double   rms;         /* root mean square residual of the final inliers against `model` */
    double   last_step;   /* Euclidean norm of the last Gauss-Newton step (c shift, d tilt, r) */
    float    model[7];    /* fp32 row the final labels were decided with: point on axis, unit direction, radius */
} gm_cylinder_fit;

/* The fit of a completed slot (GM_ERR_UNSUPPORTED for a context created without GM_CFG_CYLINDER_FIT).  For a group's
 * streamed frame: gm_get_cylinder_fit(gm_group_ctx(grp, rank), slot, ...).  A sharded group frame fits through the
 * stage call gm_group_fit_cylinder (the flag itself stays refused by gm_group_process_frame). */
gm_status gm_get_cylinder_fit(gm_ctx *ctx, uint32_t slot, gm_cylinder_fit *out);
/* getCylinder as one stage call (host buffers, blocking, slot 0; the frame's kernels).  xyz rows of 3 floats; the points
 * with labels[i] == want take part (all points when labels is NULL); init7 = starting row (point, direction, radius);
 * tau > 0.  inlier_out (may be NULL, n bytes) receives 1 for the final inliers, 0 elsewhere.  Fed a frame's valid cloud,
 * its labels with 2 -> 0, want = 0 and init7 = gm_frame_result.cylinder, it returns that frame's fit bit for bit. */
gm_status gm_fit_cylinder(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, uint32_t want,
                          const float init7[7], double tau, gm_cylinder_fit *out, uint8_t *inlier_out);

/* ---- wall deviation map (GM_CFG_SURFACE_MAP) ---------------------------------------------------------------------
 * A developed ("unrolled") map of the wall against the fitted cylinder: one cell per axial station and angular sector,
 * holding the signed radial deviation of the points that fall into it.  Run on the device right after the cylinder
 * regression of every frame, on the valid cloud (order of gm_get_cropped_xyz), the labels after the fit's relabel and
 * the fit's fp32 row fit.model = (c, d, R).
 *   map frame   computed once per frame in fp64 from the fp32 row, rounded to fp32 once, reported in gm_surface_info:
 *               a = d if d.forward >= 0, else -d;  o = c - (c.a) a (the foot of the sensor origin: t = 0 there);
 *               u = normalize(up - (up.a) a), or, when that projection is shorter than 0.1 |up|, the e1 of the fit's
 *               basis of a (GM_SURF_UP_FALLBACK);  v = a x u.
 *   per point   fp32, explicit roundings: q = p - o, t = q.a, w = q - t a, e = sqrt(w.w) - R (positive: the wall lies
 *               outside the cylinder), theta = atan2(w.v, w.u) folded to phi in [0, 2 pi) (0 toward up, increasing toward
 *               v), j = floor((t - t_min) / ds), k = min(floor(phi / dtheta), n_sectors - 1), dtheta = 2 pi / n_sectors.
 *   classes     every valid point is in exactly one: plane (label 1), beyond_gate (|e| > gate or e not finite), outside
 *               (j not in [0, n_stations)), mapped (cell j * n_sectors + k).
 *   cells       count; mean = (sum of rint(e 2^20), int64) 2^-20 / count in fp64, rounded to fp32 once; min e, max e (the
 *               exact fp32 residuals).  An empty cell: count 0, NaN elsewhere.  Every cell is a function of the set of
 *               (cell, e) pairs alone -- not of arrival order, grid or launch site -- so the frame, a replayed graph,
 *               streaming slots and the stage call give the same bytes.  No floating-point atomics.
 *   points      e (NaN for plane points) and the cell index (-1 unless mapped).
 * A failed fit (status & GM_FIT_FAILED_MASK) or a row that is not finite gives GM_SURF_NO_MODEL: every cell empty, every
 * residual NaN, every cell index -1, the class counts 0 and the frame vectors NaN. */
#define GM_SURF_MAX_CELLS   4096u      /* n_stations * n_sectors limit: a map block's LDS table, 20 B per cell = 80 KiB */
#define GM_SURF_OK          0u
#define GM_SURF_NO_MODEL    1u         /* no fitted cylinder: nothing mapped */
#define GM_SURF_UP_FALLBACK (1u << 8)  /* `up` is (nearly) parallel to the axis: u is the fit basis' e1 instead */

typedef struct gm_surface_params {
    uint32_t struct_size;     /* = sizeof(gm_surface_params) */
    uint32_t n_stations;      /* axial stations, >= 1 (default 40) */
    uint32_t n_sectors;       /* angular sectors, >= 1 (default 90: 4 degrees); n_stations * n_sectors <= GM_SURF_MAX_CELLS */
    uint32_t reserved;        /* 0 */
    double   station_length;  /* ds, metres, > 0 (default 0.25) */
    double   t_min;           /* axial coordinate of station 0's start, metres, finite (default -5: the default crop box) */
    double   gate;            /* |e| above it is beyond_gate, metres, in (0, 8] (default 0.25) */
    double   up[3];           /* sector 0 direction before projection, finite, non-zero (default 0, 0, 1) */
    double   forward[3];      /* station direction sign, finite, non-zero (default 1, 0, 0: REP-103 x forward) */
} gm_surface_params;

typedef struct gm_surface_cell {
    uint32_t count;
    float    mean, min, max;  /* metres; NaN when count == 0 */
} gm_surface_cell;

typedef struct gm_surface_info {
    uint32_t struct_size;     /* = sizeof(gm_surface_info), filled by the library */
    uint32_t status;          /* GM_SURF_* */
    uint32_t n_stations, n_sectors;
    uint32_t mapped, outside, beyond_gate, plane;   /* points per class; they add up to n_valid (0 on GM_SURF_NO_MODEL) */
    uint32_t cells_hit;       /* cells with count > 0 */
    uint32_t reserved;
    float    o[3], a[3], u[3], v[3];                /* the map frame (fp32, as the points were binned with) */
    float    R;               /* fit.model radius */
    float    t_min, station_length, sector_angle;   /* fp32 binning constants: t_min, ds, dtheta = 2 pi / n_sectors */
} gm_surface_info;

/* Host only: the defaults of the table above. */
void gm_surface_default_params(gm_surface_params *p);
/* Map parameters of the frames submitted after the call (every slot; a captured graph reads them from the device).
 * GM_ERR_NOT_READY while any slot holds a submitted frame that has not been waited for; GM_ERR_INVALID_ARG outside the
 * limits.  Works on any context (the stage call takes its own parameters). */
gm_status gm_set_surface_params(gm_ctx *ctx, const gm_surface_params *p);
/* The map of a completed slot (GM_ERR_UNSUPPORTED for a context created without GM_CFG_SURFACE_MAP).  info is required;
 * cells (row-major [n_stations][n_sectors]) may be NULL with capacity 0: *n_out = n_stations * n_sectors, and a short
 * buffer returns GM_ERR_CAPACITY (info is filled either way).  For a group's streamed frame: the rank's context. */
gm_status gm_get_surface_map(gm_ctx *ctx, uint32_t slot, gm_surface_info *info, gm_surface_cell *cells, uint32_t capacity,
                             uint32_t *n_out);
/* Per valid point of a completed slot: residual e and cell index (either pointer may be NULL); *n_out = n_valid. */
gm_status gm_get_surface_points(gm_ctx *ctx, uint32_t slot, float *residual, int32_t *cell, uint32_t capacity,
                                uint32_t *n_out);
/* The map as one stage call (host buffers, blocking, slot 0; the frame's kernel).  xyz rows of 3 floats; labels (may be
 * NULL: no point is plane); model7 = (c, d, R) as gm_cylinder_fit.model (a non-finite row gives GM_SURF_NO_MODEL);
 * p (NULL: defaults).  cells needs n_stations * n_sectors records (GM_ERR_CAPACITY otherwise); residual / cell (may be
 * NULL) n entries.  Works on any context.  Fed a frame's valid cloud, labels and fit.model with the frame's
 * parameters, it returns that frame's map bit for bit. */
gm_status gm_surface_map(gm_ctx *ctx, const float *xyz, uint32_t n, const uint8_t *labels, const float model7[7],
                         const gm_surface_params *p, gm_surface_info *info, gm_surface_cell *cells, uint32_t capacity,
                         float *residual, int32_t *cell);

/* ---- persistent wall map (gm_wall_*) ------------------------------------------------------------------------------
 * A device-resident developed map of the wall against a DESIGN cylinder, by chainage: n_stations stations of
 * station_length metres from t_min along the design axis, n_sectors sectors around it.  It outlives frames: every add
 * bins the valid cloud of one frame, taken under a caller-supplied pose (sensor -> map), into the same table.  A cell
 * holds integer accumulators only -- count (u32), sum of rint(e 2^20) (int64), min_key = ~ordered(min e) and
 * max_key = ordered(max e) (u32, updated with an integer maximum; 0 = empty), where for the fp32 residual e with bits b
 *     ordered(e) = b ^ 0x80000000 if the sign bit of b is clear, else ~b        (monotone in e; never 0 for a finite e)
 * -- so a cell is a function of the multiset of (cell, e) pairs alone: adds in any order, from slots running
 * concurrently, or merged from other maps / devices / files (gm_wall_map_add_raw) give the same bytes.
 *   design frame  once at creation, fp64, NOT rounded: d = direction / |direction|; a = d if d.forward >= 0, else -d;
 *                 o = point - (point.a) a;  u = normalize(up - (up.a) a), or, when that projection is shorter than
 *                 0.1 |up|, the e1 of the fit basis of a (GM_SURF_UP_FALLBACK in status): e1 = (h x a) / |h x a| with
 *                 h = (0,0,1) if |a_z| < 0.9, else (0,1,0);  v = a x u;  R = radius.
 *   per add       host, fp64.  pose = row-major 3x4 [Rm | tr], sensor -> map (p_map = Rm p + tr); every entry finite,
 *                 max |Rm^T Rm - I| <= 1e-6 and det Rm > 0, else GM_ERR_INVALID_ARG.  Sensor chainage s = (tr - o).a;
 *                 anchor station j_f = floor((s - t_min) / ds) (|.| < 2^62, else GM_ERR_INVALID_ARG); frame-local
 *                 origin o_f = o + (t_min + j_f ds) a.  In sensor coordinates o' = Rm^T (o_f - tr), a' = Rm^T a,
 *                 u' = Rm^T u, v' = Rm^T v, each rounded to fp32 once; R, ds, gate and dtheta = 2 pi / n_sectors
 *                 rounded to fp32 once.  All of it is reported in gm_wall_add_info.  The device therefore only sees
 *                 coordinates of the size of the crop box: a frame at chainage 5 km is binned like one at 0.
 *   per point     device, fp32, the per-point chain of the GM_CFG_SURFACE_MAP block above with (o', a', u', v', R) and
 *                 a local t_min of 0: q = p - o', t = q.a', w = q - t a', e = sqrt(w.w) - R, phi, k as stated there;
 *                 the station is j = j_f + floor(t / ds), taken in 64-bit integers.
 *   classes       every point is in exactly one: plane (label 1), beyond_gate (|e| > gate or e not finite), outside
 *                 (j not in [0, n_stations)), mapped (cell j * n_sectors + k).
 *   read          gm_surface_cell records by the rule of the block above: mean = sum 2^-20 / count in fp64 rounded to
 *                 fp32 once, min = ordered^-1(~min_key), max = ordered^-1(max_key); count 0 and NaN when empty.
 * A map belongs to the context it was created from (several per context are allowed) and is freed with it. */
#define GM_WALL_MAX_CELLS   (1u << 24)   /* n_stations * n_sectors limit (20 B of device memory per cell) */
#define GM_WALL_MAX_SECTORS 4096u

typedef struct gm_wall_map gm_wall_map;   /* opaque; owned by the context it was created from */

typedef struct gm_wall_params {
    uint32_t struct_size;     /* = sizeof(gm_wall_params) */
    uint32_t n_stations;      /* >= 1 (default 4000: 1 km at the default station_length) */
    uint32_t n_sectors;       /* 1 .. 4096 (default 90); n_stations * n_sectors <= GM_WALL_MAX_CELLS */
    uint32_t reserved;        /* 0 */
    double   station_length;  /* ds, metres, > 0 (default 0.25) */
    double   t_min;           /* chainage of station 0's start, metres, finite (default 0) */
    double   gate;            /* |e| above it is beyond_gate, metres, in (0, 8] (default 0.25) */
    double   point[3];        /* the design cylinder in map coordinates: a point of the axis (default 0, 0, 0), */
    double   direction[3];    /*   its direction, non-zero (default 1, 0, 0), */
    double   radius;          /*   its radius, > 0 (default 2) */
    double   up[3];           /* as gm_surface_params (default 0, 0, 1) */
    double   forward[3];      /* as gm_surface_params (default 1, 0, 0) */
} gm_wall_params;

typedef struct gm_wall_raw_cell {   /* 24 bytes; the encoding stated above is fixed: files of raw cells stay readable */
    int64_t  sum;             /* sum of rint(e 2^20) */
    uint32_t count;
    uint32_t min_key;         /* ~ordered(min e); 0 when empty */
    uint32_t max_key;         /* ordered(max e); 0 when empty */
    uint32_t reserved;        /* 0 */
} gm_wall_raw_cell;

typedef struct gm_wall_add_info {     /* filled on the host by every add, before the kernel has run */
    uint32_t struct_size;     /* = sizeof(gm_wall_add_info), filled by the library */
    uint32_t status;          /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the design frame's */
    int64_t  anchor_station;  /* j_f */
    float    o[3], a[3], u[3], v[3];   /* o', a', u', v': the frame-local map frame in SENSOR coordinates (fp32, as binned with) */
    float    R, station_length, sector_angle, gate;   /* fp32 binning constants */
} gm_wall_add_info;

typedef struct gm_wall_info {         /* cumulative; read after a synchronisation */
    uint32_t struct_size;     /* = sizeof(gm_wall_info), filled by the library */
    uint32_t status;          /* GM_SURF_OK or GM_SURF_UP_FALLBACK */
    uint32_t n_stations, n_sectors;
    uint64_t frames;          /* adds since create / the last full clear */
    uint64_t mapped, outside, beyond_gate, plane;   /* points per class over those adds: points added as points only
                                                       (gm_wall_map_add_raw changes cells and cells_hit, not these) */
    uint64_t cells_hit;       /* cells with count > 0 in the whole map */
    double   o[3], a[3], u[3], v[3], R;             /* the design frame in map coordinates (fp64) */
} gm_wall_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_default_params(gm_wall_params *p);
/* A zeroed map on ctx's device.  GM_ERR_INVALID_ARG: NULL, struct_size mismatch or a parameter outside its limits;
 * GM_ERR_OOM: the table does not fit; GM_ERR_DEVICE. */
gm_status gm_wall_map_create(gm_ctx *ctx, const gm_wall_params *params, gm_wall_map **map);
/* Waits for the map's adds and frees it (gm_destroy of the owning context frees the maps still alive).  NULL is ignored. */
void gm_wall_map_destroy(gm_wall_map *map);
/* Adds the valid cloud of the frame last submitted to `slot` of ctx (which must be the map's own context:
 * GM_ERR_INVALID_ARG otherwise, as for a bad slot or pose or a NULL).  The add is enqueued on the slot's stream behind the
 * frame's work and the call returns without waiting: it may follow gm_submit_frame directly or come after
 * gm_wait_frame.  It reads the point count and the slot's final labels (those of gm_get_labels; no point is plane on a
 * context without GM_CFG_RANSAC_PLANE) on the device and writes nothing per point.  A later submit to the slot is ordered
 * behind it; adds from different slots may run concurrently into one map.  With GM_CFG_GRAPH it is a plain launch after
 * the graph.  GM_ERR_NOT_READY: the slot holds no frame (never submitted, or reused by a stage call since).  add_info
 * may be NULL. */
gm_status gm_wall_map_add_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12], gm_wall_add_info *add_info);
/* The same kernel as one blocking stage call on host buffers (slot 0 of the map's context, refused with GM_ERR_NOT_READY
 * while that slot holds a frame not waited for).  xyz rows of 3 floats; labels (may be NULL: no point is plane);
 * residual (float[n]: e, NaN for plane points) and cell (int32_t[n]: j * n_sectors + k, -1 unless mapped) may be NULL.
 * Fed the xyz of a slot's gm_get_cropped_xyz rows and its gm_get_labels with the same pose, it changes the map exactly
 * as gm_wall_map_add_frame does.  GM_ERR_INVALID_ARG: NULL map / xyz with n > 0, bad pose. */
gm_status gm_wall_map_add_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                 gm_wall_add_info *add_info, float *residual, int32_t *cell);
/* Waits for every add enqueued so far. */
gm_status gm_wall_map_sync(gm_wall_map *map);
/* The five calls below synchronise first (as gm_wall_map_sync), run a small device kernel and block.  A window is
 * stations [station0, station0 + n); one outside [0, n_stations] is GM_ERR_INVALID_ARG.  Cell buffers are row-major
 * [n][n_sectors]; *n_out (may be NULL) = n * n_sectors, and a smaller capacity (in cells) returns GM_ERR_CAPACITY. */
gm_status gm_wall_map_info(gm_wall_map *map, gm_wall_info *info);
gm_status gm_wall_map_read(gm_wall_map *map, uint32_t station0, uint32_t n, gm_surface_cell *cells, uint64_t capacity,
                           uint64_t *n_out);
gm_status gm_wall_map_read_raw(gm_wall_map *map, uint32_t station0, uint32_t n, gm_wall_raw_cell *cells, uint64_t capacity,
                               uint64_t *n_out);
/* Merges n stations of raw cells ([n][n_sectors]) into the window: counts and sums add, keys take the maximum.  This is
 * how a map is restored from a file and how the maps of several devices or sessions become one.  It changes cells and
 * cells_hit only: the per-class totals and `frames` count points added as points. */
gm_status gm_wall_map_add_raw(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_raw_cell *cells);
/* Zeroes the window; clearing the whole range [0, n_stations) also zeroes the cumulative totals and `frames`. */
gm_status gm_wall_map_clear(gm_wall_map *map, uint32_t station0, uint32_t n);

/* ---- connected deviation regions of the wall map (gm_wall_map_regions) ----------------------------------------------
 * Where the wall departs from the design, or from an earlier survey (a second map, the BASELINE), as a short list.  The
 * rule is integer throughout, so the result is a function of the raw cells alone:
 *   value       q = sum / (int64) count by C integer division (toward zero), units of 2^-20 m.  Without a baseline
 *               d = q and the cell is USABLE iff count >= min_count; with one d = q(map) - q(baseline), usable iff both
 *               counts are >= min_count.
 *   threshold   T = (int64) rint(threshold 2^20), fp64, once on the host; threshold in (0, 8] and T >= 1.
 *   sign        +1 if usable and d >= T, -1 if usable and d <= -T, else 0 (not flagged).
 *   window      stations [station0, station0 + n); cells outside it do not exist for the call.
 *   neighbours  of (j, k), connectivity 4: (j +- 1, k) inside the window and (j, (k +- 1) mod n_sectors); connectivity
 *               8: also (j +- 1, (k +- 1) mod n_sectors).  The sector index wraps, the station index does not.
 *   component   a maximal set of cells connected through neighbours of the same non-zero sign.  Its LABEL is the
 *               smallest map-wide cell index j * n_sectors + k in it.  A REGION is a component of >= min_cells cells.
 *   classes     every window cell is flagged_pos, flagged_neg, EMPTY (count 0 in the map and, with a baseline, in the
 *               baseline too), UNUSABLE (not empty, not usable) or usable and below the threshold (not counted).
 *   peak        the cell of the largest |d|, the smallest index among equals (|d| compares saturated at 2^32 - 1 units,
 *               4096 m: far beyond any gate).
 * Labelling (a union-find over tiles and their seams), the per-region reduction and the min_cells filter run on the
 * device in a fixed number of launches; only info, the region list and, when asked for, cell_labels leave it.  The
 * result does not depend on the tile shape (environment GM_WALL_REGION_TILE=<stations>x<sectors>, product <= 4096, read
 * at gm_wall_map_create: tests and measurements), the grid or the order blocks run in. */
#define GM_WALL_REGION_TILE_STATIONS 64u   /* the default tile of the labelling kernel */
#define GM_WALL_REGION_TILE_SECTORS  64u

typedef struct gm_wall_region {     /* 64 bytes; every field is independent of the order cells were visited in */
    uint32_t label;                 /* smallest cell index of the region: its identity */
    int32_t  sign;                  /* +1 wall outside (overbreak / moved out), -1 inside (intrusion / moved in) */
    uint32_t cells;
    uint32_t station_min, station_max;             /* inclusive */
    uint32_t sector_min, sector_max;               /* over k */
    uint32_t sector_min_turned, sector_max_turned; /* over (k + n_sectors / 2) mod n_sectors: contiguous for a region across the seam */
    uint32_t peak_cell;             /* cell of the largest |d|; the smallest index among equals */
    int64_t  peak;                  /* its d, 2^-20 m */
    int64_t  sum_d;                 /* sum of d over the cells, 2^-20 m (times the cell area: volume) */
    uint64_t points;                /* sum of the map's counts (not the baseline's) */
} gm_wall_region;

typedef struct gm_wall_region_params {
    uint32_t struct_size;     /* = sizeof(gm_wall_region_params) */
    uint32_t min_count;       /* >= 1 (default 8): points a cell needs to be usable */
    uint32_t min_cells;       /* >= 1 (default 4): cells a component needs to be a region */
    uint32_t connectivity;    /* 4 or 8 (default 8) */
    double   threshold;       /* metres, in (0, 8] with rint(threshold 2^20) >= 1 (default 0.05) */
    uint64_t reserved;        /* 0 */
} gm_wall_region_params;

typedef struct gm_wall_regions_info {
    uint32_t struct_size;     /* = sizeof(gm_wall_regions_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;   /* the window and the map's sectors */
    int64_t  threshold_q;     /* T */
    uint64_t flagged_pos, flagged_neg, unusable, empty;   /* window cells per class (stated above) */
    uint64_t components;      /* before the min_cells filter */
    uint64_t regions;         /* after it */
    double   cell_area;       /* station_length * radius * 2 pi / n_sectors (the design radius), m^2 */
} gm_wall_regions_info;

/* (a struct tag only, no typedef: the function of the same name below fills it) */
struct gm_wall_region_metrics {   /* fp64, derived on the host from one record and the map's parameters */
    double area_m2;           /* cells * cell_area */
    double volume_m3;         /* sum_d 2^-20 * cell_area */
    double peak_m;            /* peak 2^-20 */
    double mean_m;            /* sum_d 2^-20 / cells */
    double chainage_from;     /* t_min + station_min * station_length */
    double chainage_to;       /* t_min + (station_max + 1) * station_length */
    double angle_from_deg;    /* 360 k / n_sectors at the first sector's start and the last sector's end, from whichever */
    double angle_to_deg;      /*   of the plain and the turned sector extent is shorter (plain on a tie); a turned extent
                                   is turned back, both in [0, 360] and from > to meaning "across 0"; a region on every
                                   sector gives 0 and 360 */
};

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_region_default_params(gm_wall_region_params *p);
/* The regions of the window, ascending by label.  Synchronises both maps (as gm_wall_map_sync), runs on the device and
 * blocks.  baseline (may be NULL) is an earlier epoch: another map of the same context whose n_stations, n_sectors,
 * station_length, t_min, point, direction, radius, up and forward equal the map's bit for bit (gate may differ).  prm
 * NULL: the defaults.  info and *n_out (n_out may be NULL) are filled whenever the call got as far as the device, also on
 * GM_ERR_CAPACITY: *n_out is the number of regions.  regions NULL with capacity 0 is a count query (GM_OK); fewer than
 * *n_out records of capacity returns GM_ERR_CAPACITY and writes no record.  cell_labels (may be NULL; [n][n_sectors])
 * receives the region's label for every cell of a region and -1 for every other cell (unflagged, or in a component
 * below min_cells).  n = 0 gives no regions.  The maps are not changed.  Scratch (16 B per window cell and 128 B per
 * component) is allocated on first use, kept grow-only in the map and freed with it.
 * GM_ERR_INVALID_ARG: NULL map / info, a window outside the map, a parameter outside its limits or a struct_size
 * mismatch, regions NULL with capacity > 0, baseline == map, of another context or on another grid. */
gm_status gm_wall_map_regions(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n,
                              const gm_wall_region_params *prm, gm_wall_regions_info *info, gm_wall_region *regions,
                              uint32_t capacity, uint32_t *n_out, int32_t *cell_labels);
/* Host only, no device, no map: the fp64 derivation stated at gm_wall_region_metrics from the map's parameters.
 * GM_ERR_INVALID_ARG: a NULL, p->struct_size mismatch, n_sectors 0, r->cells 0 or a sector extent outside n_sectors. */
gm_status gm_wall_region_metrics(const gm_wall_params *p, const gm_wall_region *r, struct gm_wall_region_metrics *out);

/* ---- the wall map as an ordered, decimated point list (gm_wall_map_cloud) --------------------------------------------
 * The surveyed wall as a cloud: one point per BLOCK of cells that holds enough points, sitting on the design cylinder
 * displaced by the block's mean deviation, in block order.  Blocks are merged in integers, so a block is a function of
 * the raw cells alone, and only the surviving records leave the device.
 *   blocks      the window is stations [station0, station0 + n); NJ = ceil(n / bs), NK = ceil(n_sectors / bk).  Block
 *               (J, K) covers stations j0 = station0 + J bs .. j0 + ns_J - 1, ns_J = min(bs, station0 + n - j0), and
 *               sectors K bk .. K bk + nk_K - 1, nk_K = min(bk, n_sectors - K bk): the last blocks are ragged, nothing
 *               wraps, and bs > n or bk > n_sectors is one block in that direction.
 *   merge       count = u64 sum of the cells' counts, sum = int64 sum of their sums, min_key and max_key = the maxima of
 *               their keys, cells = the number of cells with count > 0.
 *   classes     every block is exactly one of EMPTY (count 0), BELOW_MIN_COUNT (0 < count < min_count) or a POINT.
 *   record      m = (double) sum 2^-20 / (double) count (conversions round to nearest); mean = (float) m;
 *               min = ordered^-1(~min_key), max = ordered^-1(max_key), as gm_wall_map_read does for one cell.
 *   directions  host, once per call: phi_K = (2 pi) ((double)(2 K bk + nk_K) / (double)(2 n_sectors)), c_K = cos phi_K,
 *               s_K = sin phi_K by the host's libm (phi is 0 toward u and grows toward v, as in the binning).  The
 *               table (NK <= 4096 pairs) is uploaded: the device calls no fp64 trigonometric function, and
 *               gm_wall_cloud_directions returns exactly the table the call uses.
 *   position    fp64 on the map's unrounded design frame (o, a, u, v, R), t_min and ds = station_length; every
 *               operation rounded once, none contracted, in this order:
 *                   h = (double)(2 j0 + ns_J) 0.5,  t_c = t_min + h ds,  rho = R + g m,  w_i = c_K u_i + s_K v_i,
 *                   p_i = ((o_i - anchor_i) + t_c a_i) + rho w_i,  x, y, z = (float) p_i
 *               with g = exaggeration.  A map coordinate at chainage 5 km has 0.5 mm of fp32 resolution: a host sets
 *               the anchor near the window and publishes with that offset in the frame transform.
 *   order       ascending by block = J NK + K.
 * On the device a window is processed in chunks of whole block rows of at most 2^20 blocks (environment
 * GM_WALL_CLOUD_CHUNK=<blocks>, rounded down to whole block rows, at least one row, a value above 2^20 meaning 2^20, read
 * at gm_wall_map_create: tests and measurements); the trip count depends on the window, never on the data, and the result does not depend on it. */
typedef struct gm_wall_cloud_params {
    uint32_t struct_size;      /* = sizeof(gm_wall_cloud_params) */
    uint32_t block_stations;   /* bs >= 1 (default 1) */
    uint32_t block_sectors;    /* bk >= 1 (default 1) */
    uint32_t min_count;        /* >= 1 (default 1): merged points a block needs to become a point */
    double   exaggeration;     /* g, finite, >= 0 (default 1): the point sits at radius R + g * mean */
    double   anchor[3];        /* finite (default 0, 0, 0): subtracted in fp64 before the one rounding to fp32 */
    uint64_t reserved;         /* 0 */
} gm_wall_cloud_params;

typedef struct gm_wall_cloud_point {   /* 40 bytes: a PointCloud2 row, x y z FLOAT32 at 0, 4, 8 */
    float    x, y, z;          /* map coordinates minus anchor */
    float    mean, min, max;   /* gm_wall_map_read's rule applied to the merged accumulators */
    uint32_t block;            /* J * NK + K */
    uint32_t cells;            /* non-empty source cells merged */
    uint64_t count;            /* merged points */
} gm_wall_cloud_point;

typedef struct gm_wall_cloud_info {
    uint32_t struct_size;      /* = sizeof(gm_wall_cloud_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;     /* the window and the map's sectors */
    uint32_t blocks_stations, blocks_sectors;     /* NJ, NK */
    uint64_t blocks, points, below_min_count, empty;   /* blocks = points + below_min_count + empty */
} gm_wall_cloud_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_cloud_default_params(gm_wall_cloud_params *p);
/* Host only, no device, no map: the NK (cos, sin) pairs of the rule above for p->n_sectors and c->block_sectors (c NULL:
 * the defaults), cos_sin[2 K] = c_K, cos_sin[2 K + 1] = s_K.  *n_out (may be NULL) = NK; a capacity (in pairs) below NK
 * returns GM_ERR_CAPACITY and writes nothing.  GM_ERR_INVALID_ARG: p NULL, a struct_size mismatch, n_sectors outside
 * 1 .. GM_WALL_MAX_SECTORS, block_sectors 0, cos_sin NULL with capacity > 0. */
gm_status gm_wall_cloud_directions(const gm_wall_params *p, const gm_wall_cloud_params *c, double *cos_sin, uint32_t capacity,
                                   uint32_t *n_out);
/* The points of the window, ascending by block.  Synchronises the map (as gm_wall_map_sync), runs on the map's stream and
 * blocks.  prm NULL: the defaults.  info is required; it and *n_out (may be NULL; the number of points) are filled
 * whenever the call got as far as the device, also on GM_ERR_CAPACITY.  points NULL with capacity 0 is a count query
 * (GM_OK); a capacity below *n_out returns GM_ERR_CAPACITY and leaves the contents of points unspecified (copying stops,
 * counting goes on).  n = 0 gives no points.  The map is not changed.  Scratch (28 B per block of a chunk unless
 * bs = bk = 1, 40 B per block of a chunk of staging, the chained scan's own records, the direction table) is allocated
 * on first use, kept grow-only in the map and freed with it; a map that never calls this allocates nothing.
 * GM_ERR_INVALID_ARG: NULL map / info, a window outside the map, a struct_size mismatch, a parameter outside its limits,
 * points NULL with capacity > 0. */
gm_status gm_wall_map_cloud(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_cloud_params *prm,
                            gm_wall_cloud_info *info, gm_wall_cloud_point *points, uint64_t capacity, uint64_t *n_out);

/* ---- the wall map as an indexed triangle mesh (gm_wall_map_mesh) ------------------------------------------------------
 * The cloud above with faces: a surface a viewer can shade and section, a TRIANGLE_LIST marker or a shape_msgs/Mesh.
 *   vertices    exactly the rows gm_wall_map_cloud returns for the same map, window and gm_wall_cloud_params: the same
 *               records in the same block order with the same bytes.  The index of a vertex is its position in that list.
 *   quads       NJ, NK are the cloud's block counts; block (J, K) is ALIVE when it became a point.  The sectors close the
 *               tube (wrapped = 1) when NK >= 3 and GM_WALL_MESH_NO_WRAP is not set: then NKq = NK, else NKq = NK - 1.
 *               There are (NJ - 1) NKq quads (none when NJ = 1 or NKq = 0: vertices without triangles), quad
 *               Q = J NKq + K with the corners, in cyclic order, A = (J, K), B = (J + 1, K), C = (J + 1, K'), D = (J, K'),
 *               K' = (K + 1) mod NK.
 *   triangles   four alive corners: (A, B, C) in slot 2 Q and (A, C, D) in slot 2 Q + 1 (quads_two).  Three alive
 *               corners: the one triangle of the alive corners in the cyclic order above with the dead corner left out, in
 *               slot 2 Q (quads_one).  Fewer: nothing (quads_none).  With the cloud's block order (phi grows from u toward
 *               v, v = a x u) the normal (v1 - v0) x (v2 - v0) faces the axis: the viewer stands in the tunnel.
 *               GM_WALL_MESH_OUTWARD swaps the second and the third index of every triangle.
 *   step cut    max_step > 0: a triangle is dropped (cut_by_step) when for any two of its corners
 *               fabsf(mean_a - mean_b) > (float) max_step, mean the fp32 field of the vertex row, the subtraction one fp32
 *               operation: a niche or an installation grows no skirts to the wall around it.  0: no cut.  The cut is
 *               applied per triangle, after the corner rule: a quad may keep one of its two.
 *   order       ascending by slot.
 * quads = quads_two + quads_one + quads_none and triangles = 2 quads_two + quads_one - cut_by_step, always.  The result is a
 * function of the raw cells and the parameters alone.  On the device the vertex pass is the cloud's, chunked as the cloud
 * is (GM_WALL_CLOUD_CHUNK), and stores every survivor's index into a table of one uint32 per block of the window; the
 * triangle pass follows in chunks of as many whole quad rows. */
#define GM_WALL_MESH_OUTWARD (1u << 0)
#define GM_WALL_MESH_NO_WRAP (1u << 1)

typedef struct gm_wall_mesh_params {
    uint32_t struct_size;      /* = sizeof(gm_wall_mesh_params) */
    uint32_t flags;            /* GM_WALL_MESH_* (default 0) */
    gm_wall_cloud_params cloud;   /* the vertices' parameters (its own struct_size set) */
    double   max_step;         /* finite, >= 0 (default 0: no cut), metres of mean deviation */
    uint64_t reserved;         /* 0 */
} gm_wall_mesh_params;

typedef struct gm_wall_mesh_triangle {   /* 12 bytes */
    uint32_t v[3];             /* indices into the vertex list */
} gm_wall_mesh_triangle;

typedef struct gm_wall_mesh_info {
    uint32_t struct_size;      /* = sizeof(gm_wall_mesh_info), filled by the library */
    uint32_t wrapped;          /* 0 or 1 */
    gm_wall_cloud_info cloud;  /* the vertices: what gm_wall_map_cloud reports */
    uint64_t quads, quads_two, quads_one, quads_none;   /* by the corner rule, before the step cut */
    uint64_t cut_by_step, triangles;
} gm_wall_mesh_info;

/* Host only: the cloud's defaults, flags 0, max_step 0.  A NULL is ignored. */
void gm_wall_mesh_default_params(gm_wall_mesh_params *p);
/* The mesh of the window.  Synchronises the map (as gm_wall_map_sync), runs on the map's stream and blocks.  prm NULL: the
 * defaults.  info is required; it, *n_vertices and *n_triangles (either may be NULL) are filled whenever the call got as
 * far as the device, also on GM_ERR_CAPACITY.  A NULL buffer with capacity 0 is not filled; both NULL is a count query
 * (GM_OK).  A non-NULL buffer whose capacity is below its count returns GM_ERR_CAPACITY and leaves the contents of both
 * unspecified (copying stops, counting goes on).  n = 0 gives nothing.  The map is not changed.  Scratch (the cloud's, 4 B
 * per block of the window for the indices, 4 B more per block with a step cut, 12 B per slot of a chunk of triangle
 * staging, a chained scan's records) is allocated on first use, kept grow-only in the map and freed with it; a map that
 * never calls this allocates nothing.
 * GM_ERR_INVALID_ARG: NULL map / info, a window outside the map, a struct_size mismatch (prm's or prm->cloud's), an unknown
 * flag, a parameter outside its limits, reserved not 0, a NULL buffer with capacity > 0. */
gm_status gm_wall_map_mesh(gm_wall_map *map, uint32_t station0, uint32_t n, const gm_wall_mesh_params *prm,
                           gm_wall_mesh_info *info, gm_wall_cloud_point *vertices, uint64_t vertex_capacity,
                           gm_wall_mesh_triangle *triangles, uint64_t triangle_capacity, uint64_t *n_vertices,
                           uint64_t *n_triangles);
/* Host only, no device, no map: the triangle rule above on a vertex list -- rows of a cloud of NJ x NK blocks, whose
 * block field says which blocks are alive and whose mean feeds the step cut.  Fills the mesh half of info (struct_size,
 * wrapped, the quad and triangle counts; info->cloud is zeroed but for blocks_stations, blocks_sectors, blocks and points)
 * and *n_out (may be NULL) whenever the arguments are accepted, also on GM_ERR_CAPACITY.  triangles NULL with capacity 0 is
 * a count query; a capacity below *n_out returns GM_ERR_CAPACITY and writes nothing.
 * GM_ERR_INVALID_ARG: NULL info, vertices NULL with n_vertices > 0, NJ NK above GM_WALL_MAX_CELLS, NK above
 * GM_WALL_MAX_SECTORS, rows whose block is not strictly ascending or is >= NJ NK, an unknown flag, max_step not
 * finite or negative, triangles NULL with capacity > 0. */
gm_status gm_wall_mesh_triangulate(uint32_t NJ, uint32_t NK, const gm_wall_cloud_point *vertices, uint64_t n_vertices,
                                   uint32_t flags, double max_step, gm_wall_mesh_info *info, gm_wall_mesh_triangle *triangles,
                                   uint64_t capacity, uint64_t *n_out);
/* Host only: a binary_little_endian 1.0 PLY file of the mesh -- vertex properties float x, y, z, mean, min, max; faces
 * `list uchar uint vertex_indices` -- as CloudCompare and MeshLab open it.  GM_ERR_INVALID_ARG: NULL path, a NULL array
 * with a count, an index >= n_vertices, a big-endian host.  GM_ERR_DEVICE: the path cannot be written. */
gm_status gm_wall_mesh_write_ply(const char *path, const gm_wall_cloud_point *vertices, uint64_t n_vertices,
                                 const gm_wall_mesh_triangle *triangles, uint64_t n_triangles);

/* ---- the surveyed wall against a structure gauge (gm_wall_map_clearance) ---------------------------------------------
 * Does the vehicle, train or equipment envelope fit, with how much room, and where does it not: every cell of a window
 * of stations against a caller-supplied GAUGE, the radius about the design axis that the envelope needs in each sector.
 * Everything on the device is integer, so the result is a function of the raw cells, the tables and the parameters
 * alone; only the station records, the list of cells short of the margin and the totals leave the device.
 *   gauge       int32 gauge_q[n_gauges][n_sectors], units of 2^-20 m, 1 <= n_gauges <= GM_WALL_CLEAR_MAX_GAUGES.
 *               gauge_q[g][k] == 0: sector k is NOT GAUGED (the invert under the track); a negative entry is refused.
 *               station_gauge (may be NULL: table 0 everywhere) holds one uint8 per WINDOW station, the table of that
 *               station: the envelope moves with track offset and cant along the drive.  An entry >= n_gauges is refused.
 *   integers    R_q = (int64) rint(radius 2^20) and T = (int64) rint(margin 2^20), fp64, once on the host; margin in
 *               [0, 8]; a map with R_q > 2^32 (a radius above 4096 m) is refused.
 *   wall value  a cell is USABLE iff count >= min_count.  GM_WALL_CLEAR_MEAN: w = sum / (int64) count by C integer
 *               division (toward zero), the value of the regions, the check, the locate and the align, saturated at
 *               +-2^30 as the align's.  GM_WALL_CLEAR_MIN (the default, conservative): w = fix(ordered^-1(~min_key)),
 *               the innermost surveyed point, with fix(e) = (int64) rint(e 2^20) on the fp32 product, saturating at
 *               the int32 range and 0 for a NaN, as in the check.
 *   clearance   c = R_q + w - G[k] in int64 (|c| < 2^34).
 *   classes     every window cell is in exactly one, decided in this order: UNGAUGED (G[k] == 0), EMPTY (count 0),
 *               UNUSABLE (0 < count < min_count), INFRINGED (c < 0), TIGHT (0 <= c < T), CLEAR.
 *   station     one record per window station: the least c over its usable gauged cells with the smallest sector
 *               among equals (INT64_MAX and UINT32_MAX when there is none), the counts usable = infringed + tight +
 *               clear, tight, infringed, unsurveyed = empty + unusable among the gauged sectors, and the table used.
 *   list        the tight and the infringed cells, ascending by the map-wide cell index j n_sectors + k.
 *   totals      the six classes (they sum to n n_sectors), the stations with tight + infringed > 0 and with
 *               infringed > 0, and the least c of the window with the smallest cell among equals (INT64_MAX and
 *               UINT32_MAX when there is none).
 * On the device: one pass of one wave per station row for the records and the totals, then, when the list is asked
 * for, one chained-scan compaction per chunk of whole stations of at most 2^20 cells (environment
 * GM_WALL_CLEAR_CHUNK=<cells>, rounded down to whole stations, at least one, a value above 2^20 meaning 2^20, read at
 * gm_wall_map_create: tests and measurements).  The result does not depend on the chunk, the grid or the order blocks
 * run in. */
#define GM_WALL_CLEAR_MIN  0u          /* against the innermost surveyed point of each cell */
#define GM_WALL_CLEAR_MEAN 1u          /* against each cell's integer mean */
#define GM_WALL_CLEAR_MAX_GAUGES   256u
#define GM_WALL_GAUGE_MAX_VERTICES 4096u

typedef struct gm_wall_clearance_params {   /* 24 bytes */
    uint32_t struct_size;     /* = sizeof(gm_wall_clearance_params) */
    uint32_t reference;       /* GM_WALL_CLEAR_MIN (default) or GM_WALL_CLEAR_MEAN */
    uint32_t min_count;       /* >= 1 (default 8): points a cell needs to be usable */
    uint32_t reserved;        /* 0 */
    double   margin;          /* metres, in [0, 8] (default 0.10): clearance below it is tight */
} gm_wall_clearance_params;

typedef struct gm_wall_clearance_station {   /* 32 bytes */
    int64_t  min_clearance;   /* least c of the station, 2^-20 m; INT64_MAX when no cell is usable and gauged */
    uint32_t min_sector;      /* its sector, the smallest among equals; UINT32_MAX when there is none */
    uint32_t usable;          /* gauged cells with count >= min_count: infringed + tight + clear */
    uint32_t tight, infringed;
    uint32_t unsurveyed;      /* gauged cells that are empty or unusable */
    uint32_t gauge;           /* the table used */
} gm_wall_clearance_station;

typedef struct gm_wall_clearance_cell {   /* 16 bytes */
    uint32_t cell;            /* map-wide j * n_sectors + k */
    uint32_t count;
    int64_t  clearance;       /* c < T, 2^-20 m */
} gm_wall_clearance_cell;

typedef struct gm_wall_clearance_info {   /* 104 bytes */
    uint32_t struct_size;     /* = sizeof(gm_wall_clearance_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;   /* the window and the map's sectors */
    int64_t  margin_q, radius_q;                /* T, R_q */
    uint64_t ungauged, empty, unusable, infringed, tight, clear;   /* window cells per class */
    uint32_t stations_tight;       /* stations with tight + infringed > 0 */
    uint32_t stations_infringed;   /* stations with infringed > 0 */
    int64_t  min_clearance;   /* least c of the window; INT64_MAX when no cell is usable and gauged */
    uint32_t min_cell;        /* its map-wide cell, the smallest among equals; UINT32_MAX when there is none */
    uint32_t reserved;        /* 0 */
} gm_wall_clearance_info;

typedef struct gm_wall_clearance_run {   /* 72 bytes; fp64 derived on the host, one rounding per operation */
    uint32_t station_from, station_to;   /* map-wide, inclusive: the first and the last station short of the margin */
    double   chainage_from;   /* t_min + station_from * station_length */
    double   chainage_to;     /* t_min + (station_to + 1) * station_length */
    int64_t  min_clearance;   /* least min_clearance of the run's stations, 2^-20 m */
    double   min_clearance_m; /* min_clearance 2^-20 */
    uint32_t min_station;     /* map-wide; the first among equals */
    uint32_t min_sector;
    double   angle_deg;       /* (360 (2 min_sector + 1)) / (2 n_sectors): the centre of the sector */
    uint64_t tight, infringed;   /* summed over stations station_from .. station_to */
} gm_wall_clearance_run;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_clearance_default_params(gm_wall_clearance_params *p);
/* Host only, no device, no map: everything gm_wall_map_clearance refuses but the window and the output buffers, for a
 * map with the parameters p (n_sectors and radius decide) and a window of n stations.  c NULL: the defaults;
 * station_gauge may be NULL.  GM_ERR_INVALID_ARG: p or gauge_q NULL, a struct_size mismatch, n_sectors outside
 * 1 .. GM_WALL_MAX_SECTORS, rint(radius 2^20) > 2^32 or radius not positive and finite, reference above
 * GM_WALL_CLEAR_MEAN, min_count 0, margin outside [0, 8], n_gauges outside 1 .. GM_WALL_CLEAR_MAX_GAUGES, a negative
 * gauge entry, a station_gauge entry >= n_gauges. */
gm_status gm_wall_clearance_check_params(const gm_wall_params *p, const gm_wall_clearance_params *c, const int32_t *gauge_q,
                                         uint32_t n_gauges, const uint8_t *station_gauge, uint32_t n);
/* The clearance of stations [station0, station0 + n).  Synchronises the map (as gm_wall_map_sync), runs on the map's
 * stream and blocks.  prm NULL: the defaults.  info is required; it and *n_out (may be NULL; the number of list cells,
 * tight + infringed) are filled whenever the call got as far as the device, also on GM_ERR_CAPACITY.  stations NULL
 * with station_capacity 0 and cells NULL with cell_capacity 0 are count queries (GM_OK): info.n_stations records and
 * *n_out cells are what a second call needs room for.  A station_capacity below n or a cell_capacity below *n_out with
 * a buffer returns GM_ERR_CAPACITY and writes neither array.  n = 0 gives nothing.  The map is not changed.  Scratch
 * (the uploaded tables, 32 B per window station, 16 B per cell of a chunk of staging, the chained scan's own records)
 * is allocated on first use, kept grow-only in the map and freed with it; a map that never calls this allocates
 * nothing.  GM_ERR_INVALID_ARG: NULL map / info, a window outside the map, whatever gm_wall_clearance_check_params
 * refuses, stations or cells NULL with a capacity. */
gm_status gm_wall_map_clearance(gm_wall_map *map, uint32_t station0, uint32_t n, const int32_t *gauge_q, uint32_t n_gauges,
                                const uint8_t *station_gauge, const gm_wall_clearance_params *prm, gm_wall_clearance_info *info,
                                gm_wall_clearance_station *stations, uint32_t station_capacity, gm_wall_clearance_cell *cells,
                                uint64_t cell_capacity, uint64_t *n_out);
/* Host only, no device, no map: one gauge table from a polygon in the section plane.  uv holds n_vertices rows
 * (along u, along v) in metres about the design axis, shifted by offset[2] (may be NULL: no shift): P_i = uv_i + offset.
 * The polygon is closed (the last vertex joins the first), simple, has 3 .. GM_WALL_GAUGE_MAX_VERTICES vertices and
 * holds the axis strictly inside.  Sector k is the wedge between the rays at phi_k = 2 pi (k / n_sectors) and phi_k+1
 * (phi is 0 toward u and grows toward v, as in the binning; the last ray is the first).  g_k is the largest distance
 * from the axis over the vertices inside the wedge -- cross(d_k, P) >= 0 and cross(P, d_k+1) >= 0 with the ray
 * directions d = (cos phi, sin phi) of the host's libm; every vertex with one sector -- and over the intersections of
 * every edge with the wedge's two rays: exact for the boundary inside the wedge, distance being convex along an edge.
 * gauge_q[k] = ceil(g_k 2^20).  *n_out (may be NULL) = n_sectors; a capacity below it returns GM_ERR_CAPACITY and
 * writes nothing.  GM_ERR_INVALID_ARG: a NULL, p->struct_size mismatch, n_sectors outside 1 .. GM_WALL_MAX_SECTORS, a
 * vertex count outside its limits, a coordinate that is not finite, an edge of length 0, edges that cross or touch,
 * the axis outside or on the boundary, a g_k of 2048 m or more. */
gm_status gm_wall_gauge_from_polygon(const gm_wall_params *p, const double *uv, uint32_t n_vertices, const double offset[2],
                                     int32_t *gauge_q, uint32_t capacity, uint32_t *n_out);
/* Host only, no device, no map: the n station records of a window that starts at map station station0, folded into
 * chainage runs.  A station is FLAGGED iff tight + infringed > 0; flagged stations with at most max_gap stations that
 * are not flagged between them belong to one run, which starts and ends on a flagged station.  *n_out (may be NULL) =
 * the number of runs; runs NULL with capacity 0 is a count query, a capacity below *n_out returns GM_ERR_CAPACITY and
 * writes nothing.  GM_ERR_INVALID_ARG: p NULL, p->struct_size mismatch, n_sectors 0, stations NULL with n > 0, runs
 * NULL with a capacity, station0 + n above 2^32. */
gm_status gm_wall_clearance_runs(const gm_wall_params *p, const gm_wall_clearance_station *stations, uint32_t n,
                                 uint32_t station0, uint32_t max_gap, gm_wall_clearance_run *runs, uint32_t capacity,
                                 uint32_t *n_out);

/* ---- a robust profile fit per chainage section (gm_wall_map_sections) -------------------------------------------------
 * The as-built cross-section per chainage: how far the tube has closed or opened against the design radius, where its
 * centre sits against the design axis, how oval it is and in which direction -- per section of the drive and, with a
 * baseline map, between two epochs.  A station's row of sector means is a sampled rho(phi) - R; its low Fourier
 * harmonics are these quantities (h = 0 radius change, h = 1 centre offset, h = 2 ovalisation, h = 3, 4 squatting and
 * local shape).  Everything on the device is integer; the one fp64 step, a small solve per section and pass, runs on
 * the host and is exported (gm_wall_section_solve), so the records are a function of the raw cells, the basis table
 * and the parameters alone.
 *   sections    the window is stations [station0, station0 + n), S = section_stations, NS = ceil(n / S); section i is
 *               window stations [i S, min((i + 1) S, n)).
 *   column      column (i, k) is the cells of sector k over the section's stations, merged exactly as
 *               gm_wall_map_cloud merges a block: the count a u64 sum, the sum an int64 sum (empty cells add nothing),
 *               q = sum / (int64) count by C division.  Without a baseline m = q and the column is USABLE iff
 *               count >= min_count.  With a baseline (the refusals of gm_wall_map_regions) m = q(map) - q(baseline) and
 *               the column is USABLE iff both counts are >= min_count.  m saturates at +-2^24 units of 2^-20 m (16 m,
 *               twice the largest gate).  Every column is in exactly one class: EMPTY (count 0, and with a baseline
 *               count 0 there too), UNUSABLE, usable.
 *   basis       P = 1 + 2 H unknowns, H = harmonics in 0 .. 4.  The table is made once per call on the host with libm:
 *               int32 B[k][P], B[k][0] = 2^20, B[k][2h - 1] = rint(cos(h phi_k) 2^20), B[k][2h] = rint(sin(h phi_k) 2^20),
 *               phi_k = 2 pi (2k + 1) / (2 n_sectors), the sector's centre (the angle of gm_wall_clearance_run.angle_deg);
 *               one operation per statement.  gm_wall_section_basis returns the table the call uses.
 *   sums        of a pass, over the FITTED columns of a section, all int64: N[p][q] = sum B_p B_q for p <= q, packed
 *               row-major in the call's P (slot p P - p (p - 1) / 2 + q - p of 45, the unused slots 0), r[p] = sum B_p m,
 *               the fitted count, the fitted points (their merged counts, of the map) and largest_gap, the longest
 *               cyclic run of consecutive sectors that are not fitted (n_sectors when none is, 0 when all are).
 *               |N| <= 2^40 4096 = 2^52 and |r| <= 2^20 2^24 2^12 = 2^56.  This is gm_wall_section_sums.
 *   solve       on the host in fp64, one operation per statement so that nothing can contract: A = N 2^-40 (exact),
 *               b = r 2^-20 (one rounding, the conversion), a Cholesky solve A c = b.  In this order: a fitted count
 *               below max(min_columns, P) gives GM_SECTION_TOO_FEW; a pivot that is not above 1e-12 of its diagonal
 *               entry gives GM_SECTION_SINGULAR; c_q[p] = (int64) rint(c[p]), units of 2^-20 m, and |c_q| > 2^24 gives
 *               GM_SECTION_UNBOUNDED.  Each of the three FAILS the section: its later passes are skipped, its
 *               coefficients, accepted, rejected, points and residual fields are 0 and its peak sectors UINT32_MAX.
 *   model       integer: M_k = (sum_p B[k][p] c_q[p] + 2^19) >> 20 (an arithmetic shift), rho_k = m_k - M_k.
 *   passes      P_f = passes in 1 .. 4.  Pass 1 fits every usable column; pass p >= 2 fits the usable columns with
 *               |rho| <= Tr 2^(P_f - p) against the model of pass p - 1, Tr = (int64) rint(reject 2^20) >= 1, reject in
 *               (0, 8]: the tightening of the cylinder regression's 4 tau, 2 tau, tau.
 *   evaluation  one more launch against the last model: ACCEPTED are the usable columns with |rho| <= Tr, rejected =
 *               usable - accepted, rss = sum rho^2 over the accepted (<= 2^46 2^12), peak_out and peak_in the largest
 *               and the smallest rho over ALL usable columns (a rejected niche is what one wants to see) with their
 *               sectors, the smallest among equals (0 and UINT32_MAX without a usable column), points the merged count
 *               of the accepted columns, of the map.
 *   flag        GM_SECTION_OPEN_ARC: largest_gap of the last fitting pass that ran exceeds floor(max_gap_deg n_sectors /
 *               360).  It fails nothing and the values are kept, as GM_FIT_NOT_CONVERGED keeps its own: on a 120 degree
 *               arc the harmonics trade against each other (with H = 4 the least Cholesky pivot ratio falls to about
 *               1e-5), and the caller must be told.
 * h = 1 is the centre offset to FIRST ORDER only: a circle of radius R' displaced by delta also contributes
 * -delta^2 / (4 R') to h = 0 and delta^2 / (4 R') to h = 2.
 * On the device: one kernel, launched passes + 1 times per chunk of sections (2^16 by default; environment
 * GM_WALL_SECTION_CHUNK=<sections>, 0 or more than 2^16 meaning 2^16, read at gm_wall_map_create: tests only); the sums
 * go to the host and the coefficients come back between the launches.  No floating point and no floating-point atomics
 * on the device: the result does not depend on the chunk, the grid or the order. */
#define GM_SECTION_OK         0u
#define GM_SECTION_TOO_FEW    (1u << 0)   /* fewer fitted columns than max(min_columns, P) */
#define GM_SECTION_SINGULAR   (1u << 1)   /* a Cholesky pivot not above 1e-12 of its diagonal entry */
#define GM_SECTION_UNBOUNDED  (1u << 2)   /* a coefficient beyond 2^24 units (16 m) */
#define GM_SECTION_FAILED_MASK 0xFFu      /* status & mask != 0: no fit, the values are 0 */
#define GM_SECTION_OPEN_ARC   (1u << 8)   /* the fitted sectors leave a gap above max_gap_deg: the values are kept */
#define GM_WALL_SECTION_MAX_HARMONICS 4u
#define GM_WALL_SECTION_MAX_PASSES    4u

typedef struct gm_wall_section_params {   /* 40 bytes */
    uint32_t struct_size;       /* = sizeof(gm_wall_section_params) */
    uint32_t section_stations;  /* S >= 1 (default 4) */
    uint32_t harmonics;         /* H in 0 .. 4 (default 2) */
    uint32_t passes;            /* P_f in 1 .. 4 (default 3) */
    uint32_t min_count;         /* >= 1 (default 8): points a column needs to be usable */
    uint32_t min_columns;       /* >= 1 (default 24): fitted columns a pass needs (and never fewer than P) */
    double   max_gap_deg;       /* in [0, 360] (default 90): a larger gap sets GM_SECTION_OPEN_ARC */
    double   reject;            /* metres, in (0, 8] (default 0.05): Tr */
} gm_wall_section_params;

typedef struct gm_wall_section_sums {   /* 448 bytes: the sums of one pass of one section */
    int64_t  N[45];             /* the upper triangle, packed row-major in the call's P; unused slots 0 */
    int64_t  r[9];              /* unused slots 0 */
    uint32_t fitted;            /* the columns summed */
    uint32_t largest_gap;       /* sectors */
    uint64_t points;            /* merged count of the fitted columns */
} gm_wall_section_sums;

typedef struct gm_wall_section {   /* 144 bytes */
    uint32_t station_from;      /* map-wide first station */
    uint32_t stations;          /* 1 .. S */
    uint32_t status;            /* GM_SECTION_* */
    uint32_t usable;            /* columns */
    uint32_t fitted;            /* of the last fitting pass that ran */
    uint32_t accepted, rejected;
    uint32_t largest_gap;       /* of the last fitting pass that ran, sectors */
    uint64_t points;            /* merged count of the accepted columns */
    int64_t  coef_q[9];         /* c0, a1, b1, a2, b2, ..., units of 2^-20 m; unused slots 0 */
    uint64_t rss;               /* sum rho^2 over the accepted columns, units of 2^-40 m^2 */
    int64_t  peak_out, peak_in; /* the largest and the smallest rho over the usable columns */
    uint32_t peak_out_sector, peak_in_sector;
} gm_wall_section;

typedef struct gm_wall_sections_info {   /* 96 bytes */
    uint32_t struct_size;       /* = sizeof(gm_wall_sections_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;   /* the window and the map's sectors */
    uint32_t section_stations, sections;        /* S, NS */
    uint32_t harmonics, passes;                 /* H, P_f */
    int64_t  reject_q;          /* Tr */
    uint32_t max_gap_sectors;   /* floor(max_gap_deg n_sectors / 360) */
    uint32_t sections_ok;       /* status & GM_SECTION_FAILED_MASK == 0 */
    uint32_t sections_failed;
    uint32_t sections_open_arc; /* GM_SECTION_OPEN_ARC set (failed or not) */
    uint64_t empty, unusable, usable;   /* columns per class: they sum to NS n_sectors */
    uint64_t accepted, rejected;        /* of the sections that did not fail */
} gm_wall_sections_info;

struct gm_wall_section_metrics {   /* 128 bytes; fp64 derived on the host, one rounding per operation */
    double chainage_from;       /* t_min + station_from * station_length */
    double chainage_to;         /* t_min + (station_from + stations) * station_length */
    double radius_m;            /* R + c0 */
    double radial_m;            /* c0: convergence (negative: the tube has closed) */
    double centre_u, centre_v;  /* a1, b1: the centre against the design axis, to first order (see above) */
    double centre[3];           /* o + t_mid a + a1 u + b1 v in map coordinates, t_mid the section's mid chainage */
    double oval_m;              /* hypot(a2, b2) */
    double oval_angle_deg;      /* atan2(b2, a2) / 2 in [0, 180): the direction of the long axis; 0 without h = 2 */
    double diameter_max;        /* 2 (R + c0 + oval_m) */
    double diameter_min;        /* 2 (R + c0 - oval_m) */
    double rms_m;               /* sqrt(rss / accepted) 2^-20; 0 without an accepted column */
    double area_m2;             /* pi (R + c0)^2 + (pi / 2) sum_{h >= 1} (a_h^2 + b_h^2): 1/2 the ring integral of rho^2 */
    double coverage;            /* accepted / n_sectors */
};

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_section_default_params(gm_wall_section_params *p);
/* Host only, no device, no map: what gm_wall_map_sections refuses of its parameters.  GM_ERR_INVALID_ARG: NULL, a
 * struct_size mismatch, section_stations 0, harmonics above 4, passes outside 1 .. 4, min_count 0, min_columns 0,
 * max_gap_deg outside [0, 360], reject outside (0, 8] or rounding to Tr = 0. */
gm_status gm_wall_section_check_params(const gm_wall_section_params *p);
/* Host only: the basis table B[n_sectors][1 + 2 harmonics] of a map with n_sectors sectors, the one the call uploads.
 * *n_out (may be NULL) = the number of entries; basis NULL with capacity 0 is a count query, a capacity below *n_out
 * returns GM_ERR_CAPACITY and writes nothing.  GM_ERR_INVALID_ARG: n_sectors outside 1 .. GM_WALL_MAX_SECTORS, harmonics
 * above 4, basis NULL with a capacity. */
gm_status gm_wall_section_basis(uint32_t n_sectors, uint32_t harmonics, int32_t *basis, uint32_t capacity, uint32_t *n_out);
/* Host only: the solve above on one record of sums.  coef_q receives 9 entries (0 in the unused slots and on a failed
 * section), *status one of GM_SECTION_OK, _TOO_FEW, _SINGULAR, _UNBOUNDED.  GM_ERR_INVALID_ARG: a NULL, harmonics above
 * 4, min_columns 0. */
gm_status gm_wall_section_solve(const gm_wall_section_sums *sums, uint32_t harmonics, uint32_t min_columns, int64_t coef_q[9],
                                uint32_t *status);
/* Host only: the metrics of one record under the map's parameters.  A failed section gives GM_OK and zeros but for the
 * chainage interval.  GM_ERR_INVALID_ARG: a NULL, p->struct_size mismatch, n_sectors 0, harmonics above 4, a record of 0
 * stations. */
gm_status gm_wall_section_metrics(const gm_wall_params *p, const gm_wall_section *s, uint32_t harmonics,
                                  struct gm_wall_section_metrics *out);
/* The sections of stations [station0, station0 + n).  Synchronises the map and the baseline (as gm_wall_map_sync),
 * runs on the map's stream and blocks.  baseline NULL: against the design; else another map of the same context on
 * the same grid (refused as gm_wall_map_regions refuses it).  prm NULL: the defaults.  info is required; it and *n_out
 * (may be NULL; NS) are filled whenever the call got past its refusals, also on GM_ERR_CAPACITY.  sections NULL with
 * capacity 0 is a count query (GM_OK; info is complete, NS records are what a second call needs room for); a capacity
 * below NS with a buffer returns GM_ERR_CAPACITY before anything runs on the device: the totals of info are 0 then.  sums (may be NULL) receives the NS records of each section's
 * last fitting pass that ran.  n = 0 gives nothing.  Neither map is changed.  Scratch (the basis table and 592 B per
 * section of a chunk) is allocated on first use, kept grow-only in the map and freed with it; a map that never calls
 * this allocates and launches nothing new.  GM_ERR_INVALID_ARG: NULL map / info, a window outside the map, whatever
 * gm_wall_section_check_params refuses, a refused baseline, sections NULL with a capacity or with sums. */
gm_status gm_wall_map_sections(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n,
                               const gm_wall_section_params *prm, gm_wall_sections_info *info, gm_wall_section *sections,
                               uint32_t capacity, uint32_t *n_out, gm_wall_section_sums *sums);

/* ---- over- and underbreak per section and zone (gm_wall_map_quantities) -----------------------------------------------
 * What a survey is paid by: per advance the underbreak, the overbreak and the unpaid excess against the contract's two
 * lines -- the minimum excavation line, inside which rock must still come out, and the pay line, beyond which overbreak
 * is not paid -- as areas by crown, side walls and invert, and how much of the ring was surveyed at all; with a baseline
 * map the same between two epochs: how much lining went on and where it is thinner than required.  Everything on the
 * device is integer, so the records are a function of the raw cells, the tables and the parameters alone.
 *   sections    exactly those of gm_wall_map_sections: S = section_stations, NS = ceil(n / S), section i is window
 *               stations [i S, min((i + 1) S, n)).
 *   column      column (i, k) merges sector k over the section's stations as there: the count a u64 sum, the sum an
 *               int64 sum (empty cells add nothing), q = sum / (int64) count by C division, saturated at +-2^24 units
 *               of 2^-20 m.  USABLE iff count >= min_count and, with a baseline (the refusals of gm_wall_map_regions),
 *               the baseline's count too.
 *   value       R_q = (int64) rint(radius 2^20), fp64, once on the host; a map with R_q > 2^32 is refused.  The base
 *               radius is b0 = R_q without a baseline and b0 = R_q + q(baseline) with one; the wall radius is
 *               x = R_q + q(map); the compared value is v = x - b0.
 *   lines       int32 lo_q[n_profiles][n_sectors] and hi_q[n_profiles][n_sectors], offsets from the base radius in
 *               units of 2^-20 m, |entry| <= 2^24 and lo <= hi, 1 <= n_profiles <= GM_WALL_QUANTITY_MAX_PROFILES.
 *               L = b0 + lo and H = b0 + hi.  section_profile (may be NULL: table 0) holds one uint8 per SECTION, the
 *               table of that section, as gm_wall_map_clearance's station_gauge; an entry >= n_profiles is refused.
 *               Without a baseline the lines are the contract's two lines about the design axis: such a table is
 *               gm_wall_gauge_from_polygon's output minus R_q.  That helper rounds OUTWARD (the farthest point of the
 *               polygon inside the sector's wedge, then ceil): right for a pay line, a few units generous for a minimum
 *               excavation line.  With a baseline the lines are offsets from the earlier wall: lo = hi = 0 splits
 *               "moved in" from "moved out", lo = hi = -t finds lining thinner than t.
 *   zones       uint8 zone[n_sectors] (may be NULL: zone 0 everywhere), 1 <= n_zones <= GM_WALL_QUANTITY_MAX_ZONES;
 *               GM_WALL_QUANTITY_UNMEASURED (0xFF): the sector is not measured (the invert under the muck); any other
 *               entry >= n_zones is refused.
 *   classes     every column is in exactly one, decided in this order: UNMEASURED (zone 0xFF), EMPTY (count 0, and
 *               with a baseline count 0 there too), UNUSABLE, UNDER (v < lo), OVER (v > hi), WITHIN.
 *   area term   for b >= a >= 0, ann(a, b) = ((b - a) (b + a)) >> 20 in int64: twice the area of the sector between
 *               the two radii divided by the sector angle, units of 2^-20 m^2; the truncation, at most one unit per
 *               column, is part of the rule.  L, H and x are clamped at 0 from below before they enter an area term
 *               (the peaks and the classes use them as they are).  b - a < 2^26 and b + a < 2^34, so no product
 *               exceeds 2^60 and a record's sums stay below 2^52.
 *   record      per (section, zone), over the zone's columns: the counts under, within, over and unsurveyed = empty +
 *               unusable; points, the map's merged count over the usable columns; under_area = sum ann(x, L) over
 *               UNDER; over_area = sum ann(L, x) over the usable columns with x > L, WITHIN or OVER; excess_area = sum
 *               ann(H, x) over OVER -- the paid overbreak is over_area - excess_area; peak_under = max (L - x) over
 *               UNDER and peak_over = max (x - L) over x > L, each with its sector, the smallest among equals (0 and
 *               UINT32_MAX without such a column).  A zone without a sector gives zeros (and both sectors UINT32_MAX).
 *               Records are ordered [NS][n_zones].
 *   profile     optional, int32 [NS][n_sectors]: v of the column, INT32_MIN when it is not usable.  An unmeasured
 *               sector that is usable still gets its value: the drawing wants the invert too.
 *   totals      the six classes (they sum to NS n_sectors) and the sections with at least one UNDER and with at least
 *               one OVER column.  No area totals: a window's could exceed 64 bits, a record's cannot.
 * On the device: one wave per section over chunks of whole sections; it reads count and sum only.  The default chunk
 * keeps the staging (88 B per record, 4 B per profile entry) within 24 MiB; environment
 * GM_WALL_QUANTITY_CHUNK=<sections>, 0 or more than the default meaning the default, read at gm_wall_map_create: tests
 * and measurements.  No floating point and no floating-point atomics on the device: the result does not depend on the
 * chunk, the grid, the block shape or the order blocks run in. */
#define GM_WALL_QUANTITY_MAX_PROFILES 256u
#define GM_WALL_QUANTITY_MAX_ZONES    8u
#define GM_WALL_QUANTITY_UNMEASURED   0xFFu
#define GM_WALL_QUANTITY_CLASS_UNMEASURED 0u
#define GM_WALL_QUANTITY_CLASS_EMPTY      1u
#define GM_WALL_QUANTITY_CLASS_UNUSABLE   2u
#define GM_WALL_QUANTITY_CLASS_UNDER      3u
#define GM_WALL_QUANTITY_CLASS_OVER       4u
#define GM_WALL_QUANTITY_CLASS_WITHIN     5u
#define GM_WALL_QUANTITY_RUNS_ALL_ZONES   1u   /* gm_wall_quantity_runs: one run per interval over all zones */

typedef struct gm_wall_quantity_params {   /* 16 bytes */
    uint32_t struct_size;       /* = sizeof(gm_wall_quantity_params) */
    uint32_t section_stations;  /* S >= 1 (default 4) */
    uint32_t min_count;         /* >= 1 (default 8): points a column needs to be usable */
    uint32_t reserved;          /* 0 */
} gm_wall_quantity_params;

typedef struct gm_wall_quantity {   /* 88 bytes: one (section, zone) */
    uint32_t station_from;      /* map-wide first station */
    uint32_t stations;          /* 1 .. S */
    uint32_t zone;
    uint32_t profile;           /* the table used */
    uint32_t under, within, over;
    uint32_t unsurveyed;        /* measured columns that are empty or unusable */
    uint64_t points;            /* merged count of the usable columns, of the map */
    int64_t  under_area, over_area, excess_area;   /* sums of ann, units of 2^-20 m^2 */
    int64_t  peak_under, peak_over;                /* units of 2^-20 m; 0 without such a column */
    uint32_t peak_under_sector, peak_over_sector;  /* the smallest among equals; UINT32_MAX without such a column */
} gm_wall_quantity;

typedef struct gm_wall_quantities_info {   /* 96 bytes */
    uint32_t struct_size;       /* = sizeof(gm_wall_quantities_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;   /* the window and the map's sectors */
    uint32_t section_stations, sections;        /* S, NS */
    uint32_t n_zones, n_profiles;
    int64_t  radius_q;          /* R_q */
    uint64_t unmeasured, empty, unusable, under, over, within;   /* columns per class: they sum to NS n_sectors */
    uint32_t sections_under;    /* sections with at least one UNDER column */
    uint32_t sections_over;     /* sections with at least one OVER column */
} gm_wall_quantities_info;

typedef struct gm_wall_quantity_column_result {   /* 40 bytes: one column restated on the host */
    uint32_t cls;               /* GM_WALL_QUANTITY_CLASS_* */
    int32_t  v;                 /* x - b0; INT32_MIN when the column is not usable */
    int64_t  under_area, over_area, excess_area;   /* the column's three area terms (0 where its class has none) */
    int64_t  over_line;         /* x - L of a usable column (negative: the depth of the underbreak), else 0 */
} gm_wall_quantity_column_result;

struct gm_wall_quantity_metrics {   /* 136 bytes; fp64 derived on the host, one rounding per operation */
    double chainage_from;       /* t_min + station_from * station_length */
    double chainage_to;         /* t_min + (station_from + stations) * station_length */
    double length;              /* stations * station_length */
    double under_area_m2, over_area_m2, excess_area_m2;   /* ((area 2^-20) pi) / n_sectors */
    double paid_area_m2;        /* the same of over_area - excess_area */
    double under_volume_m3, over_volume_m3, excess_volume_m3, paid_volume_m3;   /* area * length */
    double peak_under_m, peak_over_m;                     /* peak 2^-20 */
    double peak_under_angle_deg, peak_over_angle_deg;     /* (360 (2 sector + 1)) / (2 n_sectors); 0 without a peak */
    double coverage;            /* usable / measured, usable = under + within + over, measured = usable + unsurveyed; 0 of 0 */
    double reserved;            /* 0 */
};

typedef struct gm_wall_quantity_run {   /* 136 bytes: a pay interval; fp64 derived on the host */
    uint32_t station_from;      /* map-wide first station of the interval */
    uint32_t stations;
    uint32_t zone;              /* UINT32_MAX: over all zones */
    uint32_t sections;          /* 1 .. run_sections */
    double   chainage_from, chainage_to;
    uint64_t under, within, over, unsurveyed, points;   /* integer sums over the interval's records */
    double   under_volume_m3, over_volume_m3, excess_volume_m3, paid_volume_m3;   /* summed in section order, then zone */
    int64_t  peak_under, peak_over;                     /* the largest of the interval, the first among equals */
    uint32_t peak_under_station, peak_under_sector;     /* station_from of that section; UINT32_MAX without a peak */
    uint32_t peak_over_station, peak_over_sector;
} gm_wall_quantity_run;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_quantity_default_params(gm_wall_quantity_params *p);
/* Host only, no device, no map: everything gm_wall_map_quantities refuses but the window, the baseline and the output
 * buffers, for a map with the parameters p (n_sectors and radius decide) and a window of n stations.  q NULL: the
 * defaults; section_profile (ceil(n / S) entries) and zone may be NULL.  GM_ERR_INVALID_ARG: p, lo_q or hi_q NULL, a
 * struct_size mismatch, n_sectors outside 1 .. GM_WALL_MAX_SECTORS, rint(radius 2^20) > 2^32 or radius not positive and
 * finite, section_stations 0, min_count 0, n_profiles outside 1 .. 256, an entry beyond +-2^24, lo > hi, a
 * section_profile entry >= n_profiles, n_zones outside 1 .. 8, a zone entry in n_zones .. 0xFE. */
gm_status gm_wall_quantity_check_params(const gm_wall_params *p, const gm_wall_quantity_params *q, const int32_t *lo_q,
                                        const int32_t *hi_q, uint32_t n_profiles, const uint8_t *section_profile, uint32_t n,
                                        const uint8_t *zone, uint32_t n_zones);
/* Host only: one column restated -- what gm_wall_check_classify is to the check.  (count, sum) is the column merged
 * over the map, (base_count, base_sum) over the baseline when has_baseline is not 0; zone_entry is the sector's zone
 * table entry (0xFF: unmeasured).  GM_ERR_INVALID_ARG: out NULL, radius_q outside 1 .. 2^32, min_count 0, an entry
 * beyond +-2^24, lo > hi. */
gm_status gm_wall_quantity_column(int64_t radius_q, uint64_t count, int64_t sum, int has_baseline, uint64_t base_count,
                                  int64_t base_sum, uint32_t min_count, int32_t lo, int32_t hi, uint32_t zone_entry,
                                  gm_wall_quantity_column_result *out);
/* Host only: the metrics of one record under the map's parameters.  GM_ERR_INVALID_ARG: a NULL, p->struct_size mismatch
 * or parameters gm_wall_map_create refuses, a record of 0 stations. */
gm_status gm_wall_quantity_metrics(const gm_wall_params *p, const gm_wall_quantity *r, struct gm_wall_quantity_metrics *out);
/* Host only: the records [n_sections][n_zones] of a call folded into pay intervals of run_sections consecutive
 * sections, the last one shorter: NR = ceil(n_sections / run_sections) intervals.  Without flags one run per interval
 * and zone, ordered [NR][n_zones]; with GM_WALL_QUANTITY_RUNS_ALL_ZONES one per interval over all zones.  Counts are
 * integer sums; each volume is the record's (gm_wall_quantity_metrics') summed in fp64 in section order, zones in
 * order within a section; the peaks are the largest of the interval, the first among equals in that order.  *n_out
 * (may be NULL) = the number of runs; runs NULL with capacity 0 is a count query, a capacity below *n_out returns
 * GM_ERR_CAPACITY and writes nothing.  GM_ERR_INVALID_ARG: p as above, records NULL with sections, n_zones outside
 * 1 .. 8, run_sections 0, an unknown flag, runs NULL with a capacity. */
gm_status gm_wall_quantity_runs(const gm_wall_params *p, const gm_wall_quantity *records, uint32_t n_sections, uint32_t n_zones,
                                uint32_t run_sections, uint32_t flags, gm_wall_quantity_run *runs, uint32_t capacity,
                                uint32_t *n_out);
/* The quantities of stations [station0, station0 + n).  Synchronises the map and the baseline (as gm_wall_map_sync),
 * runs on the map's stream and blocks.  baseline NULL: against the design; else another map of the same context on
 * the same grid (refused as gm_wall_map_regions refuses it).  prm NULL: the defaults; section_profile NULL: table 0;
 * zone NULL: zone 0 everywhere.  info is required; it and *n_out (may be NULL; NS n_zones records) are filled whenever
 * the call got past its refusals, also on GM_ERR_CAPACITY.  records NULL with capacity 0 is a count query (GM_OK; info
 * is complete); a capacity below NS n_zones with a buffer returns GM_ERR_CAPACITY and writes neither array.
 * profile_rows (may be NULL) receives NS n_sectors entries.  n = 0 gives nothing.  Neither map is changed.  Scratch
 * (the uploaded tables and the staging of a chunk) is allocated on first use, kept grow-only in the map and freed with
 * it; a map that never calls this allocates and launches nothing new.  GM_ERR_INVALID_ARG: NULL map / info, a window
 * outside the map, whatever gm_wall_quantity_check_params refuses, a refused baseline, records NULL with a capacity or
 * with profile_rows. */
gm_status gm_wall_map_quantities(gm_wall_map *map, gm_wall_map *baseline, uint32_t station0, uint32_t n, const int32_t *lo_q,
                                 const int32_t *hi_q, uint32_t n_profiles, const uint8_t *section_profile,
                                 const uint8_t *zone, uint32_t n_zones, const gm_wall_quantity_params *prm,
                                 gm_wall_quantities_info *info, gm_wall_quantity *records, uint32_t capacity, uint32_t *n_out,
                                 int32_t *profile_rows);

/* ---- a frame's changed points against the wall map (gm_wall_map_check_*) ----------------------------------------------
 * Which points of the frame in front of the sensor are NOT where the map says the wall is: rockfall, a fallen lining
 * segment, a vehicle in the profile, new shotcrete.  One device pass over the frame's valid cloud under a pose; only the
 * changed points and a few counters leave the device.  The rule is integer from e on:
 *   per check     exactly gm_wall_map_add_frame's "per add" (fp64 on the host, the anchor station, o', a', u', v' rounded
 *                 to fp32 once, the pose checks), reported in a gm_wall_add_info -- but for the gate, which is the
 *                 CHECK's own parameter rounded to fp32 once, not the map's: an object standing in the profile lies far
 *                 inside the map's gate and must not vanish.
 *   per point     the add's fp32 chain unchanged: e, the station j = j_f + floor(t / ds) in 64-bit integers, the sector k.
 *   integers      e_q = (int64) rint(e 2^20), the very integer the add sums (fp32 product rounded to nearest even, the
 *                 conversion saturating at the int32 range, 0 for a NaN -- never reached by a gated e);
 *                 T = (int64) rint(threshold 2^20), fp64, once on the host, threshold in (0, 8] and T >= 1.
 *                 A cell is USABLE iff count >= min_count.
 *   reference     GM_WALL_CHECK_MEAN: delta = e_q - q, q = sum / (int64) count by C integer division (toward zero): the
 *                 value of gm_wall_map_regions.  GM_WALL_CHECK_ENVELOPE: lo_q, hi_q = the same rint of the cell's min and
 *                 max decoded from min_key / max_key; delta = e_q - hi_q if e_q > hi_q, e_q - lo_q if e_q < lo_q, else 0
 *                 (rough rock and shotcrete have wide cells; a point inside the surveyed spread is not a change).
 *                 |delta| <= 2^24 for a map whose cells came from points (any gate <= 8).
 *   classes       every valid point is in exactly one: plane (label 1), beyond_gate (|e| > gate or e not finite), outside
 *                 (j not in [0, n_stations)), unsurveyed (mapped, cell not usable), unchanged (|delta| < T), changed_pos
 *                 (delta >= T: farther from the axis than the survey), changed_neg (delta <= -T: inside the profile).
 *   list          the changed points, ascending by index in the valid cloud, one 32-byte gm_wall_check_point each.
 *   peaks         the largest delta of a changed_pos point and the smallest of a changed_neg point (integer device
 *                 maxima), 0 when there is none.
 * The map is not changed: not its cells, not its totals, not `frames`.  Ordering: a check sees every add enqueued on any
 * slot before it and none enqueued after it (stream events, no host block), so the result is the same bytes on every
 * path.  Scratch per (map, slot) -- 32 B per point of staging sized by the slot's frame, the chained scan's own records,
 * a counter block -- is allocated on first use, kept grow-only and freed with the map. */
enum { GM_WALL_CHECK_MEAN = 0, GM_WALL_CHECK_ENVELOPE = 1 };
enum { GM_WALL_CHECK_CLS_PLANE = 0, GM_WALL_CHECK_CLS_BEYOND_GATE = 1, GM_WALL_CHECK_CLS_OUTSIDE = 2,
       GM_WALL_CHECK_CLS_UNSURVEYED = 3, GM_WALL_CHECK_CLS_UNCHANGED = 4, GM_WALL_CHECK_CLS_CHANGED_POS = 5,
       GM_WALL_CHECK_CLS_CHANGED_NEG = 6, GM_WALL_CHECK_N_CLS = 7 };

typedef struct gm_wall_check_params {
    uint32_t struct_size;     /* = sizeof(gm_wall_check_params) */
    uint32_t reference;       /* GM_WALL_CHECK_MEAN (default) or GM_WALL_CHECK_ENVELOPE */
    uint32_t min_count;       /* >= 1 (default 8): points a cell needs to be usable */
    uint32_t reserved;        /* 0 */
    double   threshold;       /* metres, in (0, 8] with rint(threshold 2^20) >= 1 (default 0.05) */
    double   gate;            /* metres, in (0, 8] (default 1.0): the check's own, not the map's */
} gm_wall_check_params;

typedef struct gm_wall_check_point {   /* 32 bytes: a PointCloud2 row, x y z FLOAT32 at 0, 4, 8 */
    float    x, y, z;         /* the valid cloud's SENSOR coordinates */
    float    delta;           /* (float)(delta 2^-20), metres: exact for |delta| <= 2^24 */
    float    e;               /* the point's residual against the design cylinder */
    int32_t  cell;            /* j * n_sectors + k */
    uint32_t index;           /* into gm_get_cropped_xyz's order */
    uint32_t row;             /* the valid cloud's pad word: the input row (stage call: = index) */
} gm_wall_check_point;

typedef struct gm_wall_check_info {
    uint32_t struct_size;     /* = sizeof(gm_wall_check_info), filled by the library */
    uint32_t status;          /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the design frame's */
    int64_t  threshold_q;     /* T */
    uint32_t n_points;        /* the valid cloud's points = the sum of the seven classes below */
    uint32_t plane, beyond_gate, outside, unsurveyed, unchanged, changed_pos, changed_neg;
    int64_t  peak_pos, peak_neg;   /* 2^-20 m; 0 when the class is empty */
} gm_wall_check_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_check_default_params(gm_wall_check_params *p);
/* Host only, no device, no map: the integer rule applied to one (cell, e) pair, so that a host can restate a row.  It
 * returns, in *cls, GM_WALL_CHECK_CLS_BEYOND_GATE, _UNSURVEYED, _UNCHANGED, _CHANGED_POS or _CHANGED_NEG; plane and
 * outside are not decidable from its inputs (the label and the station are not among them).  *delta is 0 for beyond_gate
 * and unsurveyed.  GM_ERR_INVALID_ARG: a NULL, a struct_size mismatch or a parameter outside its limits. */
gm_status gm_wall_check_classify(const gm_wall_check_params *prm, const gm_wall_raw_cell *cell, float e, int64_t *delta,
                                 uint32_t *cls);
/* Checks the valid cloud of the frame last submitted to `slot` of ctx against the map.  Enqueued on the slot's stream
 * behind the frame's work; returns without waiting.  It reads the point count and the slot's final labels on the device,
 * as the add does; with GM_CFG_GRAPH it is a plain launch after the graph.  Arguments and readiness as for
 * gm_wall_map_add_frame (prm NULL: the defaults; a parameter outside its limits is GM_ERR_INVALID_ARG).  Check followed
 * by add on the same slot is the normal use: check against what was there, then contribute.  add_info may be NULL; its
 * gate is the check's. */
gm_status gm_wall_map_check_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_check_params *prm, gm_wall_add_info *add_info);
/* The result of the last check enqueued on (map, slot).  Waits for that check only (an event recorded behind it, not the
 * slot's stream), then fills info and *n_out (the number of changed points; either may be NULL).  points NULL with
 * capacity 0 is a count query; fewer than *n_out rows of capacity returns GM_ERR_CAPACITY and writes no row.
 * GM_ERR_NOT_READY: no check was enqueued on (map, slot).  The result stays readable until the next check on that
 * (map, slot) -- gm_wall_map_check_points counts as one on slot 0 -- or until the map is destroyed. */
gm_status gm_wall_map_get_check(gm_wall_map *map, uint32_t slot, gm_wall_check_info *info, gm_wall_check_point *points,
                                uint32_t capacity, uint32_t *n_out);
/* The same kernel as one blocking stage call on host buffers (slot 0 of the map's context; gm_wall_map_add_points'
 * conventions).  info, points / capacity / n_out as gm_wall_map_get_check.  The per-point outputs may each be NULL:
 * residual (float[n]: e, NaN for plane points), cell (int32_t[n]: j * n_sectors + k for the four mapped classes, else
 * -1), delta (int32_t[n], saturated; 0 for the classes that have none), cls (uint8_t[n]: GM_WALL_CHECK_CLS_*).
 * row = index.  Fed a slot's valid cloud and labels, it returns that slot's check bit for bit. */
gm_status gm_wall_map_check_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                   const gm_wall_check_params *prm, gm_wall_add_info *add_info, gm_wall_check_info *info,
                                   gm_wall_check_point *points, uint32_t capacity, uint32_t *n_out, float *residual,
                                   int32_t *cell, int32_t *delta, uint8_t *cls);

/* ---- a frame's pose corrected against the wall map (gm_wall_map_locate_*) ----------------------------------------------
 * Every product above bins a point by e = |w| - R under the caller's pose and trusts it: odometry that is 3 cm off
 * laterally puts a cos(phi)-shaped false deviation of that size into every cell an add touches and makes a check report
 * half the wall as changed.  A locate estimates the four degrees of freedom a tube constrains -- the lateral offset of the
 * sensor from the axis (2) and the tilt of the sensor against the axis (2) -- by three gated Gauss-Newton passes over the
 * frame's valid cloud, and returns the corrected pose.  Chainage and roll about the axis are not observable on a smooth
 * wall: they stay the caller's.  The normal order per frame is locate -> check with the corrected pose -> add with it.
 *   start         host, fp64: gm_wall_map_add_frame's "per add" unchanged (the pose checks, j_f, o_f), NOT rounded.  In
 *                 sensor coordinates c = Rm^T (o_f - tr), d = Rm^T a, u' = Rm^T u, v' = Rm^T v; s0 = -c.d, the sensor's
 *                 t, is kept fixed.
 *   pass k        k = 0, 1, 2 with the gate g_k = (float)(gate 2^-k).  The state (c, d, u', v') is rounded to fp32 once
 *                 and reported in pass[k].  Every point runs the add's fp32 chain on those vectors with a local t_min of
 *                 0: q = p - c, t = q.d, w = q - t d, rho = sqrt(w.w), e = rho - R (R rounded to fp32 once).
 *   target        GM_WALL_LOCATE_DESIGN: m = 0; stations and cells are not consulted, so this works on an empty map.
 *                 GM_WALL_LOCATE_MAP: the station j = j_f + floor(t / ds) in 64-bit integers; j outside
 *                 [0, n_stations) is class OUTSIDE; the cell j n_sectors + k (the add's sector k) is USABLE iff
 *                 count >= min_count, else the point is class UNSURVEYED; m = (float)((double) q 2^-20) with
 *                 q = sum / (int64) count by C integer division: the value of the regions and the check, exact in fp32.
 *   classes       every valid point is in exactly one, decided in this order: plane (label 1), gated (e not finite),
 *                 outside, unsurveyed (those two in MAP only), then res = e - m (one fp32 subtraction) and
 *                 used iff |res| < g_k and rho > 0, else gated.
 *   sums          for a used point n = w (1 / rho) (fp32 reciprocal, rounded to nearest), a1 = -n.u', a2 = -n.v' (the fp32
 *                 dot of the chain), J = (a1, a2, t a1, t a2) in fp64; the fp64 sums are the 10 of J_i J_j, the 4 of
 *                 J_i res, the count and res^2, on the fixed grid and in the fixed order of the cylinder regression.  t is
 *                 not recentred: c sits at a station start beside the sensor, so |t| is bounded by the crop box.
 *   solve         fewer than 4 used points: GM_LOCATE_DEGENERATE.  4x4 fp64 Cholesky under the cylinder fit's pivot rule
 *                 (piv > 1e-12 diag, else GM_LOCATE_SINGULAR; so is a step that is not finite): x = -(J^T J)^-1 J^T res.
 *   update        c <- c + x0 u' + x1 v';  d <- normalize(d + x2 u' + x3 v');  u' <- normalize(u' - (u'.d) d);
 *                 v' <- d x u';  then c <- c - (c.d) d - s0 d.  rms = sqrt(sum res^2 / used).
 *   failure       a failed pass sets the status and stops the chain: later passes return at once.  `passes` counts the
 *                 passes that completed; pass[passes] holds the failed pass's frame, gate and class counts with a NaN
 *                 step, the records behind it are zero.  pose, lateral and tilt are NaN.
 *   pose          host, fp64, from the final state: Rm' = [a u v] [d u' v']^T with the columns of the unrounded design
 *                 frame, tr' = o_f - Rm' c.  lateral and tilt are the summed x0, x1 and x2, x3.  |x| of the last pass
 *                 above GM_FIT_STEP_BOUND sets GM_LOCATE_NOT_CONVERGED; the pose is still published.  The pose passes
 *                 the library's own pose check.
 * The map is not changed: not its cells, not its totals, not `frames`.  Ordering as for a check: a locate sees every add
 * enqueued on any slot before it and none enqueued after it.  No floating-point atomics; there is no host round trip
 * between the passes.  Scratch per (map, slot) -- the working state, 96 KiB of partial rows, a pinned copy of the result
 * -- is allocated on first use, kept grow-only and freed with the map; a map that never locates allocates nothing.
 * A locate in MAP mode against a map built from uncorrected poses inherits their mean error: the first survey locates in
 * DESIGN mode. */
enum { GM_WALL_LOCATE_DESIGN = 0, GM_WALL_LOCATE_MAP = 1 };
#define GM_LOCATE_OK            0u
#define GM_LOCATE_DEGENERATE    2u         /* fewer than 4 used points in a pass */
#define GM_LOCATE_SINGULAR      3u         /* a non-positive (or non-finite) Cholesky pivot, or a step that is not finite */
#define GM_LOCATE_FAILED_MASK   0xFFu      /* status & mask != 0: the pose is NaN */
#define GM_LOCATE_NOT_CONVERGED (1u << 8)  /* |last step| > GM_FIT_STEP_BOUND (the pose is still published) */
#define GM_LOCATE_PASSES        3

typedef struct gm_wall_locate_params {
    uint32_t struct_size;     /* = sizeof(gm_wall_locate_params) */
    uint32_t reference;       /* GM_WALL_LOCATE_DESIGN (default) or GM_WALL_LOCATE_MAP */
    uint32_t min_count;       /* >= 1 (default 8): points a cell needs to be usable (MAP) */
    uint32_t reserved;        /* 0 */
    double   gate;            /* metres, in (0, 8] (default 0.25): the gate of pass 0, halved by every later pass */
} gm_wall_locate_params;

typedef struct gm_wall_locate_pass {   /* 112 bytes */
    float    o[3], a[3], u[3], v[3];   /* the pass's state c, d, u', v' in SENSOR coordinates (fp32, as the points saw it) */
    float    gate;                     /* g_k */
    uint32_t plane, outside, unsurveyed, gated, used;   /* the classes: their sum is n_points */
    double   rms;                      /* of res over the used points; NaN when there is none */
    double   step[4];                  /* x: metres along u', v'; radians about them.  NaN for a failed pass */
} gm_wall_locate_pass;

typedef struct gm_wall_locate_info {   /* 488 bytes */
    uint32_t struct_size;     /* = sizeof(gm_wall_locate_info), filled by the library */
    uint32_t status;          /* GM_LOCATE_* */
    uint32_t passes;          /* passes completed: 3 unless the chain failed */
    uint32_t n_points;        /* the valid cloud's points */
    int64_t  anchor_station;  /* j_f of the caller's pose */
    double   pose[12];        /* the corrected pose, row-major 3x4 [Rm' | tr'], sensor -> map */
    double   lateral[2], tilt[2];   /* the total correction along u', v' (metres) and about them (radians) */
    gm_wall_locate_pass pass[GM_LOCATE_PASSES];
} gm_wall_locate_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_locate_default_params(gm_wall_locate_params *p);
/* Host only, no device, no map: GM_OK for parameters a locate accepts; GM_ERR_INVALID_ARG for a NULL, a struct_size
 * mismatch, a reference that is neither of the two, min_count 0 or a gate outside (0, 8] (a NaN included). */
gm_status gm_wall_locate_check_params(const gm_wall_locate_params *p);
/* Locates the valid cloud of the frame last submitted to `slot` of ctx against the map.  Enqueued on the slot's stream
 * behind the frame's work; returns without waiting.  It reads the point count and the slot's final labels on the device,
 * as the add and the check do; with GM_CFG_GRAPH it is plain launches after the graph.  Arguments, errors and readiness as
 * for gm_wall_map_check_frame (prm NULL: the defaults; a bad reference, min_count 0 or a gate outside (0, 8] is
 * GM_ERR_INVALID_ARG). */
gm_status gm_wall_map_locate_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                   const gm_wall_locate_params *prm);
/* The result of the last locate enqueued on (map, slot).  Waits for that locate only (an event recorded behind it, not
 * the slot's stream).  GM_ERR_NOT_READY: no locate was enqueued on (map, slot); GM_ERR_INVALID_ARG: NULL map / info, a bad
 * slot.  The result stays readable until the next locate on that (map, slot) -- gm_wall_map_locate_points counts as one
 * on slot 0. */
gm_status gm_wall_map_get_locate(gm_wall_map *map, uint32_t slot, gm_wall_locate_info *info);
/* The same kernels as one blocking stage call on host buffers (slot 0 of the map's context; gm_wall_map_add_points'
 * conventions).  The per-point outputs may each be NULL and are those of the last pass that ran: residual (float[n]: res,
 * NaN unless the point was used), cell (int32_t[n]: j * n_sectors + k of a point that reached a cell in MAP, else -1;
 * always -1 in DESIGN).  Fed a slot's valid cloud and labels, it returns that slot's locate bit for bit. */
gm_status gm_wall_map_locate_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                    const gm_wall_locate_params *prm, gm_wall_locate_info *info, float *residual, int32_t *cell);

/* ---- a frame's chainage and roll against the wall map (gm_wall_map_align_*) --------------------------------------------
 * A locate leaves chainage and roll about the axis to the caller, because a smooth tube does not constrain them.  A
 * surveyed wall is not smooth: joints, bolts, niches and rough rock are what the map's cell means hold.  An align bins the
 * frame's own deviation image on a patch of cells around the sensor, slides it over the map's image in whole cells, takes
 * the shift of least mean squared mismatch, refines it by a parabola per axis and returns the pose moved by it.  One
 * station of chainage error makes a check compare every point with the wrong cell; the normal order per frame is
 * locate -> align -> check -> add.  Everything from a point's residual e on is integer.
 *   per align     host, fp64: gm_wall_map_add_frame's "per add" unchanged (the pose checks, j_f, o', a', u', v' rounded to
 *                 fp32 once; reported in a gm_wall_add_info).  The gate is the align's own.  P = half_patch_stations,
 *                 A = max_station_shift, B = max_sector_shift, C = (int64) rint(clip 2^20).
 *   per point     the add's fp32 chain unchanged: e, jl = floor(t / ds) relative to the anchor, the sector k.  Classes,
 *                 exactly one per valid point, decided in this order: plane (label 1); beyond_gate (|e| > gate, or e not
 *                 finite); outside_patch (jl not in [-P, P)); binned (everything else).  The patch is anchored on j_f,
 *                 not on the map's extent: a patch station outside [0, n_stations) is still binned and never overlaps.
 *   patch         2P x n_sectors cells, row jr = jl + P.  A cell holds count (u32) and the sum of (int64) rint(e 2^20),
 *                 the integer the add sums.  A patch cell is USABLE iff count >= min_frame_count; its value is
 *                 f = sum / (int64) count by C integer division, toward zero (|f| <= 2^23: |e| <= gate <= 8).
 *   map value     a map cell is USABLE iff count >= min_count; m = sum / (int64) count, the value of the regions, the
 *                 check and the locate, saturated to [-2^30, 2^30] (a cell gm_wall_map_add_raw merged may hold any sum;
 *                 beyond 2^30 the clamp below gives the same Dc either way).
 *   score table   one record per shift (a, b), a in [-A, A] stations, b in [-B, B] sectors, at index
 *                 (a + A)(2B + 1) + (b + B).  The sums run over the patch cells (jr, k) where f is usable,
 *                 j = j_f - P + jr + a lies in [0, n_stations) and the map cell (j, (k + b) mod n_sectors) is usable (the
 *                 modulus taken into [0, n_sectors)):  D = f - m, Dc = clamp(D, -C, C),
 *                 ssd = sum Dc^2, sum_d = sum Dc, n = the cells summed.  C <= 2^23 and n <= 8192, so ssd < 2^60.  The
 *                 table is a function of the patch and the raw map cells alone: not of the grid, the block shape
 *                 (GM_WALL_ALIGN_ROWS) or the order blocks run in.
 *   selection     host (gm_wall_align_select).  A shift is VALID iff n >= min_overlap.  best (a*, b*) has the smallest
 *                 ssd / n, compared exactly by cross-multiplication in 128-bit integers; ties go to the smaller
 *                 max(|a|, |b|), then to the smaller index.  Costs in fp64: c = (double) ssd / (double) n.  The subcell
 *                 fraction, per axis: when both neighbours along the axis are in the table (no wrap) and valid and
 *                 den = c- - 2 c0 + c+ > 0, delta = clamp(0.5 (c- - c+) / den, -0.5, 0.5); otherwise 0.  runner: the
 *                 smallest cost among the valid shifts with max(|a - a*|, |b - b*|) > 1.  distinction = c_runner / c_best,
 *                 +inf when c_best == 0 or there is no runner (rms_runner is then NaN).
 *   results       shift_m = (a* + delta_a) ds;  roll = (b* + delta_b) (2 pi / n_sectors);  bias_m = sum_d 2^-20 / n of the
 *                 best shift;  rms_best, rms_runner = sqrt(c) 2^-20;  overlap = the best shift's n.
 *   status        GM_ALIGN_NO_OVERLAP: no valid shift (in GM_ALIGN_FAILED_MASK: every double of the info is NaN, the
 *                 best shift 0).  GM_ALIGN_AMBIGUOUS: distinction < min_distinction -- the wall here does not tell the
 *                 shifts apart (a smooth lining: about 1.01).  GM_ALIGN_AT_BORDER: |a*| == A > 0 or |b*| == B > 0 -- the
 *                 true shift may lie outside the search.  The pose is still published under both flag bits.
 *   pose          host, fp64.  A patch cell (j, k) that matches the map cell (j + a, k + b) means the frame really sits a
 *                 stations further along and b sectors further round (phi grows from u toward v = a x u).  Q is the
 *                 rotation by `roll` about the design axis a (Rodrigues' formula on the unrounded design frame):
 *                 Rm' = Q Rm,  tr' = o + Q (tr - o) + shift_m a.  The pose passes the library's own pose check.
 * The map is not changed.  Ordering as for a check and a locate: an align sees every add enqueued on any slot before it
 * and none enqueued after it.  No floating-point atomics, no host round trip inside the align.  Scratch per (map, slot) --
 * the patch, the two int32 value images, the table, a pinned copy of the result -- is allocated on first use, kept
 * grow-only and freed with the map; a map that never aligns allocates nothing. */
#define GM_WALL_ALIGN_MAX_PATCH_CELLS 8192u   /* 2P * n_sectors: the bin kernel's LDS table, 12 B per cell = 96 KiB */
#define GM_WALL_ALIGN_MAX_SHIFT       64u     /* A and B */
#define GM_WALL_ALIGN_MAX_SHIFTS      4096u   /* (2A + 1)(2B + 1) */
#define GM_ALIGN_OK          0u
#define GM_ALIGN_NO_OVERLAP  2u          /* no shift with n >= min_overlap */
#define GM_ALIGN_FAILED_MASK 0xFFu       /* status & mask != 0: the pose is NaN */
#define GM_ALIGN_AMBIGUOUS   (1u << 8)   /* distinction < min_distinction (the pose is still published) */
#define GM_ALIGN_AT_BORDER   (1u << 9)   /* the best shift lies on the edge of the search (the pose is still published) */

typedef struct gm_wall_align_params {   /* 56 bytes */
    uint32_t struct_size;          /* = sizeof(gm_wall_align_params) */
    uint32_t half_patch_stations;  /* P >= 1, 2P * n_sectors <= GM_WALL_ALIGN_MAX_PATCH_CELLS (default 20) */
    uint32_t max_station_shift;    /* A in 0 .. 64 (default 8) */
    uint32_t max_sector_shift;     /* B in 0 .. 64, 2B + 1 <= n_sectors (default 4); (2A + 1)(2B + 1) <= GM_WALL_ALIGN_MAX_SHIFTS */
    uint32_t min_count;            /* >= 1 (default 8): points a map cell needs to be usable */
    uint32_t min_frame_count;      /* >= 1 (default 4): points a patch cell needs to be usable */
    uint32_t min_overlap;          /* >= 1 (default 64): cells a shift needs to be valid */
    uint32_t reserved;             /* 0 */
    double   gate;                 /* metres, in (0, 8] (default 0.25) */
    double   clip;                 /* metres, in (0, 8] with rint(clip 2^20) >= 1 (default 0.05): the clamp of D */
    double   min_distinction;      /* >= 1 and finite (default 1.5) */
} gm_wall_align_params;

typedef struct gm_wall_align_score {   /* 24 bytes */
    uint64_t ssd;        /* sum Dc^2 */
    int64_t  sum_d;      /* sum Dc */
    uint32_t n;          /* cells summed */
    uint32_t reserved;   /* 0 */
} gm_wall_align_score;

typedef struct gm_wall_align_info {   /* 224 bytes */
    uint32_t struct_size;     /* = sizeof(gm_wall_align_info), filled by the library */
    uint32_t status;          /* GM_ALIGN_* */
    uint32_t n_points;        /* the valid cloud's points: the sum of the four classes */
    uint32_t plane, beyond_gate, outside_patch, binned;
    uint32_t patch_cells_usable;
    int64_t  anchor_station;  /* j_f of the caller's pose */
    uint32_t half_patch_stations, max_station_shift, max_sector_shift;   /* P, A, B as used */
    uint32_t overlap;         /* the best shift's n */
    int32_t  best_station, best_sector;       /* a*, b* */
    double   frac_station, frac_sector;       /* delta_a, delta_b */
    double   shift_m, roll, bias_m, rms_best, rms_runner, distinction;
    double   pose[12];        /* the aligned pose, row-major 3x4 [Rm' | tr'], sensor -> map */
} gm_wall_align_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_align_default_params(gm_wall_align_params *p);
/* Host only, no device, no map: GM_OK for parameters an align accepts on a map of n_sectors sectors; GM_ERR_INVALID_ARG for
 * a NULL, a struct_size mismatch, n_sectors outside 1 .. GM_WALL_MAX_SECTORS or a parameter outside the limits above (a NaN
 * included). */
gm_status gm_wall_align_check_params(const gm_wall_align_params *p, uint32_t n_sectors);
/* Host only, no device, no map: the selection and the pose of the rule above from a score table of
 * (2A + 1)(2B + 1) records (n_scores must be that).  wall: the map's parameters (its design frame, station_length,
 * n_sectors); prm NULL: the defaults.  Fills status, anchor_station, P, A, B, overlap, the best shift, the fractions, the
 * six results and the pose; the class counts, n_points and patch_cells_usable are the device's and stay 0 here.
 * GM_ERR_INVALID_ARG: a NULL, parameters either check refuses, a pose the library refuses, a wrong n_scores. */
gm_status gm_wall_align_select(const gm_wall_params *wall, const gm_wall_align_params *prm, const double pose[12],
                               const gm_wall_align_score *table, uint32_t n_scores, gm_wall_align_info *info);
/* Aligns the valid cloud of the frame last submitted to `slot` of ctx against the map.  Enqueued on the slot's stream
 * behind the frame's work; returns without waiting.  It reads the point count and the slot's final labels on the device,
 * as the add, the check and the locate do; with GM_CFG_GRAPH it is plain launches after the graph.  Arguments, errors and
 * readiness as for gm_wall_map_check_frame (prm NULL: the defaults; add_info may be NULL, its gate is the align's). */
gm_status gm_wall_map_align_frame(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                  const gm_wall_align_params *prm, gm_wall_add_info *add_info);
/* The result of the last align enqueued on (map, slot).  Waits for that align only (an event recorded behind it, not the
 * slot's stream).  *n_out (may be NULL) is the table's length (2A + 1)(2B + 1).  scores NULL with capacity 0 is a count
 * query; otherwise capacity must hold the table (GM_ERR_CAPACITY).  info may be NULL.  GM_ERR_NOT_READY: no align was
 * enqueued on (map, slot); GM_ERR_INVALID_ARG: NULL map, a bad slot, NULL scores with a capacity.  The result stays
 * readable until the next align on that (map, slot) -- gm_wall_map_align_points counts as one on slot 0. */
gm_status gm_wall_map_get_align(gm_wall_map *map, uint32_t slot, gm_wall_align_info *info, gm_wall_align_score *scores,
                                uint32_t capacity, uint32_t *n_out);
/* The same kernels as one blocking stage call on host buffers (slot 0 of the map's context; gm_wall_map_add_points'
 * conventions).  The per-point outputs may each be NULL: residual (float[n]: e, NaN for plane points), cell (int32_t[n]:
 * jr * n_sectors + k of a binned point, else -1).  Fed a slot's valid cloud and labels, it returns that slot's align bit
 * for bit. */
gm_status gm_wall_map_align_points(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels, const double pose[12],
                                   const gm_wall_align_params *prm, gm_wall_add_info *add_info, gm_wall_align_info *info,
                                   gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out, float *residual,
                                   int32_t *cell);

/* ---- a check's changed points as objects (gm_wall_map_check_objects, gm_wall_check_objects) ---------------------------
 * The changed rows of a check grouped into a short list: "one object, 1.8 m long, between 20 and 44 degrees, 0.5 m inside
 * the profile, at these sensor coordinates".  The result is a function of the MULTISET of rows (gm_wall_check_point), the
 * map's n_stations and n_sectors, an anchor station and the parameters; it does not depend on the order of the rows, the
 * tile shape, the grid or the order blocks run in.  From the decoding of a row on everything is integer; there are no
 * floating-point atomics.
 *   per row     c = cell, j = c / n_sectors, k = c % n_sectors; dq = (int64) rint(delta 2^20) by the check's own rule (fp32
 *               product rounded to nearest even, saturating at the int32 range, 0 for a NaN: exact for the rows a check
 *               wrote); sign = +1 if dq > 0, -1 if dq < 0.  A row is REJECTED if c is outside [0, n_stations n_sectors),
 *               dq == 0 or any of x, y, z, e is not finite (never a check's own row; the stage call can be fed one).
 *   blocks      anchored on the MAP, not on the window, so that a fixed object keeps its label from frame to frame:
 *               bs = block_stations, bk = block_sectors, J = j / bs, K = k / bk, NK = ceil(n_sectors / bk),
 *               B = J NK + K.  The last block in each direction is ragged, as in gm_wall_map_cloud.
 *   window      stations [max(0, j_f - H), min(n_stations, j_f + H)) around the anchor station j_f (int64), H =
 *               half_window_stations, widened to the whole block rows J0 .. J1.  A row whose J lies outside J0 .. J1 is
 *               OUTSIDE_WINDOW; an empty window (an anchor far from the map) makes every row that is not rejected
 *               OUTSIDE_WINDOW.  (J1 - J0 + 1) NK <= GM_WALL_OBJECT_MAX_BLOCKS, else GM_ERR_INVALID_ARG.
 *   planes      positive and negative rows are clustered independently.  cnt_s[B] = rows of sign s in block B; (B, s) is
 *               FLAGGED iff cnt_s[B] >= min_block_points; a row in an unflagged (B, s) is SPARSE.
 *   neighbours  gm_wall_map_regions' rule on the block grid: (J +- 1, K) inside the window, (J, (K +- 1) mod NK) and, with
 *               connectivity 8, (J +- 1, (K +- 1) mod NK).  The sector index wraps, the station index does not.
 *   component   a maximal connected set of flagged blocks of one sign; its LABEL is the smallest B in it, its points the
 *               sum of its cnt_s.  A component of >= min_points points is an OBJECT; the rows of a smaller one are SMALL.
 *   classes     every row is in exactly one of rejected, outside_window, sparse, small, in_object.
 *   record      station and sector extents over the rows' own j and k (the turned ones over (k + n_sectors / 2) mod
 *               n_sectors, as in gm_wall_region); peak = the dq of the largest |dq|, peak_index = that row's `index`, the
 *               smallest index among equals (one 64-bit integer maximum of |dq| << 32 | ~index); sum_delta = the int64 sum of
 *               dq; sum_x, sum_y, sum_z = the int64 sums of (int64) rint(x 2^16) (fp32 product rounded to nearest even,
 *               saturating at the int32 range); box_min, box_max, e_min, e_max = the exact extrema of the sensor
 *               coordinates and of e, taken through ordered() keys (see the raw cells above) with integer maxima.
 *   order       ascending by label, the negative object before the positive one at equal label.
 *   object_of_row[i]  the position in that list of the object row i belongs to, -1 for every other row.
 * On the device: the block counts are zeroed, one thread per row bins (B, s) with integer atomics, a tile of up to 4096
 * window blocks per workgroup flags and labels both planes with a union-find in LDS, the tile borders and the sector seam
 * are joined with agent-scope atomics, the forest is flattened and the roots take slots; after ONE host round trip for the
 * component count every row adds into its slot's accumulator with integer atomics, components are selected at min_points,
 * and, once the host has sorted the list, one thread per row writes object_of_row.  The tile shape (environment
 * GM_WALL_OBJECT_TILE=<block rows>x<block columns>, product <= 4096, read at gm_wall_map_create: tests and measurements)
 * changes nothing in the result. */
#define GM_WALL_OBJECT_MAX_BLOCKS (1u << 20)   /* window blocks of one call */
#define GM_WALL_OBJECT_TILE_ROWS 64u           /* the default tile of the labelling kernel, in blocks */
#define GM_WALL_OBJECT_TILE_COLS 64u

typedef struct gm_wall_object {     /* 128 bytes; every field is independent of the order rows were visited in */
    uint32_t label;                 /* smallest block index B = J * NK + K of the object: its identity */
    int32_t  sign;                  /* +1 farther from the axis than the survey, -1 inside the profile */
    uint32_t blocks;                /* flagged blocks of the component */
    uint32_t peak_index;            /* `index` of the row of the largest |dq|; the smallest index among equals */
    uint32_t station_min, station_max;             /* inclusive, over the rows' j */
    uint32_t sector_min, sector_max;               /* over the rows' k */
    uint32_t sector_min_turned, sector_max_turned; /* over (k + n_sectors / 2) mod n_sectors */
    uint64_t points;                /* rows of the object */
    int64_t  peak;                  /* that row's dq, 2^-20 m */
    int64_t  sum_delta;             /* sum of dq, 2^-20 m */
    int64_t  sum_x, sum_y, sum_z;   /* sums of rint(x 2^16), sensor coordinates, 2^-16 m */
    float    box_min[3], box_max[3];               /* sensor coordinates */
    float    e_min, e_max;          /* the rows' residuals against the design cylinder */
    uint64_t reserved;              /* 0 */
} gm_wall_object;

typedef struct gm_wall_object_params {
    uint32_t struct_size;           /* = sizeof(gm_wall_object_params) */
    uint32_t block_stations;        /* bs >= 1 (default 1) */
    uint32_t block_sectors;         /* bk >= 1 (default 1) */
    uint32_t min_block_points;      /* >= 1 (default 2): rows of one sign a block needs to be flagged */
    uint32_t min_points;            /* >= 1 (default 8): rows a component needs to be an object */
    uint32_t connectivity;          /* 4 or 8 (default 8) */
    uint32_t half_window_stations;  /* H in 1 .. 2^20 (default 128) */
    uint32_t reserved;              /* 0 */
} gm_wall_object_params;

typedef struct gm_wall_objects_info {
    uint32_t struct_size;           /* = sizeof(gm_wall_objects_info), filled by the library */
    uint32_t n_rows;                /* = the sum of the five classes below */
    uint32_t station0, n_stations;  /* the block-aligned window, clipped to the map: stations [J0 bs, min((J1 + 1) bs,
                                       n_stations)); 0, 0 when it is empty */
    uint32_t blocks_stations, blocks_sectors;   /* J1 - J0 + 1 (0 for an empty window), NK */
    uint32_t rejected, outside_window, sparse, small, in_object;   /* rows per class */
    uint32_t flagged_pos, flagged_neg;          /* flagged (block, sign) pairs */
    uint32_t components;            /* before the min_points filter */
    uint32_t objects;               /* after it */
    uint32_t reserved;              /* 0 */
} gm_wall_objects_info;

/* (a struct tag only, no typedef: the function of the same name below fills it) */
struct gm_wall_object_metrics {     /* fp64, derived on the host from one record and the map's parameters */
    double centroid[3];             /* sum 2^-16 / points, sensor coordinates */
    double mean_m;                  /* sum_delta 2^-20 / points */
    double peak_m;                  /* peak 2^-20 */
    double size[3];                 /* box_max - box_min */
    double chainage_from;           /* t_min + station_min * station_length */
    double chainage_to;             /* t_min + (station_max + 1) * station_length */
    double angle_from_deg;          /* gm_wall_region_metrics' rule on the four sector extents */
    double angle_to_deg;
};

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_object_default_params(gm_wall_object_params *p);
/* The objects of the last check enqueued on (map, slot), ascending by (label, sign).  Waits for that check's event only
 * (as gm_wall_map_get_check), takes the row count from the check's counters and the anchor j_f from the check, runs on the
 * map's own stream over the staged rows where they lie -- no row crosses PCIe -- and blocks.  The check's result stays
 * readable, the call may be repeated with other parameters, and neither the map nor the rows are changed.  prm NULL: the
 * defaults.  info is required; it and *n_out (may be NULL; the number of objects) are filled whenever the call got as far
 * as the device, also on GM_ERR_CAPACITY.  objects NULL with capacity 0 is a count query (GM_OK); fewer than *n_out
 * records of capacity returns GM_ERR_CAPACITY and writes no record.  object_of_row (may be NULL, then row_capacity must
 * be 0) receives one int32 per changed row, in the rows' order; a row_capacity below the row count returns
 * GM_ERR_CAPACITY and writes nothing there.  Zero rows or an empty window launch nothing.  Scratch -- 12 B per window block
 * and plane (count, parent, slot), 264 B per component (accumulator, record, two index words), 4 B per row of
 * object_of_row -- is allocated on first use, kept grow-only in the map and freed with it; a map that never asks
 * allocates nothing.
 * GM_ERR_NOT_READY: no check was enqueued on (map, slot).  GM_ERR_INVALID_ARG: NULL map / info, a slot out of range, a
 * struct_size mismatch, a parameter outside its limits, a window above GM_WALL_OBJECT_MAX_BLOCKS blocks, objects NULL with
 * capacity > 0, object_of_row NULL with row_capacity > 0. */
gm_status gm_wall_map_check_objects(gm_wall_map *map, uint32_t slot, const gm_wall_object_params *prm, gm_wall_objects_info *info,
                                    gm_wall_object *objects, uint32_t capacity, uint32_t *n_out, int32_t *object_of_row,
                                    uint32_t row_capacity);
/* The same kernels as one blocking stage call on n_rows host rows in any order (32 B per row of device staging beside the
 * scratch above; the map's cells are not read, only its grid).  object_of_row (may be NULL) holds n_rows entries.  Fed
 * the rows of gm_wall_map_get_check and that check's add_info.anchor_station, it returns gm_wall_map_check_objects'
 * bytes.  GM_ERR_INVALID_ARG as above, and for rows NULL with n_rows > 0. */
gm_status gm_wall_check_objects(gm_wall_map *map, const gm_wall_check_point *rows, uint32_t n_rows, int64_t anchor_station,
                                const gm_wall_object_params *prm, gm_wall_objects_info *info, gm_wall_object *objects,
                                uint32_t capacity, uint32_t *n_out, int32_t *object_of_row);
/* Host only, no device, no map: the fp64 derivation stated at gm_wall_object_metrics from the map's parameters (every
 * operation rounded once).  op may be NULL (the derivation uses the rows' own extents, not the blocks).
 * GM_ERR_INVALID_ARG: a NULL p / o / out, a struct_size mismatch, n_sectors 0, o->points 0 or an extent outside its range. */
gm_status gm_wall_object_metrics(const gm_wall_params *p, const gm_wall_object_params *op, const gm_wall_object *o,
                                 struct gm_wall_object_metrics *out);

/* ---- an add less the check's changed rows (gm_wall_map_add_frame_checked, gm_wall_map_add_points_checked) ---------------
 * A cell is count, sum, min_key, max_key, and integer sums and maxima cannot be taken back: a person at the wall binned
 * once stays in the clearance's innermost point, in the envelope and in the mean for the rest of the map's life.  The map's
 * gate only keeps out what is far from the DESIGN; the check that runs before the add knows what is far from the SURVEY,
 * and its changed rows still lie on the device.  This add leaves out the points those rows name:
 *   params   skip      bits GM_WALL_SKIP_NEG = 1 (rows inside the profile), GM_WALL_SKIP_POS = 2 (rows farther out);
 *                      default 3; 0 or any other bit is GM_ERR_INVALID_ARG
 *            min_delta metres in [0, 8], default 0;  S = (int64) rint(min_delta * 2^20), fp64, once on the host
 *   per row  dq = (int64) rint(delta * 2^20) by gm_wall_map_check_objects' own rule (exact for a check's rows).
 *            REJECTED  if dq == 0, delta not finite, or index >= n_points.
 *            SELECTED  if (dq < 0 and skip & NEG and -dq >= S) or (dq > 0 and skip & POS and dq >= S).
 *            KEPT      otherwise.
 *   per point  SKIPPED if some selected row names its index; otherwise exactly gm_wall_map_add_frame's classes and
 *              updates (plane, beyond_gate under the MAP's gate, outside, mapped).  Skipped is decided first.
 *   map      cells, cells_hit and the four cumulative class totals receive the non-skipped points only; skipped points
 *            enter no total; `frames` counts the call as one add.
 * After a check and a checked add the map's raw cells and totals are, byte for byte, those of gm_wall_map_add_points of
 * the valid cloud with the skipped indices deleted, under the same pose and labels; with no selected row they are
 * gm_wall_map_add_frame's.  On the device: one bit per point of the slot's frame in a mask that is zeroed per call, one
 * thread per staged row marks (a 32-bit atomic OR; the row count is the check's device counter, n_points the device word
 * n_valid: no host round trip), then gm_wall_map_add_frame's kernel in an instantiation that reads one 64-bit mask word
 * per wave and trip.  When to use which add: INTEGRATION.md, "Changed points, node side". */
enum { GM_WALL_SKIP_NEG = 1, GM_WALL_SKIP_POS = 2 };

typedef struct gm_wall_add_checked_params {
    uint32_t struct_size;     /* = sizeof(gm_wall_add_checked_params) */
    uint32_t skip;            /* GM_WALL_SKIP_NEG | GM_WALL_SKIP_POS (default both); not 0 */
    double   min_delta;       /* metres, in [0, 8] (default 0): a selected row has |delta| >= min_delta */
} gm_wall_add_checked_params;

typedef struct gm_wall_add_checked_info {
    uint32_t struct_size;     /* = sizeof(gm_wall_add_checked_info), filled by the library */
    uint32_t status;          /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the design frame's */
    int64_t  min_delta_q;     /* S */
    uint32_t n_points;        /* the valid cloud's points = skipped + plane + beyond_gate + outside + mapped */
    uint32_t n_rows;          /* the rows seen = rows_neg + rows_pos + rows_kept + rows_rejected */
    uint32_t rows_neg, rows_pos;      /* selected rows, by sign */
    uint32_t rows_kept, rows_rejected;
    uint32_t skipped;         /* POINTS some selected row names (rows may name a point twice) */
    uint32_t plane, beyond_gate, outside, mapped;   /* the add's classes over the points that are not skipped */
    uint32_t reserved;        /* 0 */
} gm_wall_add_checked_info;

/* Host only: the defaults of the table above.  A NULL is ignored. */
void gm_wall_add_checked_default_params(gm_wall_add_checked_params *p);
/* Host only: GM_OK iff the block would be accepted (struct_size, skip in 1 .. 3, min_delta in [0, 8]). */
gm_status gm_wall_add_checked_check_params(const gm_wall_add_checked_params *p);
/* gm_wall_map_add_frame less the points that the last check on (map, slot) selected.  Enqueued on the slot's stream behind
 * the frame and behind that check; returns without waiting; with GM_CFG_GRAPH it is plain launches after the graph.
 * Arguments and readiness as gm_wall_map_add_frame (prm NULL: the defaults).  In addition GM_ERR_NOT_READY when no check
 * was enqueued on (map, slot) FOR THE FRAME THE SLOT NOW HOLDS: a check left over from an earlier frame is refused, not
 * applied to another cloud's indices.  The pose need not be the check's.  The check's result stays readable and its rows
 * are not changed.  Other slots' checks, locates and aligns are ordered against it as against a plain add.  Scratch per
 * (map, slot) -- one bit per point of the slot's frame, a counter block -- is allocated on first use, kept grow-only and
 * freed with the map; a map that never asks allocates nothing. */
gm_status gm_wall_map_add_frame_checked(gm_wall_map *map, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_add_checked_params *prm, gm_wall_add_info *add_info);
/* The counts of the last checked add enqueued on (map, slot).  Waits for that call only (an event recorded behind it, not
 * the slot's stream).  GM_ERR_NOT_READY: no checked add was enqueued on (map, slot); GM_ERR_INVALID_ARG: NULL map / info,
 * a slot out of range.  gm_wall_map_add_points_checked does not count as one. */
gm_status gm_wall_map_get_add_checked(gm_wall_map *map, uint32_t slot, gm_wall_add_checked_info *info);
/* The same kernels as one blocking stage call on host buffers (slot 0 of the map's context; gm_wall_map_add_points'
 * conventions).  rows: n_rows gm_wall_check_points in any order, duplicates allowed (NULL with n_rows 0); they are uploaded
 * into scratch of the call's own (32 B per row), so the check result stored for slot 0 is not touched.  info (may be NULL)
 * as gm_wall_map_get_add_checked.  residual / cell (may be NULL) of a skipped point are the e of the add's chain and -1.
 * Fed a slot's valid cloud, labels and gm_wall_map_get_check's rows, it changes the map exactly as the frame call does.
 * GM_ERR_INVALID_ARG: NULL map / xyz with n > 0 / rows with n_rows > 0, bad pose, bad params. */
gm_status gm_wall_map_add_points_checked(gm_wall_map *map, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_add_checked_params *prm,
                                         const gm_wall_check_point *rows, uint32_t n_rows, gm_wall_add_info *add_info,
                                         gm_wall_add_checked_info *info, float *residual, int32_t *cell);

/* ---- a wall map on a circular-arc design axis (gm_wall_map_create_arc) -------------------------------------------------
 * The design axis of such a map is a circular arc of constant curvature in any plane that holds the design direction:
 * horizontal curves, vertical curves (portal ramps) and oblique ones.  An alignment is one map per alignment element,
 * straight (gm_wall_map_create), circular arc or clothoid (gm_wall_map_create_clothoid below).  The table, its cells and every cell-space
 * product are those of a straight map: only the per-point chain and the position rule of the cloud and the mesh see the
 * axis.  One operation per statement; fp64 on the host, not rounded, unless a rounding is named.
 *   design frame  (a, u, v, R) of the straight map's rule above, valid AT params.point, which lies on the axis at chainage
 *                 s0 = point_chainage.  c = curvature - (curvature.a) a;  kappa = |c|;  n = c / kappa;  b = a x n;
 *                 C = point + n / kappa (the centre);  un = u.n, ub = u.b, vn = v.n, vb = v.b (u and v turn with the
 *                 section about b, so the four are constants of the map).  At chainage s, psi = kappa (s - s0):
 *                 a(s) = a cos psi + n sin psi;  n(s) = n cos psi - a sin psi;  P(s) = C - n(s) / kappa;
 *                 u(s) = un n(s) + ub b;  v(s) = vn n(s) + vb b.
 *   refusals      GM_ERR_INVALID_ARG: a curvature entry or point_chainage not finite; kappa < 1e-6 (a flatter curve is a
 *                 straight map); (R + gate) kappa > 0.5; |kappa (t_min - s0)| > 3 or |kappa (t_min + n_stations ds - s0)| > 3.
 *   chainage of x r = x - C;  psi = atan2(r.a, -(r.n));  s = s0 + psi / kappa.
 *   per add       host, fp64.  The pose check of the straight rule.  Sensor chainage s = the chainage of tr; anchor station
 *                 j_f = floor((s - t_min) / ds) as above; s_f = t_min + j_f ds; psi_f = kappa (s_f - s0).  In sensor
 *                 coordinates o' = Rm^T (P(s_f) - tr), a' = Rm^T a(s_f), n' = Rm^T n(s_f), b' = Rm^T b, each rounded to
 *                 fp32 once; kappa, un, ub, vn, vb, R, ds, gate and dtheta rounded to fp32 once: gm_wall_arc_add_info
 *                 (gm_wall_arc_add_frame, host only).  The adds still fill gm_wall_add_info, with u' = Rm^T u(s_f) and
 *                 v' = Rm^T v(s_f) rounded to fp32 once; the device does not read those two.
 *   per point     device, fp32, every operation rounded to nearest (dot products as the chain above: x = fma(qx, a'x,
 *                 fma(qy, a'y, qz a'z))):
 *                   q = p - o';  x = q.a';  y = q.n';  z = q.b'
 *                   cx = kappa x;  cy = fma(-kappa, y, 1);  d = sqrt(fma(cx, cx, cy cy))
 *                   t = atan2f(cx, cy) / kappa
 *                   h = fma(x, x, y y);  yc = fma(-kappa, h, y + y) / (1 + d)      (= (1 - d) / kappa without the cancellation)
 *                   e = sqrt(fma(yc, yc, z z)) - R
 *                   phi = atan2f(fma(yc, vn, z vb), fma(yc, un, z ub)), folded to [0, 2 pi) and binned as above
 *                   j = j_f + floor(t / ds)
 *   classes       as above; in addition a point with cy <= 0 (a quarter turn or more from the anchor section) is beyond_gate.
 *   cloud, mesh   fp64 with the roundings of gm_wall_map_cloud's rule, (c, s) the block's entry of its direction table and
 *                 (cp, sp) = (cos, sin) of psi = kappa (tc - s0) for the block row's centre chainage tc, computed on the
 *                 host per block row:  yc = rho (c un + s vn);  zb = rho (c ub + s vb);  r = yc - 1 / kappa;
 *                 nr_i = n_i cp - a_i sp;  p_i = ((C_i - anchor_i) + r nr_i) + zb b_i, rounded to fp32 once.
 * gm_wall_map_locate_* and gm_wall_map_align_* return GM_ERR_UNSUPPORTED on an arc map: their Jacobians and the "move
 * along the axis" pose assume a straight axis.  The window calls (read, read_raw, add_raw, clear, info, regions,
 * clearance, sections, quantities) are unchanged; a baseline must be a map with a bitwise-equal arc (two straight maps
 * included), else GM_ERR_INVALID_ARG.  The *_metrics helpers stay centreline values: a cell's true area differs from
 * theirs by the factor 1 - kappa yc. */
typedef struct gm_wall_arc {
    uint32_t struct_size;      /* = sizeof(gm_wall_arc) */
    uint32_t reserved;         /* 0 */
    double   curvature[3];     /* map coordinates: points from the axis at `point` toward the centre of curvature,
                                  |.| = 1 / (radius of the axis); its component along the design direction is removed */
    double   point_chainage;   /* chainage of params.point, finite */
} gm_wall_arc;

typedef struct gm_wall_arc_add_info {   /* 120 bytes */
    uint32_t struct_size;      /* = sizeof(gm_wall_arc_add_info), filled by the library */
    uint32_t status;           /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the design frame's */
    int64_t  anchor_station;   /* j_f */
    double   sensor_chainage;  /* s */
    double   anchor_chainage;  /* s_f */
    float    o[3], a[3], n[3], b[3];   /* o', a', n', b' in SENSOR coordinates (fp32, as binned with) */
    float    kappa, un, ub, vn, vb;
    float    R, station_length, sector_angle, gate;
    uint32_t reserved;         /* 0 */
} gm_wall_arc_add_info;

/* gm_wall_map_create with the arc.  GM_ERR_INVALID_ARG also for a NULL arc, a struct_size mismatch and the refusals above. */
gm_status gm_wall_map_create_arc(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_arc *arc, gm_wall_map **map);
/* The map's arc; curvature 0 and point_chainage 0 on a straight map.  GM_ERR_INVALID_ARG: NULL. */
gm_status gm_wall_map_get_arc(gm_wall_map *map, gm_wall_arc *arc);
/* Host only, no context: the four below restate the rules above in fp64 for callers and tests.  GM_ERR_INVALID_ARG: NULL,
 * struct_size mismatch, params or arc refused by gm_wall_map_create_arc, an input that is not finite, a refused pose. */
gm_status gm_wall_arc_check_params(const gm_wall_params *params, const gm_wall_arc *arc);
/* The per-add frame of `pose`. */
gm_status gm_wall_arc_add_frame(const gm_wall_params *params, const gm_wall_arc *arc, const double pose[12],
                                gm_wall_arc_add_info *info);
/* The design frame at `chainage`: o = P(s), a(s), u(s), v(s).  It is (point, direction, up) of the NEXT element's map. */
gm_status gm_wall_arc_frame(const gm_wall_params *params, const gm_wall_arc *arc, double chainage, double o[3], double a[3],
                            double u[3], double v[3]);
/* A map point's chainage, angle phi in [0, 2 pi) and residual e: r = x - C; xa = r.a, xn = r.n, zb = r.b;
 * yc = 1 / kappa - sqrt(xa xa + xn xn); e = sqrt(yc yc + zb zb) - R; phi = atan2(yc vn + zb vb, yc un + zb ub). */
gm_status gm_wall_arc_project(const gm_wall_params *params, const gm_wall_arc *arc, const double xyz[3], double *chainage,
                              double *angle, double *e);
/* The map point at (chainage, angle, rho = R + e): the cloud's position rule with anchor 0 and (c, s) = (cos, sin) angle. */
gm_status gm_wall_arc_point(const gm_wall_params *params, const gm_wall_arc *arc, double chainage, double angle, double rho,
                            double xyz[3]);

/* ---- a wall map on a clothoid design axis (gm_wall_map_create_clothoid) ------------------------------------------------
 * The design axis of such a map is a transition curve: its curvature grows linearly with the chainage, in any plane that
 * holds the design direction.  With it an alignment of straights, clothoids and arcs is one map per element.  Everything
 * said of an arc map holds: only the per-point chain and the position rule of the cloud and the mesh see the axis.  One
 * operation per statement; fp64 on the host, not rounded, unless a rounding is named.  All arithmetic runs in
 * tau = s - s0, never in s, so a map at chainage 5 km evaluates like one at 0.
 *   design frame  (a, u, v, R) of the straight rule AT params.point, which lies on the axis at chainage s0 = point_chainage.
 *                 m = normal - (normal.a) a;  n = m / |m|;  b = a x n;  un = u.n, ub = u.b, vn = v.n, vb = v.b.
 *                 kappa(tau) = curvature + rate tau;  psi(tau) = tau (curvature + (0.5 rate) tau);
 *                 a(s) = a cos psi + n sin psi;  n(s) = n cos psi - a sin psi;  u(s) = un n(s) + ub b;  v(s) = vn n(s) + vb b;
 *                 P(s) = (point + X(tau) a) + Y(tau) n,  (X, Y)(tau) = the integral of (cos psi, sin psi) from 0 to tau.
 *                 The sign of kappa may change inside the map (an S-transition).
 *   quadrature    I(ta, tb), the integral from ta to tb:  K = 1 + floor(min(max(|kappa(ta)|, |kappa(tb)|) |tb - ta| / 0.25,
 *                 4095)) equal panels of width w = (tb - ta) / K, each by the 8-node Gauss-Legendre rule (nodes x_i, weights
 *                 w_i, i ascending in x):  mid = ta + (q + 0.5) w;  sx = sum_i w_i cos psi(mid + (0.5 w) x_i) in the order
 *                 of i;  X += (0.5 w) sx;  Y alike.  A table holds (X, Y) at every station start, built at creation:
 *                 tau_0 = t_min - s0,  T_0 = I(0, tau_0),  tau_j = tau_0 + j ds,  T_(j+1) = T_j + I(tau_j, tau_(j+1)),
 *                 j = 0 .. n_stations.  (X, Y)(tau) = T_jd + I(tau_jd, tau),  jd = floor((tau - tau_0) / ds) clamped to
 *                 [0, n_stations].
 *   refusals      GM_ERR_INVALID_ARG: struct_size or reserved wrong; a field not finite; |m| <= 1e-6 |normal| or 0;
 *                 |rate| (n_stations ds) < 1e-6 (the element is an arc or a straight);  (R + gate) max |kappa| > 0.5 over
 *                 tau in [tau_0, tau_0 + n_stations ds] (kappa is linear: at an end);  |psi| > 3 at either end, or where
 *                 kappa = 0 if that lies strictly inside.
 *   chainage of x r = x - point;  xa = r.a;  xn = r.n.  Start at the tau_j whose T_j is nearest to (xa, xn) (squared distance,
 *                 ties to the lowest j).  Then GM_WALL_CLOTHOID_HOST_STEPS = 6 Newton steps, no data-dependent exit:
 *                 dx = xa - X;  dy = xn - Y;  g = dx cos psi + dy sin psi;  yc = dy cos psi - dx sin psi;
 *                 tau = tau + g / (1 - kappa(tau) yc).  One more evaluation gives the reported yc (and g, which is at most
 *                 1e-10 m over the twin's sweep).  s = s0 + tau.
 *   per add       host, fp64: as on an arc.  Pose check; tau and s = s0 + tau: the chainage of tr;
 *                 j_f = floor((tau - tau_0) / ds) (that is (s - t_min) / ds, taken in tau);  s_f = t_min + j_f ds, and the
 *                 section there is evaluated at tau_0 + j_f ds.  o' = Rm^T (P(s_f) - tr), a' = Rm^T a(s_f), n' = Rm^T n(s_f), b' = Rm^T b, each rounded
 *                 to fp32 once;  kappa_f = kappa(s_f - s0) and rate rounded to fp32 once;  un, ub, vn, vb, R, ds, gate and
 *                 dtheta as on an arc: gm_wall_clothoid_add_info (gm_wall_clothoid_add_frame, host only).
 *                 gm_wall_add_info is filled as on an arc.
 *   per point     device, fp32, every operation rounded to nearest; atan2f as on an arc; (sin, cos) ps by the rule
 *                 k = rint(0.63661977236758134 ps);  r = fma(-k, 1.5703125, ps);  r = fma(-k, 4.837512969970703125e-4, r);
 *                 r = fma(-k, 7.54978995489188216e-8, r);  z = r r;
 *                 S = fma(fma(fma(-1.9515295891e-4, z, 8.3321608736e-3), z, -1.6666654611e-1) z, r, r);
 *                 C = fma(fma(fma(2.443315711809948e-5, z, -1.388731625493765e-3), z, 4.166664568298827e-2) z, z, -0.5 z) + 1;
 *                 (sin, cos) = (S, C), (C, -S), (-S, -C), (-C, S) for k mod 4 = 0, 1, 2, 3;  NaN for |ps| >= 2^20 or a NaN.
 *                   q = p - o';  x = q.a';  y = q.n';  z = q.b'                       (dot products as the chains above)
 *                   cy = fma(-kappa_f, y, 1);  t = |kappa_f| < 1e-6 ? x : atan2f(kappa_f x, cy) / kappa_f    (the arc's t)
 *                   hr = 0.5 rate.  E(t), the evaluation at a trial t, with the 4-node Gauss-Legendre rule on [0, 1]
 *                   (c_i, w_i as fp32 constants):
 *                     sg_i = t c_i;  ps_i = fma(hr, sg_i, kappa_f) sg_i;
 *                     sx = w_0 cos ps_0, then sx = fma(cos ps_i, w_i, sx), i = 1, 2, 3;  sy alike with sin
 *                     dx = x - t sx;  dy = y - t sy;  ps = fma(hr, t, kappa_f) t
 *                     g = fma(dx, cos ps, dy sin ps);  yc = fma(dy, cos ps, -(dx sin ps))
 *                   GM_WALL_CLOTHOID_STEPS = 2 Newton steps:  E(t);  den = fma(-fma(t, rate, kappa_f), yc, 1);
 *                   t = t + g / den.  Then E(t) once more for (g, yc).
 *                   e = sqrt(fma(yc, yc, z z)) - R;  phi and its sector from (yc, z) as on an arc;  j = j_f + floor(t / ds)
 *   classes       as on an arc; in addition beyond_gate: cy <= 0; a den <= 0.25; t or e not finite; a final
 *                 |g| > GM_WALL_CLOTHOID_G_BOUND = 2^-14 m (8 times the worst final |g| of the CPU sweep in
 *                 tests/test_wall_clothoid_np.py, rounded up to a power of two).  Such a point is classed before any
 *                 integer conversion or table index.
 *   cloud, mesh   fp64, (c, s) the block's direction entry; per block row of a chunk the host computes, at the row's centre
 *                 chainage tc, Pa = P(tc) - anchor (per component (point_i + X a_i) + Y n_i, then - anchor_i) and
 *                 (cp, sp) = (cos, sin) psi(tc - s0):  yc = rho (c un + s vn);  zb = rho (c ub + s vb);
 *                 nr_i = n_i cp - a_i sp;  p_i = (Pa_i + yc nr_i) + zb b_i, rounded to fp32 once.
 * gm_wall_map_locate_* and gm_wall_map_align_* return GM_ERR_UNSUPPORTED on a clothoid map, as on an arc map; a baseline
 * must be a map with a bitwise-equal clothoid (and arc), else GM_ERR_INVALID_ARG. */
#define GM_WALL_CLOTHOID_HOST_STEPS 6
#define GM_WALL_CLOTHOID_STEPS 2
#define GM_WALL_CLOTHOID_G_BOUND 6.103515625e-05f   /* 2^-14 */
typedef struct gm_wall_clothoid {
    uint32_t struct_size;      /* = sizeof(gm_wall_clothoid) */
    uint32_t reserved;         /* 0 */
    double   normal[3];        /* map coordinates: the side positive curvature turns toward; its component along the design
                                  direction is removed, then it is normalised */
    double   curvature;        /* signed, 1/m, at params.point (may be 0: the element starts on a straight) */
    double   rate;             /* d(curvature) / d(chainage), signed, 1/m^2 */
    double   point_chainage;   /* chainage of params.point, finite */
} gm_wall_clothoid;

typedef struct gm_wall_clothoid_add_info {   /* 128 bytes */
    uint32_t struct_size;      /* = sizeof(gm_wall_clothoid_add_info), filled by the library */
    uint32_t status;           /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the design frame's */
    int64_t  anchor_station;   /* j_f */
    double   sensor_chainage;  /* s */
    double   anchor_chainage;  /* s_f */
    float    o[3], a[3], n[3], b[3];   /* o', a', n', b' in SENSOR coordinates (fp32, as binned with) */
    float    kappa, un, ub, vn, vb;    /* kappa: kappa_f, the curvature at the anchor section */
    float    R, station_length, sector_angle, gate;
    float    rate;
    uint32_t reserved[2];      /* 0 */
} gm_wall_clothoid_add_info;

/* gm_wall_map_create with the clothoid.  GM_ERR_INVALID_ARG also for a NULL clothoid and the refusals above. */
gm_status gm_wall_map_create_clothoid(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_clothoid *clothoid,
                                      gm_wall_map **map);
/* The map's clothoid; all-zero on other maps.  GM_ERR_INVALID_ARG: NULL. */
gm_status gm_wall_map_get_clothoid(gm_wall_map *map, gm_wall_clothoid *clothoid);
/* Host only, no context: the five below restate the rules above in fp64 for callers and tests (each builds the table of
 * station starts anew: n_stations panels).  GM_ERR_INVALID_ARG: NULL, struct_size mismatch, params or clothoid refused by
 * gm_wall_map_create_clothoid, an input that is not finite, a refused pose. */
gm_status gm_wall_clothoid_check_params(const gm_wall_params *params, const gm_wall_clothoid *clothoid);
/* The per-add frame of `pose`. */
gm_status gm_wall_clothoid_add_frame(const gm_wall_params *params, const gm_wall_clothoid *clothoid, const double pose[12],
                                     gm_wall_clothoid_add_info *info);
/* The design frame at `chainage`: o = P(s), a(s), u(s), v(s), and the signed curvature kappa(s) toward n(s).  It is
 * (point, direction, up) of the NEXT element's map; n(s) goes to `n` (may be NULL), so that a following arc map's
 * gm_wall_arc.curvature is *curvature times n (a negative kappa turns it to the other side, as it should). */
gm_status gm_wall_clothoid_frame(const gm_wall_params *params, const gm_wall_clothoid *clothoid, double chainage, double o[3],
                                 double a[3], double u[3], double v[3], double *curvature, double n[3]);
/* A map point's chainage, angle phi in [0, 2 pi) and residual e by the chainage rule above: zb = r.b;
 * e = sqrt(yc yc + zb zb) - R; phi = atan2(yc vn + zb vb, yc un + zb ub). */
gm_status gm_wall_clothoid_project(const gm_wall_params *params, const gm_wall_clothoid *clothoid, const double xyz[3],
                                   double *chainage, double *angle, double *e);
/* The map point at (chainage, angle, rho = R + e): the cloud's position rule with anchor 0 and (c, s) = (cos, sin) angle. */
gm_status gm_wall_clothoid_point(const gm_wall_params *params, const gm_wall_clothoid *clothoid, double chainage, double angle,
                                 double rho, double xyz[3]);

/* ---- a wall alignment: one wall map per element, chained end to end (gm_wall_alignment_create) --------------------------
 * An alignment is a sequence of up to GM_WALL_ALIGNMENT_MAX_ELEMENTS elements, straight, circular arc or clothoid, each an
 * ordinary wall map of the rules above on one grid (n_sectors, station_length, gate, radius).  The alignment derives every
 * element's map from the end of the one before it, decides per frame which element maps the frame goes to, and adds a frame
 * that straddles joints in ONE launch in which every point is owned by exactly one element.  One operation per statement;
 * fp64 on the host, not rounded, unless a rounding is named.
 *   template      One gm_wall_params describes element 0: the design frame and the chainage t_min at its start, and
 *                 n_sectors, station_length, gate and radius of every element.  Its n_stations is not read (it may be 0).
 *   chaining      host, fp64.  s_start_0 = t_min;  L_i = n_stations_i ds;  s_end_i = s_start_i + L_i;  s_start_(i+1) = s_end_i.
 *                 Element 0 takes the template with its own n_stations.  Element i + 1 takes point = P(s_end_i),
 *                 direction = forward = a(s_end_i) and up = u(s_end_i) of element i: gm_wall_arc_frame's or
 *                 gm_wall_clothoid_frame's (o, a, u) at s_end_i, copied;  on a straight element P = o + (t_min_i + L_i) a
 *                 per component, a and u its design frame's.  With (a, u, v) the design frame of the derived params and
 *                 t = turn / |turn|,  m = t_0 u + t_1 v (per component):
 *                   arc       gm_wall_arc.curvature = curvature m,  point_chainage = t_min = s_start
 *                   clothoid  gm_wall_clothoid.normal = m,  curvature, rate the element's,  point_chainage = t_min = s_start
 *                   straight  t_min = point.a, the chainage the straight rule gives `point` (that rule measures chainage
 *                             from the foot of the map's origin on the axis and has no point_chainage), and the alignment
 *                             keeps the element's offset = s_start - t_min:  alignment chainage = map chainage + offset.
 *                             Element 0 takes the template's t_min as it is (offset 0): its start is o + t_min a.
 *                 The pair (u, v) turns rigidly with the section, so a horizontal left curve is the same `turn` on every
 *                 element and the sector angle is continuous across the joints.  Each element must pass gm_wall_map_create's,
 *                 _create_arc's or _create_clothoid's refusals with its derived structs.
 *   refusals      GM_ERR_INVALID_ARG: NULL; n = 0 or n > GM_WALL_ALIGNMENT_MAX_ELEMENTS; the template refused by
 *                 gm_wall_map_create with n_stations set to 1; an element's struct_size or reserved wrong, kind unknown,
 *                 n_stations = 0; on an arc or a clothoid a turn that is not finite or 0; a derived element refused.
 *   joint i       between elements i and i + 1: the plane through J_i = point of element i + 1 with the normal
 *                 aJ_i = that element's design a.  d_i(x) = (x - J_i).aJ_i.
 *   owner of x    an element looks at its OWN two joints only: element i is a candidate when d_(i-1)(x) >= 0 (none for the
 *                 first element) and d_i(x) < 0 (none for the last).  There is always one: the element before the first
 *                 joint, ascending, with d_i(x) < 0, or the last element -- and on an alignment that nowhere turns a
 *                 quarter turn away from a joint's normal it is the only one.  Where the alignment turns further, x may
 *                 lie between the joints of a distant element too: of several candidates the owner is the one whose
 *                 axis, cut to its span, is nearest to x: with (s, e) the candidate's own project of x,
 *                 over = max(s_start - s, s - s_end, 0);  dist = sqrt((e + R)^2 + over^2);  the smallest dist, ties to the
 *                 lowest index.  (The add below decides among its sides alone, by the joints between them.)
 *   project       owner by the rule above in fp64, then the owner's gm_wall_arc_project / gm_wall_clothoid_project; on a
 *                 straight element r = x - o;  t = r.a;  w = r - t a;  e = |w| - R;  phi = atan2(w.v, w.u) folded to
 *                 [0, 2 pi);  chainage = t + offset.
 *   point         the element with s_start <= chainage < s_end (the first before, the last from the end on), then its
 *                 gm_wall_arc_point / gm_wall_clothoid_point; on a straight element
 *                 x = (o + (chainage - offset) a) + rho (cos phi u + sin phi v) per component.
 *   window        [s_from, s_to], cut to the alignment: per element that it meets in more than a point,
 *                 station0 = floor((max(s_from, s_start) - s_start) / ds),  last = ceil((min(s_to, s_end) - s_start) / ds)
 *                 cut to n_stations,  n_stations = last - station0: whole stations that cover the interval, in order.
 *   per add       host.  The pose check of the straight rule.  (element, s) = project of tr.  Reach
 *                 L = 2 sqrt(3) boxFilterBound + ds, the bound of the clothoid window above.  The sides are the elements
 *                 with s_start < s + L and s_end > s - L, and the sensor's element: consecutive elements.  More than
 *                 GM_WALL_JOINT_MAX_SIDES of them: GM_ERR_UNSUPPORTED, nothing is enqueued.  One side: the add IS that
 *                 element map's add, the same launch.  Two or more: each side gets exactly the per-add frame its own map's
 *                 add computes for this pose (its anchor may lie before station 0 or past the end), and for each joint
 *                 between consecutive sides Jo' = Rm^T (J - tr) and aJ' = Rm^T aJ, each rounded to fp32 once.
 *   per point     device, fp32, every operation rounded to nearest.  For the joints of the sides, ascending:  q = p - Jo'_i;
 *                 d_i = fma(qx, ax, fma(qy, ay, qz az)).  The owner is the side before the first joint with d_i < 0, the
 *                 last side if there is none (a NaN is not < 0).  The point runs its owner's chain and no other, and is
 *                 classed and binned as an add of it alone to the owner's map under the same pose would: a point that the
 *                 owner's chain places past the owner's end is `outside` in the owner's totals, nothing is clamped.
 * So an alignment add changes every element map exactly as gm_wall_map_add_points of the sub-cloud that element owns would,
 * and every point is classed exactly once.  The LDS table's GM_SURF_MAX_CELLS cells are dealt to the sides in order (a
 * side's window: the stations of its own add's window that lie in the element, cut to what is left); a mapped point outside
 * its side's window goes to the map directly, which affects speed only.
 * Out of scope: element maps of different grids; closed loops.  The locate is gm_wall_alignment_locate_*, the align
 * (chainage and roll) gm_wall_alignment_align_*, the check and the checked add gm_wall_alignment_check_* and
 * gm_wall_alignment_add_*_checked, a check's objects gm_wall_alignment_check_objects below. */
#define GM_WALL_ALIGNMENT_MAX_ELEMENTS 256
#define GM_WALL_JOINT_MAX_SIDES 4
enum { GM_WALL_ELEMENT_STRAIGHT = 0, GM_WALL_ELEMENT_ARC = 1, GM_WALL_ELEMENT_CLOTHOID = 2 };
typedef struct gm_wall_element {   /* 48 bytes */
    uint32_t struct_size;      /* = sizeof(gm_wall_element) */
    uint32_t kind;             /* GM_WALL_ELEMENT_* */
    uint32_t n_stations;       /* >= 1 */
    uint32_t reserved;         /* 0 */
    double   turn[2];          /* arc, clothoid: the side positive curvature turns toward, in the (u, v) basis of the element's
                                  START section; non-zero, normalised by the library; not read on a straight */
    double   curvature;        /* arc: > 0; clothoid: signed, at the element's start; straight: not read */
    double   rate;             /* clothoid only */
} gm_wall_element;

typedef struct gm_wall_alignment gm_wall_alignment;   /* opaque; owned by the context it was created from */

typedef struct gm_wall_alignment_piece {   /* 16 bytes */
    uint32_t element, station0, n_stations;
    uint32_t reserved;         /* 0 */
} gm_wall_alignment_piece;

typedef struct gm_wall_alignment_add_info {   /* 160 bytes; filled on the host by every add, before the kernel has run */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_add_info), filled by the library */
    uint32_t status;           /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the OR of the sides' design frames' */
    uint32_t element;          /* the sensor's element */
    uint32_t n_sides;          /* 1 .. GM_WALL_JOINT_MAX_SIDES */
    double   chainage;         /* the sensor's chainage s */
    double   reach;            /* L */
    uint32_t side_element[GM_WALL_JOINT_MAX_SIDES];   /* ascending, consecutive; entries from n_sides on are 0 */
    int64_t  side_anchor[GM_WALL_JOINT_MAX_SIDES];    /* j_f of each side's own add */
    float    joint_o[GM_WALL_JOINT_MAX_SIDES - 1][3]; /* Jo' of the joint behind side i, as the kernel receives it */
    float    joint_a[GM_WALL_JOINT_MAX_SIDES - 1][3]; /* aJ' */
    double   offset;           /* the sensor element's chainage offset (0 unless a straight element behind the first) */
} gm_wall_alignment_add_info;

typedef struct gm_wall_alignment_totals {   /* 72 bytes; cumulative, read after a synchronisation */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_totals), filled by the library */
    uint32_t n_elements;
    uint64_t n_stations;       /* summed over the elements */
    double   chainage_min, chainage_max;   /* s_start of the first element, s_end of the last */
    uint64_t frames;           /* the element maps' frames, summed: an add counts once per side */
    uint64_t mapped, outside, beyond_gate, plane;   /* the element maps' class totals, summed */
} gm_wall_alignment_totals;

/* Host only, no context.  GM_ERR_INVALID_ARG: NULL, the refusals above, an input that is not finite, a refused pose;
 * GM_ERR_OOM: no memory for the elements or a clothoid's table.  Each of the six calls chains the alignment anew -- every
 * element's frame, and each clothoid element's table of station starts (n_stations panels) -- so a call costs about a
 * microsecond per element plus a few per hundred clothoid stations, per point for project and point: fine for a pose, a
 * window or a synthetic frame, not for a cloud per frame. */
gm_status gm_wall_alignment_check(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n);
/* The derived structs of element i, what gm_wall_map_create / _create_arc / _create_clothoid take to create a bitwise-equal
 * map: *out always; *arc on an arc element, zeroed otherwise; *clothoid on a clothoid element, zeroed otherwise (either may
 * be NULL).  The element's s_start is the template's t_min plus the lengths before it. */
gm_status gm_wall_alignment_element_params(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, uint32_t i,
                                           gm_wall_params *out, gm_wall_arc *arc, gm_wall_clothoid *clothoid);
/* A map point's owner, alignment chainage, angle phi in [0, 2 pi) and residual e (the project rule above). */
gm_status gm_wall_alignment_project(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, const double xyz[3],
                                    uint32_t *element, double *chainage, double *angle, double *e);
/* The map point at (chainage, angle, rho = R + e) (the point rule above). */
gm_status gm_wall_alignment_point(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, double chainage,
                                  double angle, double rho, double xyz[3]);
/* The plan of an add under `pose` on a context whose boxFilterBound is `bound` (> 0, finite): the sensor's element and
 * chainage, the sides and the fp32 joint planes exactly as the kernel receives them.  GM_ERR_UNSUPPORTED: more than
 * GM_WALL_JOINT_MAX_SIDES sides (info is filled but for the sides and the joints). */
gm_status gm_wall_alignment_add_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                     const double pose[12], double bound, gm_wall_alignment_add_info *info);
/* The pieces of [s_from, s_to] (finite, s_from <= s_to), the window rule above; *n_out: their number.  GM_ERR_CAPACITY: more
 * than `capacity` (pieces may be NULL with capacity 0).  A product over a chainage interval runs once per piece on
 * gm_wall_alignment_map(al, piece.element) with (piece.station0, piece.n_stations). */
gm_status gm_wall_alignment_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n, double s_from,
                                   double s_to, gm_wall_alignment_piece *pieces, uint32_t capacity, uint32_t *n_out);

/* The alignment and its n element maps on ctx's device.  GM_ERR_INVALID_ARG: NULL, the refusals above; GM_ERR_OOM;
 * GM_ERR_DEVICE.  It belongs to the context and is freed with it. */
gm_status gm_wall_alignment_create(gm_ctx *ctx, const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                   gm_wall_alignment **alignment);
/* Waits for the adds and frees the alignment and its element maps.  NULL is ignored. */
void gm_wall_alignment_destroy(gm_wall_alignment *alignment);
/* Element i's ordinary gm_wall_map, owned by the alignment (it must not be destroyed by the caller): every window call and
 * every per-slot call works on it, ordered against the alignment's adds as against its own. */
gm_status gm_wall_alignment_map(gm_wall_alignment *alignment, uint32_t i, gm_wall_map **map);
/* gm_wall_map_add_frame on the alignment: enqueued on the slot's stream behind the frame's work; for every side's map it
 * does what an add does (it waits for readers on other slots and marks the slot pending).  info may be NULL. */
gm_status gm_wall_alignment_add_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                      gm_wall_alignment_add_info *info);
/* gm_wall_map_add_points on the alignment.  residual, cell, element may be NULL; cell is relative to the owner's map and
 * element (int32_t[n]) is the owner's element index, set for every point. */
gm_status gm_wall_alignment_add_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                       const double pose[12], gm_wall_alignment_add_info *info, float *residual, int32_t *cell,
                                       int32_t *element);
/* gm_wall_map_sync on every element map. */
gm_status gm_wall_alignment_sync(gm_wall_alignment *alignment);
/* Synchronises, then the sums above. */
gm_status gm_wall_alignment_info(gm_wall_alignment *alignment, gm_wall_alignment_totals *info);

/* ---- a frame's pose corrected against a wall alignment (gm_wall_alignment_locate_*) ------------------------------------
 * gm_wall_map_locate_* on the alignment: the same four degrees of freedom, the same three gated Gauss-Newton passes, the
 * same parameters (gm_wall_locate_params, gm_wall_locate_check_params), statuses (GM_LOCATE_*) and GM_FIT_STEP_BOUND, on
 * straight, arc and clothoid elements and across their joints.  A single-element alignment is the locate of a lone arc or
 * clothoid map (gm_wall_map_locate_* keeps refusing those).  Per frame on an alignment: locate here ->
 * gm_wall_alignment_check_frame with the corrected pose -> gm_wall_alignment_add_frame_checked with it.  One operation per
 * statement.
 *   plan          host, fp64: gm_wall_alignment_add_plan's, unchanged: the sensor's ("home") element, the sides within the
 *                 reach, each side's own per-add frame, the joint planes.  More than GM_WALL_JOINT_MAX_SIDES sides:
 *                 GM_ERR_UNSUPPORTED, nothing is enqueued.  ONE side that is a straight element: the locate IS
 *                 gm_wall_map_locate_* of that element map, the same launches; the info's first 152 bytes (but for
 *                 struct_size) and each pass record's first 112 are gm_wall_locate_info's and gm_wall_locate_pass's, byte
 *                 for byte; the record's side block 0 repeats (o, a, u, v).  Everything below is the other plans'.
 *   start         host, fp64, not rounded.  (o_f, a, u, v): the home element's section at its anchor chainage s_f, from
 *                 gm_wall_arc_frame, gm_wall_clothoid_frame (evaluated in tau, as its per-add rule) or the straight frame
 *                 (o_f = o + (t_min + j_f ds) a).  The state is that section in sensor coordinates: c = Rm^T (o_f - tr),
 *                 d = Rm^T a, u' = Rm^T u, v' = Rm^T v;  s0 = -c.d is kept fixed.
 *   attached      host, fp64, once per locate.  Every vector of every side's per-add block -- o', a', n', b' of a curved
 *                 side at ITS anchor section, o', a', u', v' of a straight side -- and of every joint plane (J, aJ) is
 *                 expressed in the home section: a point X as h = ((X - o_f).a, (X - o_f).u, (X - o_f).v), a direction D as
 *                 h = (D.a, D.u, D.v).  The home side's own o and a are h = (0, 0, 0) and (1, 0, 0) exactly, and on a
 *                 straight home side u, v are (0, 1, 0) and (0, 0, 1).  kappa_f, rate, un, ub, vn, vb (rounded to fp32 once,
 *                 as the side's add has them) and the anchor stations do not move.
 *   image         of an attached vector under a state, fp64: a point c + ((h0 d + h1 u') + h2 v'), a direction
 *                 (h0 d + h1 u') + h2 v', per component; rounded to fp32 once.
 *   pass k        k = 0, 1, 2 with the gate g_k = (float)(gate 2^-k).  The state is rounded to fp32 once and reported in
 *                 pass[k].o, a, u, v; every side's block and every joint plane is the image under the pass's state and is
 *                 reported in pass[k].side and pass[k].joint_o / joint_a.  Pass 0's are computed by the host and travel in
 *                 the launch arguments; after pass k the thread that solves it writes those of pass k + 1.
 *   per point     device, fp32, every operation rounded to nearest.
 *                 owner   the add's rule on the pass's planes:  q = p - Jo'_i;  d_i = fma(qx, ax, fma(qy, ay, qz az));  the
 *                         side before the first joint, ascending, with d_i < 0, else the last side.
 *                 chain   the owner's alone, on its block of the pass, exactly the add's chain of that axis above:
 *                         straight  q, t, w of the locate's chain above;  rho = sqrt(fma(wx, wx, fma(wy, wy, wz wz))),
 *                                   the root rounded to nearest as on the curved sides;  e = rho - R;
 *                                   nrm = w (1 / rho) (fp32 reciprocal, rounded to nearest);  guard: none.
 *                         arc       x, y, z, cx, cy, d, t, yc of the arc rule;  rho = sqrt(fma(yc, yc, z z));  e = rho - R;
 *                                   cs = cy / d;  sn = cx / d;  guard: cy > 0.
 *                         clothoid  x, y, z, t, g, yc of the clothoid rule;  rho and e alike;  (sn, cs) = the (sin, cos) of
 *                                   ps in the closing E(t);  guard: the clothoid rule's (cy > 0, every den > 0.25, t finite,
 *                                   |g| <= GM_WALL_CLOTHOID_G_BOUND).
 *                         curved    nt_i = fma(cs, n'_i, -(sn a'_i));  nrm_i = fma(yc, nt_i, z b'_i) (1 / rho)  (the same
 *                                   reciprocal): the unit radial direction (yc n(t) + z b) / rho in sensor coordinates.
 *                 target  GM_WALL_LOCATE_DESIGN: m = 0.  GM_WALL_LOCATE_MAP: j = the owner's j_f + floor(t / ds) in 64-bit
 *                         integers against the owner's n_stations; the sector by the owner's rule (a straight side from
 *                         (w.v', w.u') of its block, a curved side from (yc, z) and its un, ub, vn, vb); count, sum and the
 *                         min_count and sum / count rules of gm_wall_map_locate_* on the OWNER's table.
 *                 classes in this order: plane (label 1); gated (e not finite, or the guard fails: before any integer
 *                         conversion or table index); outside, unsurveyed (MAP only); res = e - m;  used iff |res| < g_k and
 *                         rho > 0, else gated.
 *   sums          for a used point, fp64 from the fp32 values nrm, p and the pass's fp32 state (o, a, u, v):
 *                 c0_i = o_i + s0 a_i;  q = p - c0;  J = -(nrm.u, nrm.v, nrm.(v x q), -(nrm.(u x q))), dot and cross products
 *                 in the order x, y, z.  These are the lateral offset along u', v' and the tilt of d toward u', v', the tilt
 *                 turning the map about the sensor's own foot c0 (on a straight side the columns span (a1, a2, t a1, t a2)
 *                 of gm_wall_map_locate_*: J_3 = (t - s0) a1).  The 10 J_i J_j, the 4 J_i res, the count and res^2, their
 *                 grid and order, the solve, its pivot rule and its failures are gm_wall_map_locate_*'s.
 *   update        c0 = c + s0 d + x0 u' + x1 v';  d <- normalize(d + x2 u' + x3 v');  u' <- normalize(u' - (u'.d) d);
 *                 v' <- d x u';  c <- c0 - (c0.d) d - s0 d.  (That is gm_wall_map_locate_*'s update of the same correction.)
 *                 Every attached vector follows by its image.
 *   pose          host, fp64: Rm' = [a u v] [d u' v']^T with the home section's unrounded columns, tr' = o_f - Rm' c;
 *                 lateral, tilt, GM_LOCATE_NOT_CONVERGED and the failure rules as gm_wall_map_locate_*.
 * The element maps are not changed.  Ordering as for a check, against every side's map: the locate sees every add enqueued
 * before it on any slot, through the alignment or through an element map, and none enqueued after it.  No floating-point
 * atomics, no host round trip between the passes, one pending result per (alignment, slot).  Scratch per (alignment,
 * slot) -- the working state, 96 KiB of partial rows, a pinned copy of the result -- and the stage call's three per-point
 * arrays are allocated on first use, kept grow-only and freed with the alignment; an alignment that never locates across
 * a joint or on a curved element allocates nothing.  Out of scope: chainage and roll: they are gm_wall_alignment_align_*'s
 * below. */
typedef struct gm_wall_alignment_locate_pass {   /* 376 bytes; the first 112 are gm_wall_locate_pass */
    float    o[3], a[3], u[3], v[3];   /* the pass's state c, d, u', v' in SENSOR coordinates (fp32, as the points saw it) */
    float    gate;                     /* g_k */
    uint32_t plane, outside, unsurveyed, gated, used;   /* the classes over all sides: their sum is n_points */
    double   rms;
    double   step[4];
    float    side[GM_WALL_JOINT_MAX_SIDES][12];         /* per side o', a', n', b' (straight: o', a', u', v') of the pass */
    float    joint_o[GM_WALL_JOINT_MAX_SIDES - 1][3];   /* Jo' of the pass */
    float    joint_a[GM_WALL_JOINT_MAX_SIDES - 1][3];   /* aJ' */
} gm_wall_alignment_locate_pass;

typedef struct gm_wall_alignment_locate_info {   /* 1448 bytes; the first 152 are gm_wall_locate_info's */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_locate_info), filled by the library */
    uint32_t status;           /* GM_LOCATE_* */
    uint32_t passes;
    uint32_t n_points;
    int64_t  anchor_station;   /* j_f of the home side */
    double   pose[12];         /* the corrected pose, row-major 3x4 [Rm' | tr'], sensor -> map */
    double   lateral[2], tilt[2];
    uint32_t element;          /* the home element */
    uint32_t n_sides;
    uint32_t side_element[GM_WALL_JOINT_MAX_SIDES];   /* as gm_wall_alignment_add_info */
    uint32_t side_kind[GM_WALL_JOINT_MAX_SIDES];      /* GM_WALL_ELEMENT_* */
    int64_t  side_anchor[GM_WALL_JOINT_MAX_SIDES];
    float    side_axis[GM_WALL_JOINT_MAX_SIDES][6];   /* kappa_f, rate, un, ub, vn, vb as the chains took them (0 where unused) */
    gm_wall_alignment_locate_pass pass[GM_LOCATE_PASSES];
} gm_wall_alignment_locate_info;

typedef struct gm_wall_alignment_locate_start {   /* 1008 bytes: what a locate starts from, host only */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_locate_start), filled by the library */
    uint32_t home;             /* the home element's index among the sides */
    gm_wall_alignment_add_info add;   /* the plan of the add under the same pose */
    double   c[3], d[3], u[3], v[3];  /* the start, sensor coordinates */
    double   s0;
    double   o_f[3], a[3], fu[3], fv[3];   /* the home section in map coordinates, not rounded */
    double   side[GM_WALL_JOINT_MAX_SIDES][12];      /* h of each side's four vectors */
    double   joint[GM_WALL_JOINT_MAX_SIDES - 1][6];  /* h of J and of aJ */
    float    side_axis[GM_WALL_JOINT_MAX_SIDES][6];
    uint32_t side_kind[GM_WALL_JOINT_MAX_SIDES];
} gm_wall_alignment_locate_start;

/* Host only, no context: the start, the attached vectors and the constants of a locate under `pose` on a context whose
 * boxFilterBound is `bound`.  Errors as gm_wall_alignment_add_plan. */
gm_status gm_wall_alignment_locate_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                        const double pose[12], double bound, gm_wall_alignment_locate_start *start);
/* gm_wall_map_locate_frame on the alignment (prm NULL: the defaults).  GM_ERR_INVALID_ARG: NULL, a foreign context, a bad
 * slot, bad parameters, a refused pose; GM_ERR_NOT_READY: the slot holds no frame; GM_ERR_UNSUPPORTED: too many sides. */
gm_status gm_wall_alignment_locate_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                         const gm_wall_locate_params *prm);
/* The result of the last locate enqueued on (alignment, slot); waits for that locate only.  GM_ERR_NOT_READY: none was
 * enqueued; GM_ERR_INVALID_ARG: NULL, a bad slot.  gm_wall_alignment_locate_points counts as a locate on slot 0. */
gm_status gm_wall_alignment_get_locate(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_locate_info *info);
/* The same kernels as one blocking stage call on host buffers (slot 0).  The per-point outputs may each be NULL and are
 * those of the last pass that ran: residual (res, NaN unless used), cell (relative to the map of that pass's owner, -1
 * unless the point reached a cell in MAP); element is the owner's element index in pass 0, set for every point: the owner
 * under the caller's pose, which is gm_wall_alignment_add_points' under the same pose. */
gm_status gm_wall_alignment_locate_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                          const double pose[12], const gm_wall_locate_params *prm,
                                          gm_wall_alignment_locate_info *info, float *residual, int32_t *cell, int32_t *element);

/* ---- a frame's changed points against a wall alignment, and the add less them (gm_wall_alignment_check_*,
 * gm_wall_alignment_add_*_checked) ------------------------------------------------------------------------------------------
 * gm_wall_map_check_* and gm_wall_map_add_*_checked on the alignment: the same parameters (gm_wall_check_params,
 * gm_wall_add_checked_params), the same seven classes, the same 32-byte row, across the joints.  Per frame on an alignment:
 * gm_wall_alignment_locate_frame -> gm_wall_alignment_check_frame with the located pose -> gm_wall_alignment_add_frame_checked.
 *   per check     host, fp64.  The plan is gm_wall_alignment_add_plan's for this pose, unchanged: the sensor's element, the
 *                 sides within the reach L, the fp32 joint planes Jo', aJ'; it is reported in a gm_wall_alignment_add_info.
 *                 Each side's per-add frame is the one its own map's CHECK computes: the add's frame, except that the gate
 *                 is the check's parameter rounded to fp32 once.  More than GM_WALL_JOINT_MAX_SIDES sides:
 *                 GM_ERR_UNSUPPORTED, nothing is enqueued.  Parameters and their refusals are gm_wall_check_params'.
 *   per point     device, fp32.  The owner by the add's rule:  q = p - Jo'_i;  d_i = fma(qx, ax, fma(qy, ay, qz az)) over
 *                 the joints in ascending order; the side before the first d_i < 0, else the last side.  The point runs its
 *                 owner's chain alone (straight, arc or clothoid, as gm_wall_map_check_* of that map runs it) under the
 *                 check's gate, and a mapped point takes the check's integer rule against the OWNER's table: the count
 *                 first, then sum or keys only for a usable cell.  Every valid point is in exactly one of the seven
 *                 classes, and the class counts are kept per side.
 *   rows          gm_wall_check_point, ascending by index in the valid cloud, from the one launch.  cell holds
 *                 side << 24 | cell: the low 24 bits are the cell in the owner's map (a cell is < 2^24), side indexes
 *                 side_element[] of the check's plan (GM_WALL_ROW_SIDE, GM_WALL_ROW_CELL).  With one side this is the
 *                 element map's row, byte for byte.
 *   one side      the check IS that element map's gm_wall_map_check_frame / _check_points: the same launch, the shared
 *                 fields byte for byte; gm_wall_alignment_get_check then reads that map's result.
 *   ordering      no map is changed.  The check sees every add enqueued before it on any slot of every side's map, through
 *                 the alignment or through an element map, and none enqueued after: a later add on any slot waits for it
 *                 through the alignment's pending results, as for a locate.
 *   checked add   gm_wall_map_add_*_checked's parameters, row classes (rejected, selected, kept) and
 *                 gm_wall_add_checked_info, unchanged.  A row is read for delta and index only: the side bits of cell do not
 *                 matter.  The add plan is computed for the add's own pose, which need not be the check's; its sides need
 *                 not be the check's sides.  Point i is skipped iff a selected row names it, decided before ownership;
 *                 every element map then changes exactly as gm_wall_map_add_points of the sub-cloud it owns with the
 *                 skipped indices deleted, and with no selected row the result is gm_wall_alignment_add_frame's.  `frames`
 *                 counts once per side; skipped points enter no total.  The info's status is the OR of the sides'.
 * The frame call takes the rows of the last check enqueued THROUGH THE ALIGNMENT on that slot, wherever they are staged (a
 * one-side check: the element map's buffer), and returns GM_ERR_NOT_READY when there is none for the frame the slot now
 * holds, or when a check on that element map itself has since replaced a one-side check's rows.  Scratch per (alignment,
 * slot) -- 32 B per point of staging, the scan records, the counter block, one mask bit per point, pinned copies of the
 * results -- is allocated by the first call that is not an element map's own, kept grow-only and freed with the alignment;
 * an alignment that never checks allocates nothing. */
#define GM_WALL_ROW_SIDE(cell) ((uint32_t)(cell) >> 24)
#define GM_WALL_ROW_CELL(cell) ((uint32_t)(cell) & 0xFFFFFFu)
typedef struct gm_wall_alignment_check_info {   /* 184 bytes; filled by gm_wall_alignment_get_check / _check_points */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_check_info), filled by the library */
    uint32_t status;           /* GM_SURF_OK or GM_SURF_UP_FALLBACK: the OR of the sides' design frames' */
    int64_t  threshold_q;      /* T */
    uint32_t n_points;         /* the valid cloud's points = the sum of the seven classes below */
    uint32_t plane, beyond_gate, outside, unsurveyed, unchanged, changed_pos, changed_neg;   /* summed over the sides */
    int64_t  peak_pos, peak_neg;   /* 2^-20 m over all sides; 0 when the class is empty */
    uint32_t n_sides;          /* of the check's plan */
    uint32_t reserved;         /* 0 */
    uint32_t side_class[GM_WALL_JOINT_MAX_SIDES][GM_WALL_CHECK_N_CLS];   /* GM_WALL_CHECK_CLS_* order; 0 from n_sides on */
} gm_wall_alignment_check_info;

/* gm_wall_map_check_frame on the alignment (prm NULL: the defaults).  plan may be NULL.  GM_ERR_INVALID_ARG: NULL, a foreign
 * context, a bad slot, bad parameters, a refused pose; GM_ERR_NOT_READY: the slot holds no frame; GM_ERR_UNSUPPORTED: too
 * many sides. */
gm_status gm_wall_alignment_check_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_check_params *prm, gm_wall_alignment_add_info *plan);
/* The result of the last check enqueued on (alignment, slot), as gm_wall_map_get_check: waits for that check only; info,
 * n_out may be NULL; points NULL with capacity 0 is a count query; GM_ERR_CAPACITY writes no row.  GM_ERR_NOT_READY: none
 * was enqueued; GM_ERR_INVALID_ARG: NULL, a bad slot.  gm_wall_alignment_check_points counts as a check on slot 0. */
gm_status gm_wall_alignment_get_check(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_check_info *info,
                                      gm_wall_check_point *points, uint32_t capacity, uint32_t *n_out);
/* The same kernel as one blocking stage call on host buffers (slot 0).  The per-point outputs may each be NULL: residual
 * (e, NaN for plane points), cell (relative to the owner's map, -1 if unmapped), delta (saturated), cls
 * (GM_WALL_CHECK_CLS_*), element (the owner's element index, set for every point).  row = index. */
gm_status gm_wall_alignment_check_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_check_params *prm, gm_wall_alignment_add_info *plan,
                                         gm_wall_alignment_check_info *info, gm_wall_check_point *points, uint32_t capacity,
                                         uint32_t *n_out, float *residual, int32_t *cell, int32_t *delta, uint8_t *cls,
                                         int32_t *element);
/* gm_wall_alignment_add_frame less the points that the last check on (alignment, slot) selected (prm NULL: the defaults).
 * Errors as gm_wall_alignment_add_frame and gm_wall_map_add_frame_checked.  plan may be NULL. */
gm_status gm_wall_alignment_add_frame_checked(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                              const gm_wall_add_checked_params *prm, gm_wall_alignment_add_info *plan);
/* The counts of the last checked add enqueued on (alignment, slot); waits for that call only.  GM_ERR_NOT_READY: none was
 * enqueued; GM_ERR_INVALID_ARG: NULL, a bad slot.  gm_wall_alignment_add_points_checked does not count as one. */
gm_status gm_wall_alignment_get_add_checked(gm_wall_alignment *alignment, uint32_t slot, gm_wall_add_checked_info *info);
/* The same kernels as one blocking stage call on host buffers (slot 0).  rows: n_rows gm_wall_check_points in any order,
 * duplicates allowed (NULL with n_rows 0).  plan, info, residual, cell, element may be NULL; residual / cell of a skipped
 * point are the e of its owner's chain and -1. */
gm_status gm_wall_alignment_add_points_checked(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                               const double pose[12], const gm_wall_add_checked_params *prm,
                                               const gm_wall_check_point *rows, uint32_t n_rows, gm_wall_alignment_add_info *plan,
                                               gm_wall_add_checked_info *info, float *residual, int32_t *cell, int32_t *element);

/* ---- a frame's chainage and roll against a wall alignment (gm_wall_alignment_align_*) -----------------------------------
 * gm_wall_map_align_* on the alignment: the same parameters (gm_wall_align_params), integer rule, statuses (GM_ALIGN_*) and
 * score table, on straight, arc and clothoid elements and across their joints.  Every element shares one grid and is a
 * whole number of stations long, and (u, v) turns rigidly with the section: the alignment is one continuous image of
 * global station x sector.  Per frame on an alignment: gm_wall_alignment_locate_frame -> gm_wall_alignment_align_frame ->
 * gm_wall_alignment_check_frame -> gm_wall_alignment_add_frame_checked.  One operation per statement.
 *   global station  base_i = the sum of n_stations of the elements before i;  G = base_i + j for station j of element i;
 *                 total = the sum over all elements.
 *   per align     host, fp64.  The plan is gm_wall_alignment_add_plan's under the caller's pose, unchanged, with the same
 *                 reach: the sides, each side's own per-add frame, the joint planes; the refusals are the add's (more than
 *                 GM_WALL_JOINT_MAX_SIDES sides: GM_ERR_UNSUPPORTED, nothing is enqueued).  With e the sensor's side,
 *                 G_f = base_e + side_anchor[e];  per side  row0_s = base_s + side_anchor[s] - G_f + P  in 64-bit integers,
 *                 refused (GM_ERR_INVALID_ARG) unless it fits an int32.  The gate is the align's own, rounded to fp32 once.
 *                 P, A, B, C as gm_wall_map_align_*.
 *   per point     device, fp32.  The owner by the add's rule on the plan's planes.  The point runs its owner's chain alone
 *                 (straight, arc or clothoid, as gm_wall_map_align_* instantiates the add's chain on a straight map).
 *                 Classes in the chain's order: plane; beyond_gate; outside_patch; binned.  jl = floor(t / ds) relative to
 *                 the OWNER's anchor;  jr = row0_owner + jl in 64-bit integers (|jl| >= 4e18: outside_patch);  binned iff
 *                 0 <= jr < 2P.  Nothing is clamped to the owner's span: a point that its owner's chain places past the
 *                 owner's end is binned at the row the chain gives it, and a row outside [0, total) is still binned and
 *                 never overlaps, as on a map.  The patch cell jr * n_sectors + k, the sums of rint(e 2^20), the
 *                 min_frame_count rule and f are gm_wall_map_align_*'s.  The class counts are kept per side.
 *   map image     rows G = G_f - P - A .. G_f + P + A - 1.  Row G reads element i with base_i <= G < base_(i+1) at station
 *                 j = G - base_i, and is unusable outside [0, total).  m as on a map: min_count, integer division,
 *                 saturation.  The elements the rows meet are passed as pieces (element table, first global row,
 *                 n_stations), ascending; more than GM_WALL_ALIGN_MAX_PIECES: GM_ERR_UNSUPPORTED, nothing is enqueued.  The
 *                 pieces may be more than the sides: P + A stations can reach past the add's reach.
 *   score table, selection, status   gm_wall_map_align_*'s, unchanged, on (f, m).
 *   pose          host, fp64.  s = the plan's chainage of the sensor;  s' = s + shift_m.  F(x) = [a(x) u(x) v(x)] and P(x):
 *                 the design frame at alignment chainage x of the element the `point` rule picks for x (the first element
 *                 before the start, the last from the end on; gm_wall_arc_frame's, gm_wall_clothoid_frame's, or the
 *                 straight frame at x - offset).  Q = the rotation by `roll` about the first axis in section coordinates
 *                 ((1, 0, 0), (0, cos, -sin), (0, sin, cos) by rows).  M = F(s') Q F(s)^T;  Rm' = M Rm;
 *                 tr' = P(s') + M (tr - P(s)).  On a straight element this is gm_wall_map_align_*'s pose.  The pose passes
 *                 the library's own pose check.
 *   one straight side   n_sides == 1, the sensor's element is straight and every image row lies in that element or outside
 *                 [0, total): the align IS gm_wall_map_align_* of that element map -- the same launches, the table, the
 *                 shared info fields and the pose byte for byte.  Every other plan, of 1 .. GM_WALL_JOINT_MAX_SIDES sides,
 *                 runs the rule above.
 *   ordering      no map is changed.  The align sees every add enqueued before it on any slot to the map of any piece (not
 *                 only of the sides), through the alignment or through an element map, and none enqueued after: a later
 *                 add on any slot waits for it through the alignment's pending results, as for a locate and a check.
 * No floating-point atomics, no ticket, no host round trip inside the align.  Scratch per (alignment, slot) -- the patch,
 * the two int32 images, the table, a pinned copy of the result -- is allocated by the first align that is not an element
 * map's own, kept grow-only and freed with the alignment; an alignment that never aligns allocates nothing. */
#define GM_WALL_ALIGN_MAX_PIECES 8
typedef struct gm_wall_alignment_align_piece {   /* 16 bytes */
    uint32_t element;
    uint32_t n_stations;       /* the element's */
    int64_t  first_row;        /* base_element: the global station of its station 0 */
} gm_wall_alignment_align_piece;

typedef struct gm_wall_alignment_align_plan_info {   /* 336 bytes: what an align's kernels receive, host only */
    uint32_t struct_size;      /* = sizeof(gm_wall_alignment_align_plan_info), filled by the library */
    uint32_t n_pieces;         /* 1 .. GM_WALL_ALIGN_MAX_PIECES; 0: no image row lies in [0, total) */
    gm_wall_alignment_add_info add;   /* the plan of the add under the same pose */
    int64_t  anchor_global;    /* G_f */
    int64_t  total;            /* the alignment's stations */
    int32_t  row0[GM_WALL_JOINT_MAX_SIDES];   /* per side; 0 from n_sides on */
    uint32_t own;              /* 1: the "one straight side" rule holds: the align is the element map's own */
    uint32_t home;             /* the sensor's element's index among the sides */
    gm_wall_alignment_align_piece piece[GM_WALL_ALIGN_MAX_PIECES];   /* ascending; zero from n_pieces on */
} gm_wall_alignment_align_plan_info;

typedef struct gm_wall_alignment_align_info {   /* 472 bytes; the first 224 are gm_wall_align_info's */
    uint32_t struct_size;     /* = sizeof(gm_wall_alignment_align_info), filled by the library */
    uint32_t status;          /* GM_ALIGN_* */
    uint32_t n_points;
    uint32_t plane, beyond_gate, outside_patch, binned;   /* summed over the sides */
    uint32_t patch_cells_usable;
    int64_t  anchor_station;  /* j_f of the sensor's side */
    uint32_t half_patch_stations, max_station_shift, max_sector_shift;
    uint32_t overlap;
    int32_t  best_station, best_sector;
    double   frac_station, frac_sector;
    double   shift_m, roll, bias_m, rms_best, rms_runner, distinction;
    double   pose[12];        /* the aligned pose (the rule above) */
    uint32_t element;         /* the sensor's element */
    uint32_t n_sides;
    double   chainage;        /* s */
    int64_t  anchor_global;   /* G_f */
    uint32_t side_class[GM_WALL_JOINT_MAX_SIDES][4];   /* plane, beyond_gate, outside_patch, binned per side; 0 from n_sides on */
    gm_wall_alignment_add_info plan;
} gm_wall_alignment_align_info;

/* Host only, no context: the plan of an align under `pose` on a context whose boxFilterBound is `bound`: the add's plan,
 * G_f, row0 per side and the pieces exactly as the kernels receive them.  prm NULL: the defaults.  GM_ERR_INVALID_ARG: NULL,
 * the alignment's refusals, parameters gm_wall_align_check_params refuses on the alignment's n_sectors, a refused pose, a
 * row0 beyond int32; GM_ERR_UNSUPPORTED: too many sides, or more than GM_WALL_ALIGN_MAX_PIECES pieces. */
gm_status gm_wall_alignment_align_plan(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                          const double pose[12], double bound, const gm_wall_align_params *prm,
                                          gm_wall_alignment_align_plan_info *plan);
/* Host only, no context: the selection and the pose of the rule above from a score table of (2A + 1)(2B + 1) records, as
 * gm_wall_align_select on a map: everything of info but the device's counts (n_points, the classes, side_class,
 * patch_cells_usable stay 0).  Errors as gm_wall_alignment_align_plan; a wrong n_scores: GM_ERR_INVALID_ARG. */
gm_status gm_wall_alignment_align_select(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                         const double pose[12], double bound, const gm_wall_align_params *prm,
                                         const gm_wall_align_score *table, uint32_t n_scores, gm_wall_alignment_align_info *info);
/* gm_wall_map_align_frame on the alignment (prm NULL: the defaults).  plan may be NULL.  GM_ERR_INVALID_ARG: NULL, a foreign
 * context, a bad slot, bad parameters, a refused pose; GM_ERR_NOT_READY: the slot holds no frame; GM_ERR_UNSUPPORTED: too
 * many sides or pieces. */
gm_status gm_wall_alignment_align_frame(gm_wall_alignment *alignment, gm_ctx *ctx, uint32_t slot, const double pose[12],
                                        const gm_wall_align_params *prm, gm_wall_alignment_align_plan_info *plan);
/* The result of the last align enqueued on (alignment, slot), as gm_wall_map_get_align: waits for that align only; info,
 * n_out may be NULL; scores NULL with capacity 0 is a count query; GM_ERR_CAPACITY.  GM_ERR_NOT_READY: none was enqueued;
 * GM_ERR_INVALID_ARG: NULL, a bad slot.  gm_wall_alignment_align_points counts as an align on slot 0. */
gm_status gm_wall_alignment_get_align(gm_wall_alignment *alignment, uint32_t slot, gm_wall_alignment_align_info *info,
                                      gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out);
/* The same kernels as one blocking stage call on host buffers (slot 0).  The per-point outputs may each be NULL: residual
 * (e, NaN for plane points), cell (jr * n_sectors + k of a binned point, else -1), element (the owner's element index, set
 * for every point). */
gm_status gm_wall_alignment_align_points(gm_wall_alignment *alignment, const float *xyz, uint32_t n, const uint8_t *labels,
                                         const double pose[12], const gm_wall_align_params *prm,
                                         gm_wall_alignment_align_plan_info *plan, gm_wall_alignment_align_info *info,
                                         gm_wall_align_score *scores, uint32_t capacity, uint32_t *n_out, float *residual,
                                         int32_t *cell, int32_t *element);

/* ---- a check's changed points as objects on a wall alignment (gm_wall_alignment_check_objects) ----------------------------
 * gm_wall_map_check_objects on the alignment: the same parameters (gm_wall_object_params), the same 128-byte record
 * (gm_wall_object), on the alignment's GLOBAL station grid, so that an object that lies across a joint plane is ONE object
 * and keeps its label whatever sides the frame's plan happened to have.  Per frame on an alignment:
 * gm_wall_alignment_locate_frame -> gm_wall_alignment_align_frame -> gm_wall_alignment_check_frame ->
 * gm_wall_alignment_check_objects -> gm_wall_alignment_add_frame_checked.
 *   global station  base_i, G = base_i + j and total as in the align section above.
 *   size          GM_ERR_UNSUPPORTED unless total <= 2^32 - 1 and ceil(total / bs) NK <= 2^32 - 1: G and the label are then
 *                 32-bit and the kernels need no 64-bit division.
 *   per row       side = GM_WALL_ROW_SIDE(cell), c = GM_WALL_ROW_CELL(cell).  A row is REJECTED if side >= n_sides of the
 *                 check's plan, if c >= n_stations_e n_sectors of that side's element e = side_element[side], if dq == 0 or
 *                 if any of x, y, z, e is not finite.  Otherwise j = c / n_sectors, k = c % n_sectors, G = base_e + j.  The
 *                 side is checked before it picks anything: no load or store index depends on an unchecked side.
 *   blocks, window, planes, neighbours, component, classes, order, object_of_row
 *                 the map rule's (gm_wall_map_check_objects), word for word, on a virtual map of `total` stations with G in
 *                 place of j.  Blocks are anchored on global station 0: J = G / bs, so a block may hold stations of two
 *                 elements when base_i % bs != 0; label = J NK + K.  The anchor is G_f = base_e + side_anchor[e] of the
 *                 sensor's side, in int64; the window is [max(0, G_f - H), min(total, G_f + H)), widened to block rows;
 *                 above GM_WALL_OBJECT_MAX_BLOCKS blocks GM_ERR_INVALID_ARG.
 *   record        station_min / station_max are global stations; everything else as on a map.  The sector extents are
 *                 continuous across joints because (u, v) turns rigidly with the section.
 * So the result is what gm_wall_check_objects gives on ONE straight map of `total` stations fed the same rows with cell
 * rewritten to G n_sectors + k, around the anchor G_f -- byte for byte wherever such a map can exist
 * (total n_sectors <= 2^24); the decode lives in the kernel so that the call also works where none can.  A one-side check
 * on element 0 gives that element map's gm_wall_map_check_objects records byte for byte; on element i with base_i % bs == 0
 * the same records with label shifted by (base_i / bs) NK and the station extents by base_i.
 * On the device: gm_wall_map_check_objects' launches; the three kernels that read a row (bin, reduce, rows) are joint
 * instantiations of the map's code behind a decode that reads a by-value side table, the others are the map's own. */
typedef struct gm_wall_alignment_objects_info {   /* 136 bytes; the first 64 are gm_wall_objects_info's */
    uint32_t struct_size;           /* = sizeof(gm_wall_alignment_objects_info), filled by the library */
    uint32_t n_rows;                /* = the sum of the five classes below */
    uint32_t station0, n_stations;  /* the block-aligned window in GLOBAL stations, clipped to [0, total); 0, 0 when empty */
    uint32_t blocks_stations, blocks_sectors;
    uint32_t rejected, outside_window, sparse, small, in_object;
    uint32_t flagged_pos, flagged_neg;
    uint32_t components;
    uint32_t objects;
    uint32_t reserved;              /* 0 */
    uint32_t element;               /* the sensor's element */
    uint32_t n_sides;               /* of the check's plan */
    int64_t  anchor_global;         /* G_f */
    int64_t  total;                 /* the alignment's stations */
    uint32_t side_element[GM_WALL_JOINT_MAX_SIDES];   /* 0 from n_sides on */
    uint32_t side_first[GM_WALL_JOINT_MAX_SIDES];     /* base of each side's element */
    uint32_t side_rows[GM_WALL_JOINT_MAX_SIDES];      /* the rows of each side that were not rejected; 0 from n_sides on */
} gm_wall_alignment_objects_info;

/* (a struct tag only, no typedef: the function of the same name below fills it) */
struct gm_wall_alignment_object_metrics {   /* 112 bytes; the first 96 are gm_wall_object_metrics' */
    double centroid[3];
    double mean_m;
    double peak_m;
    double size[3];
    double chainage_from;           /* t_min + station_min * station_length, alignment chainage */
    double chainage_to;             /* t_min + (station_max + 1) * station_length */
    double angle_from_deg;
    double angle_to_deg;
    uint32_t element_from, element_to;   /* the elements of station_min and of station_max */
    uint32_t station_from, station_to;   /* those stations inside them: station_min - base_from, station_max - base_to */
};

/* The objects of the last check enqueued THROUGH THE ALIGNMENT on (alignment, slot), ascending by (label, sign).  It finds
 * the rows wherever they are staged (the alignment's buffer, or after a one-side check the element map's), by
 * gm_wall_alignment_add_frame_checked's rules, waits for that check's event only, runs over the staged rows where they lie
 * -- no row crosses PCIe -- and blocks.  It may be repeated with other parameters and changes neither the maps nor the
 * rows.  info is required; count queries, GM_ERR_CAPACITY and the NULL rules are gm_wall_map_check_objects'.  Zero rows or
 * an empty window launch nothing.  Scratch (gm_wall_map_check_objects' amounts) belongs to the alignment: allocated by
 * the first call, kept grow-only, freed with the alignment; an alignment that never asks allocates nothing.  The tile shape
 * (GM_WALL_OBJECT_TILE, read at gm_wall_alignment_create) changes nothing in the result.
 * GM_ERR_NOT_READY: no check was enqueued on (alignment, slot), or a check on the element map itself has since replaced a
 * one-side check's rows.  GM_ERR_UNSUPPORTED: the size rule.  GM_ERR_INVALID_ARG: as gm_wall_map_check_objects. */
gm_status gm_wall_alignment_check_objects(gm_wall_alignment *alignment, uint32_t slot, const gm_wall_object_params *prm,
                                          gm_wall_alignment_objects_info *info, gm_wall_object *objects, uint32_t capacity,
                                          uint32_t *n_out, int32_t *object_of_row, uint32_t row_capacity);
/* The same kernels as one blocking stage call on n_rows host rows in any order.  The sides and the anchor are taken from
 * plan: n_sides, side_element, side_anchor, element.  object_of_row (may be NULL) holds n_rows entries.  Fed the rows and
 * the plan of gm_wall_alignment_get_check it returns gm_wall_alignment_check_objects' bytes.  GM_ERR_INVALID_ARG as above,
 * and for rows NULL with n_rows > 0, a NULL plan, a plan whose struct_size is wrong, whose sides are not 1 ..
 * GM_WALL_JOINT_MAX_SIDES consecutive ascending elements of this alignment, or whose element is not among them. */
gm_status gm_wall_alignment_check_objects_rows(gm_wall_alignment *alignment, const gm_wall_check_point *rows, uint32_t n_rows,
                                               const gm_wall_alignment_add_info *plan, const gm_wall_object_params *prm,
                                               gm_wall_alignment_objects_info *info, gm_wall_object *objects, uint32_t capacity,
                                               uint32_t *n_out, int32_t *object_of_row);
/* Host only, no context: an info's window fields, element, n_sides, anchor_global, total, side_element and side_first
 * exactly as the device calls report them for this plan (the counts stay 0).  prm NULL: the defaults.  Refusals: the
 * alignment's, the plan's and the parameters' (GM_ERR_INVALID_ARG), the size rule (GM_ERR_UNSUPPORTED). */
gm_status gm_wall_alignment_object_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                          const gm_wall_alignment_add_info *plan, const gm_wall_object_params *prm,
                                          gm_wall_alignment_objects_info *info);
/* Host only: gm_wall_object_metrics' derivation for a record on the global grid, with the template's t_min and
 * station_length (every operation rounded once), and the elements and the stations inside them of the record's two station
 * extents.  op may be NULL.  GM_ERR_INVALID_ARG: NULL, the alignment's refusals, gm_wall_object_metrics' refusals, a
 * station extent outside [0, total). */
gm_status gm_wall_alignment_object_metrics(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n,
                                           const gm_wall_object_params *op, const gm_wall_object *o,
                                           struct gm_wall_alignment_object_metrics *out);

/* ---- connected deviation regions of a wall alignment (gm_wall_alignment_regions) ------------------------------------------
 * gm_wall_map_regions on the alignment: the same parameters (gm_wall_region_params), the same 64-byte record
 * (gm_wall_region), on a window of the alignment's GLOBAL station grid, so that a patch of overbreak or an intrusion that
 * lies across a joint plane is ONE region with one label, one min_cells test, its whole volume and its one peak.
 *   global station  base_i, G = base_i + j and total as in the align and the objects sections above.
 *   window        the global stations [station0, station0 + n), inside [0, total]; n = 0 gives no regions and launches
 *                 nothing.
 *   size          GM_ERR_UNSUPPORTED if total n_sectors > 2^31 - 1 (labels are global cell indices G n_sectors + k, and
 *                 cell_labels is int32 with -1 for none) or if the window holds more than
 *                 GM_WALL_ALIGNMENT_REGION_MAX_CELLS cells (1 GiB of scratch at 16 B per cell).
 *   rule          gm_wall_map_regions', word for word, on a virtual map of `total` stations: d, the classes, the sign, 4-
 *                 and 8-connectivity, the wrap around the ring, min_cells, the peak and its tie rule, the record and the
 *                 ascending label order.  Cell (G, k) of the virtual map is cell (G - base_e, k) of the map of the element
 *                 e that owns station G.
 *   record        label and peak_cell are global cell indices, station_min and station_max global stations.  The sector
 *                 extents are continuous across joints because (u, v) turns rigidly with the section.
 *   baseline      (may be NULL) another alignment of the same context whose template parameters (but for gate and the
 *                 unused n_stations) and whose element list (kind, n_stations, turn, curvature, rate) equal this
 *                 alignment's bit for bit; cell (G, k) of the baseline is read beside cell (G, k).
 * The rule has no floating point and never sees the axis, so the result is what gm_wall_map_regions gives on ONE straight
 * map of `total` stations fed the element maps' raw cells concatenated in element order -- byte for byte wherever such a map
 * can exist (total n_sectors <= 2^24); the pieces are read where they lie so that the call also works where none can.  A
 * window inside element 0 gives that element map's gm_wall_map_regions bytes; a window inside element i the same records
 * with label and peak_cell shifted by base_i n_sectors and the station extents by base_i.
 * On the device: gm_wall_map_regions' launches; the two kernels that read a cell (tiles, reduce) are joint instantiations
 * of the map's code behind a table of the window's pieces in device memory, the others are the map's own. */
#define GM_WALL_ALIGNMENT_REGION_MAX_CELLS (1u << 26)   /* the most cells of a window */

typedef struct gm_wall_alignment_regions_info {   /* 112 bytes; the first 80 are gm_wall_regions_info's */
    uint32_t struct_size;     /* = sizeof(gm_wall_alignment_regions_info), filled by the library */
    uint32_t station0, n_stations, n_sectors;   /* the window in GLOBAL stations and the template's sectors */
    int64_t  threshold_q;     /* T */
    uint64_t flagged_pos, flagged_neg, unusable, empty;
    uint64_t components;
    uint64_t regions;
    double   cell_area;       /* station_length * radius * 2 pi / n_sectors of the template, m^2 */
    int64_t  total;           /* the alignment's stations */
    uint32_t n_pieces;        /* the elements the window meets: element_from .. element_to, consecutive (0: n = 0) */
    uint32_t element_from, element_to;
    uint32_t station_from;    /* the window's first station inside element_from */
    uint32_t station_to;      /* the window's last station inside element_to, inclusive */
    uint32_t reserved;        /* 0 */
} gm_wall_alignment_regions_info;

/* (a struct tag only, no typedef: the function of the same name below fills it) */
struct gm_wall_alignment_region_metrics {   /* 120 bytes; the first 64 are gm_wall_region_metrics' */
    double area_m2;
    double volume_m3;
    double peak_m;
    double mean_m;
    double chainage_from;           /* t_min + station_min * station_length, alignment chainage */
    double chainage_to;             /* t_min + (station_max + 1) * station_length */
    double angle_from_deg;
    double angle_to_deg;
    uint32_t element_from, element_to;   /* the elements of station_min and of station_max */
    uint32_t station_from, station_to;   /* those stations inside them: station_min - base_from, station_max - base_to */
    uint32_t peak_element, peak_station, peak_sector;   /* of peak_cell: G_p = peak_cell / n_sectors = base + peak_station, k_p */
    uint32_t reserved;              /* 0 */
    double peak_point[3];           /* gm_wall_alignment_point at chainage t_min + (G_p + 0.5) station_length, angle
                                       (2 pi (k_p + 0.5)) / n_sectors and rho = radius + peak 2^-20 (every operation rounded
                                       once): where to send someone */
};

/* The regions of the window, ascending by label.  Synchronises every element map the window meets and the baseline's (as
 * gm_wall_map_sync: it sees every add enqueued before it, through the alignment or through an element map), runs on the
 * device and blocks.  prm NULL: the defaults.  info is required; count queries, GM_ERR_CAPACITY, *n_out, cell_labels
 * ([n][n_sectors]) and the NULL rules are gm_wall_map_regions'.  No map is changed.  Scratch (gm_wall_map_regions' amounts
 * and 96 B per piece) belongs to the alignment: allocated by the first call, kept grow-only, freed with the alignment; an
 * alignment that never asks allocates nothing.  The tile is element map 0's (GM_WALL_REGION_TILE, read at its create) and
 * changes nothing in the result.
 * GM_ERR_UNSUPPORTED: the size rule.  GM_ERR_INVALID_ARG: as gm_wall_map_regions, a window outside [0, total], a baseline
 * that is the alignment itself, of another context, on another template or with another element list. */
gm_status gm_wall_alignment_regions(gm_wall_alignment *alignment, gm_wall_alignment *baseline, uint32_t station0, uint32_t n,
                                    const gm_wall_region_params *prm, gm_wall_alignment_regions_info *info, gm_wall_region *regions,
                                    uint32_t capacity, uint32_t *n_out, int32_t *cell_labels);
/* Host only, no context: an info's window fields (station0, n_stations, n_sectors, cell_area, total, n_pieces and the four
 * element and station fields) exactly as the device call reports them (threshold_q and the counts stay 0).  Refusals: the
 * alignment's and the window's (GM_ERR_INVALID_ARG), the size rule (GM_ERR_UNSUPPORTED; its first arm is tested before the
 * window, its second behind it). */
gm_status gm_wall_alignment_region_window(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n_el,
                                          uint32_t station0, uint32_t n, gm_wall_alignment_regions_info *info);
/* Host only: gm_wall_region_metrics' derivation for a record on the global grid, with the template's t_min, station_length,
 * radius and n_sectors, the elements and the stations inside them of the record's two station extents and of its peak cell,
 * and the design position of the peak.  GM_ERR_INVALID_ARG: NULL, the alignment's refusals, gm_wall_region_metrics'
 * refusals, a station extent or a peak cell outside [0, total). */
gm_status gm_wall_alignment_region_metrics(const gm_wall_params *params, const gm_wall_element *elements, uint32_t n_el,
                                           const gm_wall_region *r, struct gm_wall_alignment_region_metrics *out);

/* "Compressed map" record of a completed slot.  The reference defines no such
 * output; this is a build-defined format: header, primitive records,
 * then n_voxels rows of x,y,z,count (float32).  Returns the bytes needed in
 * *n_bytes (also on GM_ERR_CAPACITY). */
typedef struct gm_map_header {
    char     magic[4];       /* "GMAP" */
    uint32_t version;        /* 1 */
    uint32_t n_primitives;
    uint32_t n_voxels;
    float    leaf, bound;
    uint32_t n_points;       /* valid points the map was built from */
    uint32_t reserved;
    float    eigenvalues[3];
    float    center_axis[3];
} gm_map_header;
typedef struct gm_map_primitive {
    uint32_t type;           /* 1 plane (a,b,c,d refit), 2 cylinder (point, axis, radius): the RANSAC hypothesis, or with
                                GM_CFG_CYLINDER_FIT and a successful fit gm_cylinder_fit.model / .inliers */
    uint32_t inliers;
    float    params[7];
    float    pad;
} gm_map_primitive;
gm_status gm_get_compressed_map(gm_ctx *ctx, uint32_t slot, void *buf, size_t capacity, size_t *n_bytes);

/* ---- multi-device group: one host thread, every local GPU ---------------------
 * The reference is one single-threaded process (ros::spin(), src/geometric_mapping.cpp:146,169: subscriber queue 1, one
 * frame at a time) on one CPU core; it has no counterpart for this section.  north_star: "Frames shard spatially across
 * the 8 GPUs of one node with an RCCL all-gather of fitted primitives over xGMI only when a scan exceeds single-GPU
 * capacity"; BASELINE configs[3] (one frame over 4 GPUs) and configs[4] (frames streamed over 8 GPUs).
 *
 * A group owns one gm_ctx per rank (one rank per device) and, across distinct devices, one RCCL communicator per rank
 * (ncclCommInitAll, single process; librccl is loaded at run time, the copy the process already has if it has one).
 *
 * SHARDED FRAME.  gm_group_process_frame cuts ONE frame into x-slabs balanced by the count of in-box points, adds a
 * 1.01 * neighborRadius halo (neighbours only, never outputs: gm_set_owned_range) ON THE HOST before H2D -- one parallel
 * pass for a histogram of x over the VoxelGrid lattice, edges on lattice planes (exactly, by the kernels' own float
 * expression) so that no voxel straddles two ranks, one parallel pass that scatters the rows into per-rank page-locked
 * buffers -- runs the unchanged single-GPU pipeline on every rank asynchronously, and exchanges the results with ONE
 * ncclAllGather of a 24-double record per rank (scatter partials, counts, the rank's fitted plane / cylinder).  The
 * merged frame: scatter = sum of the partials (rank order), 3x3 solve, counts summed, voxel centroids of the ranks in
 * ascending pcl key order (bit for bit the unsharded frame's; a lattice too coarse to cut along is merged through the
 * ranks' exact fixed-point voxel sums instead); fitted primitives by vote -- every rank's fit is a candidate, every rank
 * counts every candidate's inliers on its own resident owned points (gm_score_frame), the largest total wins.
 * The cylinder regression of a sharded frame is a stage call after it, gm_group_fit_cylinder: the ranks' sums of every
 * Gauss-Newton pass are merged into one regression on the device (one ncclAllGather of a 24-double row per pass).
 *
 * STREAMING.  Frames that fit one GPU are independent: gm_group_submit_frame hands a whole frame to the next device in
 * turn (its next free slot; gm_config.n_slots frames in flight per device), gm_group_wait_frame returns the frames in
 * submission order.  No collective.  Results are those of gm_process_frame on that device, bit for bit. */
typedef struct gm_group gm_group; /* opaque */
#define GM_GROUP_LOOPBACK (1u << 0) /* ranks may share a device (tests on a 1-GPU box): the records travel by device
                                       copies instead of RCCL; everything else is the same code */
gm_status gm_group_create(const gm_config *cfg, const int32_t *devices, uint32_t n_ranks, uint32_t flags, gm_group **out);
void gm_group_destroy(gm_group *grp);
uint32_t gm_group_size(const gm_group *grp);
/* the rank's own context, for the per-rank accessors (gm_get_normals, gm_get_voxel_centroids, ...) */
gm_ctx *gm_group_ctx(gm_group *grp, uint32_t rank);
const char *gm_group_last_error(const gm_group *grp); /* grp may be NULL for a failure inside gm_group_create */
/* One sharded frame, blocking.  cloud must be host rows.  res: the merged frame (n_cropped counts every in-box point
 * once; eigen results from the summed scatter; plane / cylinder = the vote's winners with their global inlier counts).
 * After a failure nothing of the frame is in flight and the accessors below report GM_ERR_NOT_READY; after a failed
 * collective (GM_ERR_COMM) the group refuses further work. */
gm_status gm_group_process_frame(gm_group *grp, const gm_cloud *cloud, gm_frame_result *res);
/* /choppedCloud of the last sharded frame in the single-GPU order (ascending input row); rows x,y,z,pad(= input row) */
gm_status gm_group_get_cropped_xyz(gm_group *grp, float *xyzw, uint32_t capacity, uint32_t *n_out);
/* pcl::VoxelGrid output of the last sharded frame, ascending key order: rows x,y,z,count (src/tunnel_processing.cpp:217-220) */
gm_status gm_group_get_voxel_centroids(gm_group *grp, float *xyzc, uint32_t capacity, uint32_t *n_out);
/* per centroid: nx,ny,nz,curvature of its nearest valid point / that point's index in gm_group_get_cropped_xyz's order
 * (kdtree->nearestKSearch + normals->at of the marker loop, src/tunnel_processing.cpp:237-249); the search runs on every
 * rank, the closest point of all wins.  Needs GM_CFG_NEAREST | GM_CFG_VOXEL_GRID. */
gm_status gm_group_get_voxel_normals(gm_group *grp, float *nxyzc, uint32_t capacity, uint32_t *n_out);
gm_status gm_group_get_voxel_nearest(gm_group *grp, int32_t *idx, uint32_t capacity, uint32_t *n_out);
/* Least-squares cylinder over the last sharded frame (gm_group_process_frame), every rank's resident valid cloud.
 * init7: starting row (point, direction, radius); NULL = the frame's published (voted) cylinder.  tau = the group's
 * ransac_threshold.  Afterwards every rank's labels are those of the published plane (1) and of the fit (2), 0 elsewhere.
 * Same algorithm, statuses and record as gm_fit_cylinder / GM_CFG_CYLINDER_FIT.  The ranks' sums of each pass are
 * all-gathered (4 rounds) and merged in rank order on every rank; a 1-rank group gives the single-device fit bit for bit.
 * No plane (flag off, no inliers or a NaN row): every label starts at 0.  GM_ERR_NOT_READY without a completed sharded
 * frame; GM_ERR_COMM after a failed collective (the group then refuses further work); GM_ERR_DEVICE if the ranks'
 * records differ.  The rank contexts need not have GM_CFG_CYLINDER_FIT. */
gm_status gm_group_fit_cylinder(gm_group *grp, const float init7[7], gm_cylinder_fit *out);
/* the last gm_group_fit_cylinder result of the current sharded frame (GM_ERR_NOT_READY otherwise) */
gm_status gm_group_get_cylinder_fit(const gm_group *grp, gm_cylinder_fit *out);
/* labels of the last sharded frame, one per row of gm_group_get_cropped_xyz and in its order (the ranks' RANSAC labels,
 * or those of gm_group_fit_cylinder once it ran; GM_ERR_NOT_READY without a GM_CFG_RANSAC_* flag before a fit) */
gm_status gm_group_get_labels(gm_group *grp, uint8_t *labels, uint32_t capacity, uint32_t *n_out);
/* wall-clock split of the last gm_group_process_frame call, milliseconds */
enum { GM_GROUP_T_CUT = 0,    /* host: histogram, edges, rows scattered into the per-rank page-locked buffers */
       GM_GROUP_T_SUBMIT = 1, /* host: the ranks' frames enqueued (H2D + launch chains) */
       GM_GROUP_T_DEVICE = 2, /* waiting for H2D, kernels and the all-gather of every rank */
       GM_GROUP_T_MERGE = 3,  /* records merged, voxel lists merged, primitive vote */
       GM_GROUP_T_TOTAL = 4,
       GM_GROUP_N_TIMINGS = 5 };
gm_status gm_group_get_timing(const gm_group *grp, double *ms, uint32_t capacity);
/* the n_ranks + 1 slab edges of the last sharded frame (first -inf, last +inf); *on_lattice = 1 when they lie on planes
 * of the VoxelGrid lattice */
gm_status gm_group_get_edges(const gm_group *grp, double *edges, uint32_t capacity, uint32_t *on_lattice);
/* streaming: a whole frame to the next device in turn, asynchronously (cloud as for gm_submit_frame: host rows are
 * released on return unless GM_CLOUD_PINNED); GM_ERR_NOT_READY when every slot of every device holds a frame */
gm_status gm_group_submit_frame(gm_group *grp, const gm_cloud *cloud);
/* the oldest frame in flight (submission order); *rank / *slot (may be NULL) name where its bulky outputs can be fetched
 * (gm_get_cropped_xyz(gm_group_ctx(grp, rank), slot, ...)) until that slot is submitted to again */
gm_status gm_group_wait_frame(gm_group *grp, gm_frame_result *res, uint32_t *rank, uint32_t *slot);
/* never blocks: GM_OK when the oldest frame in flight has finished (gm_group_wait_frame returns at once),
 * GM_ERR_NOT_READY while it is running or when no frame is in flight */
gm_status gm_group_poll_frame(gm_group *grp);
uint32_t gm_group_in_flight(const gm_group *grp);

#ifdef __cplusplus
}
#endif
#endif /* GM_HIP_H */
