// gm_tunnel_processing.cpp -- see gm_tunnel_processing.hpp.  Plain C++11; links libgm_hip.so.
#include "gm_tunnel_processing.hpp"

#include <cmath>
#include <cstring>

namespace gm_host {

void Processor::check(gm_status s, const char *what)
{
    if (s != GM_OK) throw Error(s, std::string(what) + ": " + gm_status_string(s) + ": " + gm_last_error(ctx_));
}

Processor::Processor(double b, double leaf, double r, double wf, int device, unsigned flags)
    : ctx_(0), grp_(0), cur_(0), cur_slot_(0), n_slots_(1), next_slot_(0), pending_(0), wall_(0), alignment_(0), newest_slot_(-1), check_slot_(-1), al_check_slot_(-1),
      submitted_(0), waited_(0)
{
    gm_config cfg;
    gm_default_config(&cfg);
    cfg.boxFilterBound = b; cfg.voxelGridLeafSize = leaf; cfg.neighborRadius = r; cfg.weightingFactor = wf;
    cfg.device = device; cfg.flags = flags;
    gm_status s = gm_create(&cfg, &ctx_);
    if (s != GM_OK) throw Error(s, std::string("gm_create: ") + gm_last_error(0));
    cur_ = ctx_;
    std::memset(&last_, 0, sizeof(last_));
}

Processor::Processor(double b, double leaf, double r, double wf, const std::vector<int> &devices, unsigned flags,
                     unsigned slots_per_device)
    : ctx_(0), grp_(0), cur_(0), cur_slot_(0), n_slots_(slots_per_device ? slots_per_device : 1), next_slot_(0), pending_(0), wall_(0), alignment_(0),
      newest_slot_(-1), check_slot_(-1), al_check_slot_(-1), submitted_(0), waited_(0)
{
    if (devices.empty()) throw Error(GM_ERR_INVALID_ARG, "Processor: empty device list");
    gm_config cfg;
    gm_default_config(&cfg);
    cfg.boxFilterBound = b; cfg.voxelGridLeafSize = leaf; cfg.neighborRadius = r; cfg.weightingFactor = wf;
    cfg.flags = flags; cfg.n_slots = n_slots_;
    std::vector<int32_t> dev(devices.begin(), devices.end());
    // a device listed twice ("0,0": two ranks that stream on one GPU) needs the group's loopback flag; streaming has no
    // collective, so nothing else changes
    bool repeats = false;
    for (size_t a = 0; a < dev.size(); ++a)
        for (size_t c = a + 1; c < dev.size(); ++c) repeats = repeats || dev[a] == dev[c];
    gm_status s = gm_group_create(&cfg, &dev[0], (uint32_t)dev.size(), repeats ? GM_GROUP_LOOPBACK : 0u, &grp_);
    if (s != GM_OK) throw Error(s, std::string("gm_group_create: ") + gm_group_last_error(0));
    ctx_ = gm_group_ctx(grp_, 0);
    cur_ = ctx_;
    std::memset(&last_, 0, sizeof(last_));
}

Processor::~Processor()
{
    for (size_t i = 0; i < cloud_bufs_.size(); ++i) {   // (gm_set_cloud_output waits for a frame that still writes the rows)
        CloudBuf &b = cloud_bufs_[i];
        gm_set_cloud_output(b.ctx, b.slot, 0, 0);
        if (b.rows) gm_host_free(b.ctx, b.rows);
        for (size_t k = 0; k < b.retired.size(); ++k) gm_host_free(b.ctx, b.retired[k].rows);
    }
    if (grp_) gm_group_destroy(grp_);   // (owns the contexts)
    else gm_destroy(ctx_);
}

void Processor::enableCloudOutput(unsigned max_points)
{
    if (cloud_bufs_.empty()) {
        const unsigned ranks = grp_ ? gm_group_size(grp_) : 1u;
        for (unsigned r = 0; r < ranks; ++r)
            for (unsigned s = 0; s < n_slots_; ++s) {
                CloudBuf b;
                b.ctx = grp_ ? gm_group_ctx(grp_, r) : ctx_; b.slot = s; b.rows = 0; b.cap = 0u; b.since = 0;
                cloud_bufs_.push_back(b);
            }
    }
    growCloudOutput(max_points ? max_points : 1u);
}

// Retired rows received the slot's frames below the `since` of the rows that replaced them.  Frames leave in submission
// order and the accessors read frame waited_ - 1, so once that frame is one of the replacement's, none of the retired
// rows' frames is in flight or can still be read.
void Processor::freeRetiredCloudRows()
{
    for (size_t i = 0; i < cloud_bufs_.size(); ++i) {
        CloudBuf &b = cloud_bufs_[i];
        while (!b.retired.empty()) {
            const unsigned long long replaced_at = b.retired.size() > 1 ? b.retired[1].since : b.since;
            if (waited_ <= replaced_at) break;
            gm_host_free(b.ctx, b.retired[0].rows);
            b.retired.erase(b.retired.begin());
        }
    }
}

void Processor::growCloudOutput(unsigned n_points)
{
    freeRetiredCloudRows();
    for (size_t i = 0; i < cloud_bufs_.size(); ++i) {
        CloudBuf &b = cloud_bufs_[i];
        if (b.cap >= n_points) continue;
        const unsigned cap = n_points + n_points / 4u;
        void *rows = 0;
        gm_status s = gm_host_alloc(b.ctx, (size_t)cap * 16u, &rows);
        if (s != GM_OK) throw Error(s, std::string("enableCloudOutput: ") + gm_last_error(b.ctx));
        s = gm_set_cloud_output(b.ctx, b.slot, (float *)rows, cap);   // (waits for the slot's frame in flight, if any)
        if (s != GM_OK) { gm_host_free(b.ctx, rows); throw Error(s, std::string("enableCloudOutput: ") + gm_last_error(b.ctx)); }
        // A frame in flight, or the finished frame the accessors refer to, may have written its cloud into the old rows:
        // they are retired, not freed, unless no frame was submitted since they were set.
        if (b.rows) {
            if (b.since == submitted_) gm_host_free(b.ctx, b.rows);
            else { const CloudRows old = {b.rows, b.since}; b.retired.push_back(old); }
        }
        b.rows = (float *)rows; b.cap = cap; b.since = submitted_;
    }
}

unsigned Processor::capacity() const { return grp_ ? gm_group_size(grp_) * n_slots_ : n_slots_; }
unsigned Processor::inFlight() const { return grp_ ? gm_group_in_flight(grp_) : pending_; }

void Processor::submitFrame(const void *rows, unsigned n, unsigned step, unsigned ox, unsigned oy, unsigned oz, bool bigendian)
{
    gm_cloud c = {rows, n, step, ox, oy, oz, bigendian ? GM_CLOUD_BIGENDIAN : 0u};
    if (!cloud_bufs_.empty()) growCloudOutput(n);
    if (grp_) {
        gm_status s = gm_group_submit_frame(grp_, &c);
        if (s != GM_OK) throw Error(s, std::string("submitFrame: ") + gm_group_last_error(grp_));
        ++submitted_;
        return;
    }
    if (pending_ >= n_slots_) throw Error(GM_ERR_NOT_READY, "submitFrame: every slot holds a frame (waitFrame first)");
    check(gm_submit_frame(ctx_, next_slot_, &c), "submitFrame");
    newest_slot_ = (int)next_slot_;
    next_slot_ = (next_slot_ + 1) % n_slots_;
    ++pending_;
    ++submitted_;
}

gm_frame_result Processor::waitFrame()
{
    gm_frame_result r;
    if (grp_) {
        uint32_t rank = 0, slot = 0;
        if (!gm_group_in_flight(grp_)) throw Error(GM_ERR_NOT_READY, "waitFrame: no frame in flight");
        ++waited_;   // (the frame leaves the queue whatever the wait returns)
        gm_status s = gm_group_wait_frame(grp_, &r, &rank, &slot);
        if (s != GM_OK) throw Error(s, std::string("waitFrame: ") + gm_group_last_error(grp_));
        cur_ = gm_group_ctx(grp_, rank);
        cur_slot_ = slot;
        last_ = r;
        return r;
    }
    if (!pending_) throw Error(GM_ERR_NOT_READY, "waitFrame: no frame in flight");
    const unsigned slot = (next_slot_ + n_slots_ - pending_) % n_slots_;   // the oldest
    --pending_;   // (the frame leaves the queue whatever the wait returns: a failed frame must not be waited for again)
    ++waited_;
    check(gm_wait_frame(ctx_, slot, &r), "waitFrame");
    cur_ = ctx_; cur_slot_ = slot;
    last_ = r;
    return r;
}

bool Processor::tryWaitFrame(gm_frame_result &result)
{
    gm_status s;
    if (grp_) {
        if (!gm_group_in_flight(grp_)) return false;
        s = gm_group_poll_frame(grp_);
        if (s != GM_OK && s != GM_ERR_NOT_READY) throw Error(s, std::string("tryWaitFrame: ") + gm_group_last_error(grp_));
    } else {
        if (!pending_) return false;
        s = gm_poll_frame(ctx_, (next_slot_ + n_slots_ - pending_) % n_slots_);
        if (s != GM_OK && s != GM_ERR_NOT_READY) check(s, "tryWaitFrame");
    }
    if (s != GM_OK) return false;
    result = waitFrame();
    return true;
}

PointCloud Processor::chopCloud(const double &bound, const PointCloud &cloud)
{
    gm_cloud c = {cloud.empty() ? 0 : &cloud[0], (uint32_t)cloud.size(), 16, 0, 4, 8, 0};
    PointCloud out(cloud.size() ? cloud.size() : 1);
    uint32_t n = 0;
    check(gm_chop_cloud(ctx_, &c, bound, &out[0].x, (uint32_t)out.size(), &n), "chopCloud");
    out.resize(n);
    return out;
}

NormalCloud Processor::getNormals(const double &radius, PointCloud &cloud)
{
    const size_t n0 = cloud.size();
    std::vector<float> xyz(3 * (n0 ? n0 : 1));
    for (size_t i = 0; i < n0; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
    PointCloud oc(n0 ? n0 : 1);
    NormalCloud on(n0 ? n0 : 1);
    uint32_t n = 0;
    check(gm_get_normals_stage(ctx_, &xyz[0], (uint32_t)n0, radius, &oc[0].x, &on[0].normal[0], (uint32_t)oc.size(), &n),
          "getNormals");
    oc.resize(n); on.resize(n);
    cloud.swap(oc);  // ExtractIndices::filter(*cloud): the caller's cloud is compacted in place
    return on;
}

void Processor::getLocalFrame(const int &cloudSize, const double &wf, const NormalCloud &nrm, Vector3f &vals, Matrix3f &vecs)
{
    if (cloudSize < 0 || (size_t)cloudSize > nrm.size())
        throw std::out_of_range("getLocalFrame: cloudSize exceeds the normals cloud");  // the reference's .at() (:106)
    check(gm_get_local_frame(ctx_, nrm.empty() ? 0 : &nrm[0].normal[0], (uint32_t)cloudSize, wf, vals.v, vecs.m, 0),
          "getLocalFrame");
}

PointCloud Processor::voxelGrid(const double &leaf, const PointCloud &cloud)
{
    const size_t n0 = cloud.size();
    std::vector<float> xyz(3 * (n0 ? n0 : 1));
    for (size_t i = 0; i < n0; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
    PointCloud out(n0 ? n0 : 1);
    uint32_t n = 0, fl = 0;
    check(gm_voxel_grid(ctx_, &xyz[0], (uint32_t)n0, leaf, &out[0].x, (uint32_t)out.size(), &n, &fl), "voxelGrid");
    out.resize(n);
    return out;
}

std::vector<int> Processor::nearest(const PointCloud &cloud, const PointCloud &queries)
{
    std::vector<float> a(3 * (cloud.size() ? cloud.size() : 1)), q(3 * (queries.size() ? queries.size() : 1));
    for (size_t i = 0; i < cloud.size(); ++i) { a[3 * i] = cloud[i].x; a[3 * i + 1] = cloud[i].y; a[3 * i + 2] = cloud[i].z; }
    for (size_t i = 0; i < queries.size(); ++i) { q[3 * i] = queries[i].x; q[3 * i + 1] = queries[i].y; q[3 * i + 2] = queries[i].z; }
    std::vector<int> idx(queries.size() ? queries.size() : 1);
    check(gm_nearest(ctx_, &a[0], (uint32_t)cloud.size(), &q[0], (uint32_t)queries.size(), &idx[0]), "nearest");
    idx.resize(queries.size());
    return idx;
}

gm_frame_result Processor::processFrame(const void *rows, unsigned n, unsigned step, unsigned ox, unsigned oy, unsigned oz,
                                        bool bigendian)
{
    if (grp_ || pending_) {   // (frames already in flight finish first: results come back in submission order)
        while (inFlight()) waitFrame();
        submitFrame(rows, n, step, ox, oy, oz, bigendian);
        return waitFrame();
    }
    gm_cloud c = {rows, n, step, ox, oy, oz, bigendian ? GM_CLOUD_BIGENDIAN : 0u};
    if (!cloud_bufs_.empty()) growCloudOutput(n);
    gm_frame_result r;
    ++submitted_; ++waited_;   // (submitted and waited for in one call)
    check(gm_process_frame(ctx_, &c, &r), "processFrame");
    cur_ = ctx_; cur_slot_ = 0;
    newest_slot_ = 0;
    last_ = r;
    return r;
}

PointCloud Processor::choppedCloud()
{
    for (size_t i = 0; i < cloud_bufs_.size(); ++i) {   // the rows are already on the host (enableCloudOutput)
        const CloudBuf &b = cloud_bufs_[i];
        if (b.ctx != cur_ || b.slot != cur_slot_ || !b.rows || !waited_) continue;
        // the rows the frame wrote into: those set last before it was submitted (replaced since, if a larger frame came)
        const unsigned long long frame = waited_ - 1;
        const float *rows = b.rows;
        if (frame < b.since)
            for (size_t k = b.retired.size(); k-- > 0;) { rows = b.retired[k].rows; if (b.retired[k].since <= frame) break; }
        PointCloud out(last_.n_valid);
        if (last_.n_valid) std::memcpy(&out[0].x, rows, (size_t)last_.n_valid * sizeof(PointXYZ));
        return out;
    }
    uint32_t n = 0;
    gm_status s = gm_get_cropped_xyz(cur_, cur_slot_, 0, 0, &n);
    if (s != GM_OK && s != GM_ERR_CAPACITY) check(s, "choppedCloud");
    PointCloud out(n ? n : 1);
    check(gm_get_cropped_xyz(cur_, cur_slot_, &out[0].x, (uint32_t)out.size(), &n), "choppedCloud");
    out.resize(n);
    return out;
}

NormalCloud Processor::normals()
{
    uint32_t n = 0;
    gm_status s = gm_get_normals(cur_, cur_slot_, 0, 0, &n);
    if (s != GM_OK && s != GM_ERR_CAPACITY) check(s, "normals");
    NormalCloud out(n ? n : 1);
    check(gm_get_normals(cur_, cur_slot_, &out[0].normal[0], (uint32_t)out.size(), &n), "normals");
    out.resize(n);
    return out;
}

PointCloud Processor::voxelCentroids()
{
    uint32_t n = 0;
    gm_status s = gm_get_voxel_centroids(cur_, cur_slot_, 0, 0, &n);
    if (s != GM_OK && s != GM_ERR_CAPACITY) check(s, "voxelCentroids");
    PointCloud out(n ? n : 1);
    check(gm_get_voxel_centroids(cur_, cur_slot_, &out[0].x, (uint32_t)out.size(), &n), "voxelCentroids");
    out.resize(n);
    return out;
}

NormalCloud Processor::voxelNormals()
{
    uint32_t n = 0;
    gm_status s = gm_get_voxel_normals(cur_, cur_slot_, 0, 0, &n);
    if (s != GM_OK && s != GM_ERR_CAPACITY) check(s, "voxelNormals");
    NormalCloud out(n ? n : 1);
    check(gm_get_voxel_normals(cur_, cur_slot_, &out[0].normal[0], (uint32_t)out.size(), &n), "voxelNormals");
    out.resize(n);
    return out;
}

// ---- marker formatting: src/tunnel_processing.cpp:161-205, 225-256, 260-300 ----

Marker Processor::rvizArrow(const Vector3f &start, const Vector3f &end, const Vector3f &scale, const Vector4f &color,
                            const std::string &ns, const int &id, const std::string &frame)
{
    Marker m;
    m.frame_id = frame;      // :174 (stamp = ros::Time::now() and seq = 0 are set by the ROS shim)
    m.ns = ns; m.id = id;    // :177-178
    m.type = MARKER_ARROW; m.action = MARKER_ADD;  // :179-180
    for (int k = 0; k < 3; ++k) { m.points[0][k] = start(k); m.points[1][k] = end(k); m.scale[k] = scale(k); }
    m.color_a = color(0); m.color_r = color(1); m.color_g = color(2); m.color_b = color(3);  // :199-202: A,R,G,B
    m.position[0] = m.position[1] = m.position[2] = 0.0;   // the reference leaves the pose default-constructed
    m.orientation[0] = m.orientation[1] = m.orientation[2] = 0.0; m.orientation[3] = 1.0;
    return m;
}

// one CYLINDER marker centred on `pos`, its z axis along the unit `d`, diameter 2 rad, `length` long
static void cylinder_marker(const double pos[3], const double d[3], double rad, double length, Marker &m,
                            const std::string &frame)
{
    m.frame_id = frame; m.ns = "cylinder"; m.id = 0;
    m.type = MARKER_CYLINDER; m.action = MARKER_ADD;
    for (int k = 0; k < 3; ++k) { m.position[k] = pos[k]; m.points[0][k] = m.points[1][k] = 0.0; }
    // shortest-arc rotation taking the marker's z axis onto d: q = (z x d, 1 + z.d), normalised
    double q[4] = {-d[1], d[0], 0.0, 1.0 + d[2]};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (qn < 1e-12) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }   // d = -z: half turn about x
    else for (int k = 0; k < 4; ++k) q[k] /= qn;
    for (int k = 0; k < 4; ++k) m.orientation[k] = q[k];
    m.scale[0] = m.scale[1] = 2.0 * rad; m.scale[2] = length;
    m.color_a = 0.3f; m.color_r = 0.0f; m.color_g = 1.0f; m.color_b = 1.0f;
}

bool Processor::rvizCylinder(const gm_frame_result &r, const double &length, Marker &m, const std::string &frame)
{
    const double p[3] = {r.cylinder[0], r.cylinder[1], r.cylinder[2]};
    double d[3] = {r.cylinder[3], r.cylinder[4], r.cylinder[5]};
    const double rad = r.cylinder[6];
    const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(r.cylinder_inliers > 0) || !(dn > 0.0) || !(rad == rad)) return false;   // no cylinder this frame
    for (int k = 0; k < 3; ++k) d[k] /= dn;
    const double t = p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
    const double pos[3] = {p[0] - t * d[0], p[1] - t * d[1], p[2] - t * d[2]};
    cylinder_marker(pos, d, rad, length, m, frame);
    return true;
}

bool Processor::rvizCylinder(const gm_cylinder_fit &f, const double &length, Marker &m, const std::string &frame)
{
    if ((f.status & GM_FIT_FAILED_MASK) != 0) return false;   // no fitted cylinder
    const double dn = std::sqrt(f.axis[0] * f.axis[0] + f.axis[1] * f.axis[1] + f.axis[2] * f.axis[2]);
    if (!(dn > 0.0) || !(f.radius == f.radius)) return false;
    const double d[3] = {f.axis[0] / dn, f.axis[1] / dn, f.axis[2] / dn};
    cylinder_marker(f.point, d, f.radius, length, m, frame);
    return true;
}

gm_cylinder_fit Processor::getCylinder(const PointCloud &cloud, const float init[7], const double &tau,
                                       const std::vector<uint8_t> &labels, unsigned want, std::vector<uint8_t> *inliers)
{
    const size_t n = cloud.size();
    if (!labels.empty() && labels.size() != n) throw Error(GM_ERR_INVALID_ARG, "getCylinder: labels must have one entry per point");
    std::vector<float> xyz(3 * (n ? n : 1));
    for (size_t i = 0; i < n; ++i) { xyz[3 * i] = cloud[i].x; xyz[3 * i + 1] = cloud[i].y; xyz[3 * i + 2] = cloud[i].z; }
    if (inliers) inliers->assign(n ? n : 1, 0);
    gm_cylinder_fit f;
    std::memset(&f, 0, sizeof(f));
    check(gm_fit_cylinder(ctx_, &xyz[0], (uint32_t)n, labels.empty() ? 0 : &labels[0], want, init, tau, &f,
                          inliers ? &(*inliers)[0] : 0), "getCylinder");
    if (inliers) inliers->resize(n);
    return f;
}

gm_cylinder_fit Processor::cylinderFit()
{
    gm_cylinder_fit f;
    std::memset(&f, 0, sizeof(f));
    check(gm_get_cylinder_fit(cur_, cur_slot_, &f), "cylinderFit");
    return f;
}

void Processor::setSurfaceParams(const gm_surface_params &params)
{
    if (grp_) {
        for (unsigned r = 0; r < gm_group_size(grp_); ++r) {
            gm_ctx *c = gm_group_ctx(grp_, r);
            const gm_status s = gm_set_surface_params(c, &params);
            if (s != GM_OK) throw Error(s, std::string("setSurfaceParams: ") + gm_status_string(s) + ": " + gm_last_error(c));
        }
        return;
    }
    check(gm_set_surface_params(ctx_, &params), "setSurfaceParams");
}

void Processor::getSurfaceMap(gm_surface_info &info, std::vector<gm_surface_cell> &cells)
{
    uint32_t n = 0;
    gm_status s = gm_get_surface_map(cur_, cur_slot_, &info, 0, 0, &n);
    if (s != GM_OK && s != GM_ERR_CAPACITY) throw Error(s, std::string("getSurfaceMap: ") + gm_status_string(s) + ": " + gm_last_error(cur_));
    cells.resize(n);
    s = gm_get_surface_map(cur_, cur_slot_, &info, n ? &cells[0] : 0, n, &n);
    if (s != GM_OK) throw Error(s, std::string("getSurfaceMap: ") + gm_status_string(s) + ": " + gm_last_error(cur_));
}

void Processor::createWallMap(const gm_wall_params &params) { createWallMap(params, 0); }

void Processor::createWallMap(const gm_wall_params &params, const gm_wall_arc *arc) { createWallMap(params, arc, 0); }

void Processor::createWallMap(const gm_wall_params &params, const gm_wall_arc *arc, const gm_wall_clothoid *clothoid)
{
    if (grp_) throw Error(GM_ERR_UNSUPPORTED, "createWallMap: a wall map belongs to one context (single-device Processor)");
    if (arc && clothoid) throw Error(GM_ERR_INVALID_ARG, "createWallMap: an arc and a clothoid exclude each other");
    gm_wall_map *m = 0;
    if (clothoid) check(gm_wall_map_create_clothoid(ctx_, &params, clothoid, &m), "createWallMap");
    else check(arc ? gm_wall_map_create_arc(ctx_, &params, arc, &m) : gm_wall_map_create(ctx_, &params, &m), "createWallMap");
    if (wall_) gm_wall_map_destroy(wall_);
    wall_ = m;
    check_slot_ = -1;
}

void Processor::createWallAlignment(const gm_wall_params &params, const std::vector<gm_wall_element> &elements)
{
    if (grp_) throw Error(GM_ERR_UNSUPPORTED, "createWallAlignment: a wall alignment belongs to one context (single-device Processor)");
    gm_wall_alignment *al = 0;
    check(gm_wall_alignment_create(ctx_, &params, elements.empty() ? 0 : &elements[0], (uint32_t)elements.size(), &al),
          "createWallAlignment");
    if (alignment_) gm_wall_alignment_destroy(alignment_);
    alignment_ = al;
    al_check_slot_ = -1;
}

gm_wall_alignment_add_info Processor::addToWallAlignment(const double pose[12])
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "addToWallAlignment: createWallAlignment first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "addToWallAlignment: no frame yet");
    gm_wall_alignment_add_info info;
    check(gm_wall_alignment_add_frame(alignment_, ctx_, (unsigned)newest_slot_, pose, &info), "addToWallAlignment");
    return info;
}

gm_wall_alignment_locate_info Processor::locateWallAlignment(const double pose[12], const gm_wall_locate_params &prm)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "locateWallAlignment: createWallAlignment first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "locateWallAlignment: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_alignment_locate_frame(alignment_, ctx_, slot, pose, &prm), "locateWallAlignment");
    gm_wall_alignment_locate_info info;
    check(gm_wall_alignment_get_locate(alignment_, slot, &info), "locateWallAlignment");
    return info;
}

gm_wall_alignment_align_info Processor::alignWallAlignment(const double pose[12], const gm_wall_align_params &prm,
                                                           std::vector<gm_wall_align_score> *scores, gm_wall_alignment_align_plan_info *plan)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "alignWallAlignment: createWallAlignment first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "alignWallAlignment: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_alignment_align_frame(alignment_, ctx_, slot, pose, &prm, plan), "alignWallAlignment");
    gm_wall_alignment_align_info info;
    uint32_t count = 0;
    check(gm_wall_alignment_get_align(alignment_, slot, &info, 0, 0, &count), "alignWallAlignment");
    if (scores) {
        scores->resize(count);
        if (count) check(gm_wall_alignment_get_align(alignment_, slot, &info, &(*scores)[0], count, &count), "alignWallAlignment");
    }
    return info;
}

std::vector<gm_wall_check_point> Processor::checkWallAlignment(const double pose[12], const gm_wall_check_params &prm,
                                                               gm_wall_alignment_check_info *info, gm_wall_alignment_add_info *plan)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "checkWallAlignment: createWallAlignment first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "checkWallAlignment: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_alignment_check_frame(alignment_, ctx_, slot, pose, &prm, plan), "checkWallAlignment");
    al_check_slot_ = (int)slot;
    gm_wall_alignment_check_info local;
    gm_wall_alignment_check_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_alignment_get_check(alignment_, slot, ip, 0, 0, &count), "checkWallAlignment");
    std::vector<gm_wall_check_point> points(count);
    if (count) check(gm_wall_alignment_get_check(alignment_, slot, ip, &points[0], count, &count), "checkWallAlignment");
    points.resize(count);
    return points;
}

std::vector<gm_wall_object> Processor::wallAlignmentCheckObjects(const gm_wall_object_params &prm, gm_wall_alignment_objects_info *info)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "wallAlignmentCheckObjects: createWallAlignment first");
    if (al_check_slot_ < 0) throw Error(GM_ERR_NOT_READY, "wallAlignmentCheckObjects: checkWallAlignment first");
    gm_wall_alignment_objects_info local;
    gm_wall_alignment_objects_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_alignment_check_objects(alignment_, (unsigned)al_check_slot_, &prm, ip, 0, 0, &count, 0, 0), "wallAlignmentCheckObjects");
    std::vector<gm_wall_object> objects(count);
    if (count)
        check(gm_wall_alignment_check_objects(alignment_, (unsigned)al_check_slot_, &prm, ip, &objects[0], count, &count, 0, 0),
              "wallAlignmentCheckObjects");
    objects.resize(count);
    return objects;
}

std::vector<gm_wall_region> Processor::wallAlignmentRegions(const gm_wall_region_params &prm, uint32_t station0, uint32_t n,
                                                            gm_wall_alignment_regions_info *info)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "wallAlignmentRegions: createWallAlignment first");
    gm_wall_alignment_regions_info local;
    gm_wall_alignment_regions_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_alignment_regions(alignment_, 0, station0, n, &prm, ip, 0, 0, &count, 0), "wallAlignmentRegions");
    std::vector<gm_wall_region> regions(count);
    if (count)
        check(gm_wall_alignment_regions(alignment_, 0, station0, n, &prm, ip, &regions[0], count, &count, 0), "wallAlignmentRegions");
    regions.resize(count);
    return regions;
}

gm_wall_alignment_add_info Processor::addToWallAlignmentChecked(const double pose[12], const gm_wall_add_checked_params &prm,
                                                                gm_wall_add_checked_info *info)
{
    if (!alignment_) throw Error(GM_ERR_NOT_READY, "addToWallAlignmentChecked: createWallAlignment first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "addToWallAlignmentChecked: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    gm_wall_alignment_add_info plan;
    check(gm_wall_alignment_add_frame_checked(alignment_, ctx_, slot, pose, &prm, &plan), "addToWallAlignmentChecked");
    if (info) check(gm_wall_alignment_get_add_checked(alignment_, slot, info), "addToWallAlignmentChecked");
    return plan;
}

gm_wall_add_info Processor::addToWallMap(const double pose[12])
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "addToWallMap: createWallMap first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "addToWallMap: no frame yet");
    gm_wall_add_info info;
    check(gm_wall_map_add_frame(wall_, ctx_, (unsigned)newest_slot_, pose, &info), "addToWallMap");
    return info;
}

void Processor::readWallMap(unsigned station0, unsigned n, std::vector<gm_surface_cell> &cells)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "readWallMap: createWallMap first");
    uint64_t nc = 0;
    gm_status s = gm_wall_map_read(wall_, station0, n, 0, 0, &nc);
    if (s != GM_OK && s != GM_ERR_CAPACITY) check(s, "readWallMap");
    cells.resize((size_t)nc);
    if (nc) check(gm_wall_map_read(wall_, station0, n, &cells[0], nc, &nc), "readWallMap");
}

std::vector<gm_wall_region> Processor::wallMapRegions(unsigned station0, unsigned n, const gm_wall_region_params &prm, gm_wall_regions_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapRegions: createWallMap first");
    gm_wall_regions_info local;
    gm_wall_regions_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_map_regions(wall_, 0, station0, n, &prm, ip, 0, 0, &count, 0), "wallMapRegions");
    std::vector<gm_wall_region> regions(count);
    if (count) check(gm_wall_map_regions(wall_, 0, station0, n, &prm, ip, &regions[0], count, &count, 0), "wallMapRegions");
    regions.resize(count);
    return regions;
}

std::vector<gm_wall_cloud_point> Processor::wallMapCloud(unsigned station0, unsigned n, const gm_wall_cloud_params &prm, gm_wall_cloud_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapCloud: createWallMap first");
    gm_wall_cloud_info local;
    gm_wall_cloud_info *ip = info ? info : &local;
    uint64_t count = 0;
    check(gm_wall_map_cloud(wall_, station0, n, &prm, ip, 0, 0, &count), "wallMapCloud");
    std::vector<gm_wall_cloud_point> points((size_t)count);
    if (count) check(gm_wall_map_cloud(wall_, station0, n, &prm, ip, &points[0], count, &count), "wallMapCloud");
    points.resize((size_t)count);
    return points;
}

void Processor::wallMapMesh(unsigned station0, unsigned n, const gm_wall_mesh_params &prm, std::vector<gm_wall_cloud_point> *vertices,
                            std::vector<gm_wall_mesh_triangle> *triangles, gm_wall_mesh_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapMesh: createWallMap first");
    gm_wall_mesh_info local;
    gm_wall_mesh_info *ip = info ? info : &local;
    uint64_t nv = 0, nt = 0;
    check(gm_wall_map_mesh(wall_, station0, n, &prm, ip, 0, 0, 0, 0, &nv, &nt), "wallMapMesh");
    if (vertices) vertices->resize((size_t)nv);
    if (triangles) triangles->resize((size_t)nt);
    const bool wv = vertices && nv, wt = triangles && nt;
    if (wv || wt)
        check(gm_wall_map_mesh(wall_, station0, n, &prm, ip, wv ? &(*vertices)[0] : 0, wv ? nv : 0, wt ? &(*triangles)[0] : 0,
                               wt ? nt : 0, &nv, &nt),
              "wallMapMesh");
}

gm_wall_clearance_info Processor::wallMapClearance(unsigned station0, unsigned n, const std::vector<int32_t> &gauge_q,
                                                   const std::vector<uint8_t> &station_gauge, const gm_wall_clearance_params &prm,
                                                   std::vector<gm_wall_clearance_station> &stations,
                                                   std::vector<gm_wall_clearance_cell> &cells)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapClearance: createWallMap first");
    gm_wall_info wi;
    check(gm_wall_map_info(wall_, &wi), "wallMapClearance");
    if (gauge_q.empty() || gauge_q.size() % wi.n_sectors) throw Error(GM_ERR_INVALID_ARG, "wallMapClearance: gauge_q is not whole tables of n_sectors entries");
    if (!station_gauge.empty() && station_gauge.size() != n) throw Error(GM_ERR_INVALID_ARG, "wallMapClearance: station_gauge needs one entry per window station");
    const unsigned n_gauges = (unsigned)(gauge_q.size() / wi.n_sectors);
    const uint8_t *sg = station_gauge.empty() ? 0 : &station_gauge[0];
    gm_wall_clearance_info info;
    uint64_t count = 0;
    check(gm_wall_map_clearance(wall_, station0, n, &gauge_q[0], n_gauges, sg, &prm, &info, 0, 0, 0, 0, &count), "wallMapClearance");
    stations.resize(n);
    cells.resize((size_t)count);
    if (n)
        check(gm_wall_map_clearance(wall_, station0, n, &gauge_q[0], n_gauges, sg, &prm, &info, &stations[0], n,
                                    count ? &cells[0] : 0, count, &count), "wallMapClearance");
    return info;
}

gm_wall_sections_info Processor::wallMapSections(unsigned station0, unsigned n, const gm_wall_section_params &prm,
                                                 std::vector<gm_wall_section> &sections, gm_wall_map *baseline,
                                                 std::vector<gm_wall_section_sums> *sums)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapSections: createWallMap first");
    gm_wall_sections_info info;
    uint32_t count = 0;
    check(gm_wall_map_sections(wall_, baseline, station0, n, &prm, &info, 0, 0, &count, 0), "wallMapSections");
    sections.assign(count, gm_wall_section());
    if (sums) sums->assign(count, gm_wall_section_sums());
    if (count)
        check(gm_wall_map_sections(wall_, baseline, station0, n, &prm, &info, &sections[0], count, &count, sums ? &(*sums)[0] : 0),
              "wallMapSections");
    return info;
}

struct gm_wall_section_metrics Processor::wallSectionMetrics(const gm_wall_params &params, const gm_wall_section &section,
                                                             unsigned harmonics)
{
    struct gm_wall_section_metrics out;
    gm_status s = gm_wall_section_metrics(&params, &section, harmonics, &out);
    if (s != GM_OK) throw Error(s, "wallSectionMetrics: the record or the parameters were refused");
    return out;
}

gm_wall_quantities_info Processor::wallMapQuantities(unsigned station0, unsigned n, const std::vector<int32_t> &lo_q,
                                                     const std::vector<int32_t> &hi_q, const gm_wall_quantity_params &prm,
                                                     std::vector<gm_wall_quantity> &records, gm_wall_map *baseline,
                                                     const std::vector<uint8_t> &section_profile, const std::vector<uint8_t> &zone,
                                                     unsigned n_zones, std::vector<int32_t> *profile_rows)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapQuantities: createWallMap first");
    gm_wall_info wi;
    check(gm_wall_map_info(wall_, &wi), "wallMapQuantities");
    if (lo_q.empty() || lo_q.size() % wi.n_sectors || hi_q.size() != lo_q.size())
        throw Error(GM_ERR_INVALID_ARG, "wallMapQuantities: lo_q and hi_q are not the same whole tables of n_sectors entries");
    if (!zone.empty() && zone.size() != wi.n_sectors) throw Error(GM_ERR_INVALID_ARG, "wallMapQuantities: zone needs one entry per sector");
    const unsigned S = prm.section_stations ? prm.section_stations : 1, NS = n ? (n - 1) / S + 1 : 0;
    if (!section_profile.empty() && section_profile.size() != NS)
        throw Error(GM_ERR_INVALID_ARG, "wallMapQuantities: section_profile needs one entry per section");
    const unsigned n_profiles = (unsigned)(lo_q.size() / wi.n_sectors);
    const uint8_t *sp = section_profile.empty() ? 0 : &section_profile[0], *zn = zone.empty() ? 0 : &zone[0];
    gm_wall_quantities_info info;
    uint32_t count = 0;
    check(gm_wall_map_quantities(wall_, baseline, station0, n, &lo_q[0], &hi_q[0], n_profiles, sp, zn, n_zones, &prm, &info, 0, 0,
                                 &count, 0), "wallMapQuantities");
    records.assign(count, gm_wall_quantity());
    if (profile_rows) profile_rows->assign((size_t)info.sections * wi.n_sectors, 0);
    if (count)
        check(gm_wall_map_quantities(wall_, baseline, station0, n, &lo_q[0], &hi_q[0], n_profiles, sp, zn, n_zones, &prm, &info,
                                     &records[0], count, &count, profile_rows ? &(*profile_rows)[0] : 0), "wallMapQuantities");
    return info;
}

struct gm_wall_quantity_metrics Processor::wallQuantityMetrics(const gm_wall_params &params, const gm_wall_quantity &record)
{
    struct gm_wall_quantity_metrics out;
    gm_status s = gm_wall_quantity_metrics(&params, &record, &out);
    if (s != GM_OK) throw Error(s, "wallQuantityMetrics: the record or the parameters were refused");
    return out;
}

std::vector<gm_wall_quantity_run> Processor::wallQuantityRuns(const gm_wall_params &params, const std::vector<gm_wall_quantity> &records,
                                                              unsigned n_zones, unsigned run_sections, bool all_zones)
{
    if (!n_zones || records.size() % n_zones) throw Error(GM_ERR_INVALID_ARG, "wallQuantityRuns: records holds n_zones records per section");
    const unsigned ns = (unsigned)(records.size() / n_zones), flags = all_zones ? GM_WALL_QUANTITY_RUNS_ALL_ZONES : 0u;
    const gm_wall_quantity *rp = records.empty() ? 0 : &records[0];
    uint32_t count = 0;
    gm_status s = gm_wall_quantity_runs(&params, rp, ns, n_zones, run_sections, flags, 0, 0, &count);
    if (s != GM_OK) throw Error(s, "wallQuantityRuns: the records or the parameters were refused");
    std::vector<gm_wall_quantity_run> runs(count);
    if (count) {
        s = gm_wall_quantity_runs(&params, rp, ns, n_zones, run_sections, flags, &runs[0], count, &count);
        if (s != GM_OK) throw Error(s, "wallQuantityRuns failed");
    }
    return runs;
}

std::vector<int32_t> Processor::wallGaugeFromPolygon(const gm_wall_params &params, const std::vector<double> &uv, const double offset[2])
{
    if (uv.empty() || uv.size() % 2) throw Error(GM_ERR_INVALID_ARG, "wallGaugeFromPolygon: uv holds (u, v) pairs");
    std::vector<int32_t> gauge(params.n_sectors ? params.n_sectors : 1);
    uint32_t got = 0;
    gm_status s = gm_wall_gauge_from_polygon(&params, &uv[0], (unsigned)(uv.size() / 2), offset, &gauge[0], (unsigned)gauge.size(), &got);
    if (s != GM_OK) throw Error(s, "wallGaugeFromPolygon: the polygon or the parameters were refused");
    gauge.resize(got);
    return gauge;
}

std::vector<gm_wall_check_point> Processor::checkWallMap(const double pose[12], const gm_wall_check_params &prm, gm_wall_check_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "checkWallMap: createWallMap first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "checkWallMap: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_map_check_frame(wall_, ctx_, slot, pose, &prm, 0), "checkWallMap");
    check_slot_ = (int)slot;
    gm_wall_check_info local;
    gm_wall_check_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_map_get_check(wall_, slot, ip, 0, 0, &count), "checkWallMap");
    std::vector<gm_wall_check_point> points(count);
    if (count) check(gm_wall_map_get_check(wall_, slot, ip, &points[0], count, &count), "checkWallMap");
    points.resize(count);
    return points;
}

gm_wall_add_info Processor::addToWallMapChecked(const double pose[12], const gm_wall_add_checked_params &prm, gm_wall_add_checked_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "addToWallMapChecked: createWallMap first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "addToWallMapChecked: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    gm_wall_add_info add;
    check(gm_wall_map_add_frame_checked(wall_, ctx_, slot, pose, &prm, &add), "addToWallMapChecked");
    if (info) check(gm_wall_map_get_add_checked(wall_, slot, info), "addToWallMapChecked");
    return add;
}

gm_wall_locate_info Processor::locateWallMap(const double pose[12], const gm_wall_locate_params &prm)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "locateWallMap: createWallMap first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "locateWallMap: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_map_locate_frame(wall_, ctx_, slot, pose, &prm), "locateWallMap");
    gm_wall_locate_info info;
    check(gm_wall_map_get_locate(wall_, slot, &info), "locateWallMap");
    return info;
}

gm_wall_align_info Processor::alignWallMap(const double pose[12], const gm_wall_align_params &prm, std::vector<gm_wall_align_score> *scores)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "alignWallMap: createWallMap first");
    if (newest_slot_ < 0) throw Error(GM_ERR_NOT_READY, "alignWallMap: no frame yet");
    const unsigned slot = (unsigned)newest_slot_;
    check(gm_wall_map_align_frame(wall_, ctx_, slot, pose, &prm, nullptr), "alignWallMap");
    gm_wall_align_info info;
    uint32_t n = 0;
    check(gm_wall_map_get_align(wall_, slot, &info, nullptr, 0, &n), "alignWallMap");
    if (scores) {
        scores->resize(n);
        check(gm_wall_map_get_align(wall_, slot, nullptr, n ? &(*scores)[0] : nullptr, n, &n), "alignWallMap");
    }
    return info;
}

std::vector<gm_wall_object> Processor::wallCheckObjects(const gm_wall_object_params &prm, gm_wall_objects_info *info)
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallCheckObjects: createWallMap first");
    if (check_slot_ < 0) throw Error(GM_ERR_NOT_READY, "wallCheckObjects: checkWallMap first");
    gm_wall_objects_info local;
    gm_wall_objects_info *ip = info ? info : &local;
    uint32_t count = 0;
    check(gm_wall_map_check_objects(wall_, (unsigned)check_slot_, &prm, ip, 0, 0, &count, 0, 0), "wallCheckObjects");
    std::vector<gm_wall_object> objects(count);
    if (count) check(gm_wall_map_check_objects(wall_, (unsigned)check_slot_, &prm, ip, &objects[0], count, &count, 0, 0), "wallCheckObjects");
    objects.resize(count);
    return objects;
}

gm_wall_info Processor::wallMapInfo()
{
    if (!wall_) throw Error(GM_ERR_NOT_READY, "wallMapInfo: createWallMap first");
    gm_wall_info info;
    check(gm_wall_map_info(wall_, &info), "wallMapInfo");
    return info;
}

MarkerArray Processor::rvizNormals(const double &leafSize, const PointCloud &cloud, const NormalCloud &nrm)
{
    const PointCloud vox = voxelGrid(leafSize, cloud);        // :217-220
    const std::vector<int> idx = nearest(cloud, vox);         // :239 (searched in the compacted cloud)
    MarkerArray out(vox.size());
    const Vector3f scale = {{0.025f, 0.075f, 0.0625f}};       // :230
    const Vector4f color = {{1, 0, 0, 1}};                    // :231
    for (size_t i = 0; i < vox.size(); ++i) {
        const Vector3f s = {{vox[i].x, vox[i].y, vox[i].z}};
        const Normal &nn = nrm.at((size_t)idx[i]);
        const Vector3f e = {{nn.normal[0], nn.normal[1], nn.normal[2]}};   // :247-249: the arrow END is the normal itself
        out[i] = rvizArrow(s, e, scale, color, "normals", (int)i);
    }
    return out;
}

MarkerArray Processor::rvizNormalsFromFrame()
{
    const PointCloud vox = voxelCentroids();                  // :217-220, computed inside the frame
    const NormalCloud vn = voxelNormals();                    // :239 + :247-249, gathered on the device
    MarkerArray out(vox.size());
    const Vector3f scale = {{0.025f, 0.075f, 0.0625f}};       // :230
    const Vector4f color = {{1, 0, 0, 1}};                    // :231
    for (size_t i = 0; i < vox.size(); ++i) {
        const Vector3f s = {{vox[i].x, vox[i].y, vox[i].z}};
        const Normal &nn = vn.at(i);
        const Vector3f e = {{nn.normal[0], nn.normal[1], nn.normal[2]}};
        out[i] = rvizArrow(s, e, scale, color, "normals", (int)i);
    }
    return out;
}

MarkerArray Processor::rvizEigens(const Vector3f &vals, const Matrix3f &vecs)
{
    MarkerArray out(3);
    const float nrm = std::sqrt(vals(0) * vals(0) + vals(1) * vals(1) + vals(2) * vals(2));
    for (int i = 0; i < 3; ++i) {
        const float e = (1.0f / nrm) * std::fabs(vals(i));    // :265
        const Vector3f scale = {{(float)(0.1 - (0.05 * e)), (float)(0.3 - (0.15 * e)), (float)(0.25 - (0.125 * e))}};  // :274-278
        const Vector4f color = {{1.0f, i == 0 ? 1.0f : 0.0f, i == 1 ? 1.0f : 0.0f, i == 2 ? 1.0f : 0.0f}};          // :280-287
        const Vector3f zero = {{0, 0, 0}};
        out[i] = rvizArrow(zero, vecs.col(i), scale, color, "eigenBasis", i);   // :289-296
    }
    return out;
}

}  // namespace gm_host
