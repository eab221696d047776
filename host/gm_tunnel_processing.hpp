// gm_tunnel_processing.hpp -- ROS-free C++ host mirror of the reference's
// processing + marker functions, implemented on the C ABI of libgm_hip.so.
//
// Same names, argument order and meaning as
//   /root/reference include/geometric_mapping/tunnel_processing.hpp:38-54,66-85
// with PCL / Eigen / ROS message types replaced by plain structs of identical
// layout, so a catkin node can convert at its edges (ros/geometric_mapping_node.cpp)
// and everything below compiles with a bare C++11 compiler -- no HIP headers.
// Unlike the reference nothing here is heap-allocated-and-leaked
// (src/tunnel_processing.cpp:131,135,171,225,261): results are values.
#ifndef GM_TUNNEL_PROCESSING_HPP
#define GM_TUNNEL_PROCESSING_HPP

#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/gm_hip.h"

namespace gm_host {

struct PointXYZ { float x, y, z, pad; };                 // = pcl::PointXYZ (16 B)
struct Normal { float normal[3]; float curvature; };      // meaningful fields of pcl::Normal
typedef std::vector<PointXYZ> PointCloud;
typedef std::vector<Normal> NormalCloud;

struct Vector3f { float v[3]; float operator()(int i) const { return v[i]; } float &operator()(int i) { return v[i]; } };
struct Vector4f { float v[4]; float operator()(int i) const { return v[i]; } };
struct Matrix3f {                                         // column-major, like Eigen::Matrix3f
    float m[9];
    float operator()(int r, int c) const { return m[3 * c + r]; }
    Vector3f col(int c) const { Vector3f o = {{m[3 * c], m[3 * c + 1], m[3 * c + 2]}}; return o; }
};

// visualization_msgs/Marker fields the reference fills (src/tunnel_processing.cpp:161-205)
struct Marker {
    std::string frame_id, ns;
    int id, type, action;
    double points[2][3];
    double scale[3];
    float color_a, color_r, color_g, color_b;
    double position[3], orientation[4];                   // pose (x,y,z,w); identity for the reference's arrows
};
typedef std::vector<Marker> MarkerArray;
enum { MARKER_ARROW = 0, MARKER_CYLINDER = 3, MARKER_ADD = 0 };   // visualization_msgs::Marker::ARROW / CYLINDER / ADD

class Error : public std::runtime_error {
public:
    Error(gm_status s, const std::string &what) : std::runtime_error(what), status(s) {}
    gm_status status;
};

// Owns the gm_ctx; the reference's globals `params` + per-call PCL objects collapse into this.
class Processor {
public:
    // names/defaults: include/geometric_mapping/paramHandler.hpp:26-29, launch/mapping.launch:7-10
    Processor(double boxFilterBound = 5.0, double voxelGridLeafSize = 0.5, double neighborRadius = 0.5,
              double weightingFactor = 0.2, int device = 0, unsigned flags = GM_CFG_DEFAULT);
    // Several devices: frames are streamed round-robin over them (gm_group_submit_frame / gm_group_wait_frame,
    // `slots_per_device` frames in flight on each) -- the reference's one-frame-at-a-time consumer
    // (src/geometric_mapping.cpp:146,169) becomes a pipeline as deep as capacity().  processFrame() keeps working
    // (submit + wait), the stage calls use the first device.
    Processor(double boxFilterBound, double voxelGridLeafSize, double neighborRadius, double weightingFactor,
              const std::vector<int> &devices, unsigned flags, unsigned slots_per_device = 2);
    ~Processor();

    // ---- streaming (any constructor; with one device and one slot it degenerates to processFrame) ----
    unsigned capacity() const;        // frames that can be in flight
    unsigned inFlight() const;
    void submitFrame(const void *rows, unsigned n_points, unsigned point_step, unsigned off_x, unsigned off_y, unsigned off_z,
                     bool bigendian = false);   // the rows may be released on return
    gm_frame_result waitFrame();      // the oldest frame in flight; the accessors below then refer to it
    // the same without blocking: false (and `result` untouched) while the oldest frame in flight is still running or when
    // nothing is in flight (gm_poll_frame / gm_group_poll_frame).  The reference publishes each frame inside its own
    // callback (src/geometric_mapping.cpp:100-117); a host with frames in flight calls this at the top of every
    // callback and from a timer, and publishes whatever has finished.
    bool tryWaitFrame(gm_frame_result &result);
    // /choppedCloud straight into page-locked host rows (gm_set_cloud_output): one buffer per slot of every device, each
    // with room for max_points rows (grown when a larger frame is submitted).  The copy overlaps the tail of the frame;
    // choppedCloud() then reads those rows instead of fetching the cloud from the device.  Rows replaced by a growth stay
    // allocated while a frame that wrote into them is in flight or is the frame the accessors refer to.
    void enableCloudOutput(unsigned max_points);

    // ---- tunnel_processing.hpp:38-54 ----
    PointCloud chopCloud(const double &bound, const PointCloud &cloud);
    // compacts `cloud` in place (NaN-normal rows removed), like the reference (:81-85)
    NormalCloud getNormals(const double &neighborRadius, PointCloud &cloud);
    void getLocalFrame(const int &cloudSize, const double &weightingFactor, const NormalCloud &cloud_normals,
                       Vector3f &eigenVals, Matrix3f &eigenVecs);
    // the pcl::VoxelGrid half of rvizNormals (:214-220)
    PointCloud voxelGrid(const double &leafSize, const PointCloud &cloud);
    // kdtree->nearestKSearch(q, 1) (:237-239)
    std::vector<int> nearest(const PointCloud &cloud, const PointCloud &queries);

    // ---- the whole callback (src/geometric_mapping.cpp:55-92) in one device pass ----
    gm_frame_result processFrame(const void *rows, unsigned n_points, unsigned point_step, unsigned off_x, unsigned off_y,
                                 unsigned off_z, bool bigendian = false);
    PointCloud choppedCloud();        // /choppedCloud of the last frame
    NormalCloud normals();
    PointCloud voxelCentroids();
    NormalCloud voxelNormals();       // normals->at(kIndices[0]) per voxel centroid (needs GM_CFG_NEAREST)

    // ---- tunnel_processing.hpp:66-85 (pure host formatting, no device work) ----
    static Marker rvizArrow(const Vector3f &start, const Vector3f &end, const Vector3f &scale, const Vector4f &color,
                            const std::string &ns, const int &id = 0, const std::string &frame = "/velodyne");
    MarkerArray rvizNormals(const double &leafSize, const PointCloud &cloud, const NormalCloud &normals);
    // the same markers from what the last processFrame already left on the device (context created with
    // GM_CFG_NEAREST): voxel centroids + the normal of each centroid's nearest point -- a few KB of D2H, no second
    // voxel grid / 1-NN pass, no upload of the cloud
    MarkerArray rvizNormalsFromFrame();
    static MarkerArray rvizEigens(const Vector3f &eigenVals, const Matrix3f &eigenVecs);
    // The reference's unfinished cylinder output (getCylinder stub src/tunnel_processing.cpp:149-154, publisher
    // "centerAxisOutput" of type Marker src/geometric_mapping.cpp:41,119-121,163-165, param displayCylinder
    // launch/mapping.launch:15): one CYLINDER marker from gm_frame_result.cylinder (needs GM_CFG_RANSAC_CYLINDER),
    // centred on the axis point nearest the sensor origin, z axis along the fitted axis, `length` metres long.
    // Returns false (marker untouched) when the frame produced no cylinder.
    static bool rvizCylinder(const gm_frame_result &result, const double &length, Marker &marker,
                             const std::string &frame = "/velodyne");
    // The same marker from the least-squares fit (gm_cylinder_fit): centred on fit.point, z axis along fit.axis, diameter
    // 2 * fit.radius.  Returns false (marker untouched) when the fit failed (status GM_FIT_NO_MODEL / _DEGENERATE /
    // _SINGULAR).
    static bool rvizCylinder(const gm_cylinder_fit &fit, const double &length, Marker &marker,
                             const std::string &frame = "/velodyne");
    // getCylinder (tunnel_processing.hpp:56-59, whose body is the empty "//Regression function" stub of
    // src/tunnel_processing.cpp:149-154): least-squares cylinder (gm_fit_cylinder) from `init` = point, direction,
    // radius over the points with labels[i] == want (every point when `labels` is empty); `inliers` (may be null)
    // receives 1 for each final inlier.  A failed fit is reported in the status, not thrown.
    gm_cylinder_fit getCylinder(const PointCloud &cloud, const float init[7], const double &tau,
                                const std::vector<uint8_t> &labels = std::vector<uint8_t>(), unsigned want = 0,
                                std::vector<uint8_t> *inliers = 0);
    // the fit of the frame the accessors refer to (context created with GM_CFG_CYLINDER_FIT)
    gm_cylinder_fit cylinderFit();
    // Wall deviation map (GM_CFG_SURFACE_MAP, include/gm_hip.h): the map parameters of the frames processed after the
    // call, on every device (gm_set_surface_params; throws GM_ERR_NOT_READY while frames are in flight) ...
    void setSurfaceParams(const gm_surface_params &params);
    // ... and the map of the frame the accessors refer to: info and the cells, row-major [n_stations][n_sectors]
    void getSurfaceMap(gm_surface_info &info, std::vector<gm_surface_cell> &cells);
    // Persistent wall map (gm_wall_*, include/gm_hip.h): one map against a design cylinder, owned by the processor's
    // context (single device; GM_ERR_UNSUPPORTED with several).  createWallMap replaces the map of an earlier call.
    void createWallMap(const gm_wall_params &params);
    // the same on a circular-arc design axis (gm_wall_map_create_arc): one map per alignment element, straight or arc.
    // locateWallMap and alignWallMap throw GM_ERR_UNSUPPORTED on such a map (locateWallAlignment below locates on curves).
    void createWallMap(const gm_wall_params &params, const gm_wall_arc *arc);
    // the same on a clothoid design axis (gm_wall_map_create_clothoid; arc must then be NULL): with it an alignment of
    // straights, transition curves and arcs is one map per element.  locateWallMap and alignWallMap throw
    // GM_ERR_UNSUPPORTED on such a map too.
    void createWallMap(const gm_wall_params &params, const gm_wall_arc *arc, const gm_wall_clothoid *clothoid);
    // adds the frame just processed or submitted (the newest one) under pose = row-major 3x4 [R | t], sensor -> map.
    // Enqueued behind the frame's work: call it right after submitFrame, or after processFrame / waitFrame.
    gm_wall_add_info addToWallMap(const double pose[12]);
    // stations [station0, station0 + n) as records, row-major [n][n_sectors] (waits for the adds enqueued so far)
    void readWallMap(unsigned station0, unsigned n, std::vector<gm_surface_cell> &cells);
    gm_wall_info wallMapInfo();
    // connected deviation regions of stations [station0, station0 + n) against the design (gm_wall_map_regions),
    // ascending by label; info, when given, receives the call's counts
    std::vector<gm_wall_region> wallMapRegions(unsigned station0, unsigned n, const gm_wall_region_params &prm, gm_wall_regions_info *info = nullptr);
    // stations [station0, station0 + n) as a point list (gm_wall_map_cloud): one record per block of cells that holds
    // prm.min_count points, ascending by block; info, when given, receives the call's counts
    std::vector<gm_wall_cloud_point> wallMapCloud(unsigned station0, unsigned n, const gm_wall_cloud_params &prm, gm_wall_cloud_info *info = nullptr);
    // stations [station0, station0 + n) as an indexed triangle mesh (gm_wall_map_mesh): vertices receives wallMapCloud's
    // rows under prm.cloud, triangles three indices into them per face (either may be null: not wanted); info, when
    // given, receives the call's counts.  A TRIANGLE_LIST marker takes the vertices' x, y, z in the triangles' order.
    void wallMapMesh(unsigned station0, unsigned n, const gm_wall_mesh_params &prm, std::vector<gm_wall_cloud_point> *vertices, std::vector<gm_wall_mesh_triangle> *triangles, gm_wall_mesh_info *info = nullptr);
    // stations [station0, station0 + n) against a structure gauge (gm_wall_map_clearance): gauge_q holds whole tables of
    // n_sectors entries (2^-20 m, 0 = not gauged), station_gauge one table index per window station (empty: table 0
    // everywhere).  stations receives one record per station, cells the tight and the infringed cells ascending by
    // cell; the map is not changed.  A call for the end of a drive or for one window, not for every frame.
    gm_wall_clearance_info wallMapClearance(unsigned station0, unsigned n, const std::vector<int32_t> &gauge_q,
                                            const std::vector<uint8_t> &station_gauge, const gm_wall_clearance_params &prm,
                                            std::vector<gm_wall_clearance_station> &stations,
                                            std::vector<gm_wall_clearance_cell> &cells);
    // one gauge table from a closed simple polygon uv = (u0, v0, u1, v1, ...) in the section plane, metres about the
    // design axis, shifted by offset (may be null): gm_wall_gauge_from_polygon, host only
    static std::vector<int32_t> wallGaugeFromPolygon(const gm_wall_params &params, const std::vector<double> &uv,
                                                     const double offset[2] = 0);
    // the profile fit per section of stations [station0, station0 + n) (gm_wall_map_sections): convergence, centre and
    // ovalisation per chainage, against the design or, with baseline (another map on the same grid, of this context),
    // against that epoch.  One record per section; sums, when given, receives each section's last fitting pass; the map
    // is not changed.  A call for the end of a drive or for a service, not for every frame.
    gm_wall_sections_info wallMapSections(unsigned station0, unsigned n, const gm_wall_section_params &prm,
                                          std::vector<gm_wall_section> &sections, gm_wall_map *baseline = 0,
                                          std::vector<gm_wall_section_sums> *sums = 0);
    // the fp64 metrics of one record of wallMapSections under the map's parameters (gm_wall_section_metrics, host only)
    static struct gm_wall_section_metrics wallSectionMetrics(const gm_wall_params &params, const gm_wall_section &section,
                                                             unsigned harmonics);
    // under- and overbreak per section and zone of stations [station0, station0 + n) (gm_wall_map_quantities) against the
    // two lines lo_q / hi_q (whole tables of n_sectors offsets, units of 2^-20 m) about the design radius or, with baseline
    // (another map on the same grid, of this context), about that epoch's wall.  section_profile (empty: table 0) picks each
    // section's table, zone (empty: zone 0; 0xFF: not measured) each sector's zone.  One record per section and zone,
    // ordered [sections][n_zones]; profile_rows, when given, receives [sections][n_sectors]; the map is not changed.
    gm_wall_quantities_info wallMapQuantities(unsigned station0, unsigned n, const std::vector<int32_t> &lo_q,
                                              const std::vector<int32_t> &hi_q, const gm_wall_quantity_params &prm,
                                              std::vector<gm_wall_quantity> &records, gm_wall_map *baseline = 0,
                                              const std::vector<uint8_t> &section_profile = std::vector<uint8_t>(),
                                              const std::vector<uint8_t> &zone = std::vector<uint8_t>(), unsigned n_zones = 1,
                                              std::vector<int32_t> *profile_rows = 0);
    // the fp64 metrics of one record of wallMapQuantities under the map's parameters (gm_wall_quantity_metrics, host only)
    static struct gm_wall_quantity_metrics wallQuantityMetrics(const gm_wall_params &params, const gm_wall_quantity &record);
    // the records folded into pay intervals of run_sections sections (gm_wall_quantity_runs, host only)
    static std::vector<gm_wall_quantity_run> wallQuantityRuns(const gm_wall_params &params, const std::vector<gm_wall_quantity> &records,
                                                              unsigned n_zones, unsigned run_sections, bool all_zones = false);
    // the changed points of the newest frame (as addToWallMap takes it) against the map under pose (gm_wall_map_check_frame +
    // gm_wall_map_get_check), ascending by index; the map is not changed.  info, when given, receives the call's counts.
    // Check, then addToWallMap: against what was there, then contribute.
    std::vector<gm_wall_check_point> checkWallMap(const double pose[12], const gm_wall_check_params &prm, gm_wall_check_info *info = nullptr);
    // addToWallMap less the points the last checkWallMap of the newest frame selected (gm_wall_map_add_frame_checked +
    // gm_wall_map_get_add_checked): the order per frame is then locate, align, checkWallMap, addToWallMapChecked.  info, when
    // given, receives the call's counts (and the call waits for them).  GM_ERR_NOT_READY without a check of this frame.
    gm_wall_add_info addToWallMapChecked(const double pose[12], const gm_wall_add_checked_params &prm, gm_wall_add_checked_info *info = nullptr);
    // the pose of the newest frame corrected against the map (gm_wall_map_locate_frame + gm_wall_map_get_locate): the lateral
    // offset and the tilt against the axis are estimated, chainage and roll stay the caller's; the map is not changed.
    // info.pose is the corrected pose (NaN when info.status & GM_LOCATE_FAILED_MASK).  The order per frame: locateWallMap,
    // alignWallMap with the located pose, then checkWallMap and addToWallMap with the aligned pose.
    gm_wall_locate_info locateWallMap(const double pose[12], const gm_wall_locate_params &prm);
    // chainage and roll of the newest frame's pose against the map's texture (gm_wall_map_align_frame +
    // gm_wall_map_get_align): the frame's deviation image is slid over the map's in whole cells and refined by a parabola;
    // the map is not changed.  info.pose is the aligned pose (NaN when info.status & GM_ALIGN_FAILED_MASK; published under
    // GM_ALIGN_AMBIGUOUS and GM_ALIGN_AT_BORDER, which say how far to trust it).  scores, when given, receives the table of
    // (2A + 1)(2B + 1) records.
    gm_wall_align_info alignWallMap(const double pose[12], const gm_wall_align_params &prm,
                                    std::vector<gm_wall_align_score> *scores = nullptr);
    // the changed points of the last checkWallMap grouped into objects on the device (gm_wall_map_check_objects on the slot
    // that check ran on), ascending by (label, sign); the check's result and the map are not changed, and the call may be
    // repeated with other parameters.  info, when given, receives the call's counts.
    std::vector<gm_wall_object> wallCheckObjects(const gm_wall_object_params &prm, gm_wall_objects_info *info = nullptr);
    gm_wall_map *wallMap() { return wall_; }
    // Wall alignment (gm_wall_alignment_*, include/gm_hip.h): one wall map per element -- straight, arc, clothoid -- chained
    // end to end from the template `params` (element 0's frame and the grid of every element), owned by the processor's
    // context (single device).  createWallAlignment replaces the alignment of an earlier call.
    void createWallAlignment(const gm_wall_params &params, const std::vector<gm_wall_element> &elements);
    // adds the newest frame (as addToWallMap takes it) to the element maps within its reach in one launch
    // (gm_wall_alignment_add_frame): every point goes to the one element that owns it.  The products run per element map,
    // gm_wall_alignment_map(wallAlignment(), i, &map), over the pieces of gm_wall_alignment_window.
    gm_wall_alignment_add_info addToWallAlignment(const double pose[12]);
    // corrects the newest frame's pose against the alignment (gm_wall_alignment_locate_frame + gm_wall_alignment_get_locate):
    // locateWallMap on straight, arc and clothoid elements and across their joints; the element maps are not changed.
    // info.pose is the corrected pose (NaN when info.status & GM_LOCATE_FAILED_MASK).  The order per frame on an alignment:
    // locateWallAlignment, checkWallAlignment with the located pose, addToWallAlignmentChecked with it.
    gm_wall_alignment_locate_info locateWallAlignment(const double pose[12], const gm_wall_locate_params &prm);
    // the newest frame's chainage and roll against the alignment (gm_wall_alignment_align_frame + gm_wall_alignment_get_align):
    // alignWallMap on straight, arc and clothoid elements and across their joints; the element maps are not changed.
    // info.pose is the aligned pose (NaN when info.status & GM_ALIGN_FAILED_MASK); scores and plan, when given, receive the
    // score table and the plan of the call's sides and pieces.  The order per frame on an alignment: locateWallAlignment,
    // alignWallAlignment with the located pose, checkWallAlignment with the aligned pose, addToWallAlignmentChecked with it.
    gm_wall_alignment_align_info alignWallAlignment(const double pose[12], const gm_wall_align_params &prm,
                                                    std::vector<gm_wall_align_score> *scores = nullptr,
                                                    gm_wall_alignment_align_plan_info *plan = nullptr);
    // the changed points of the newest frame against the alignment under pose (gm_wall_alignment_check_frame +
    // gm_wall_alignment_get_check): every point against the map of the element that owns it, ascending by index; a row's
    // cell holds side << 24 | cell (GM_WALL_ROW_SIDE, GM_WALL_ROW_CELL; side indexes plan->side_element).  The element maps
    // are not changed.  info and plan, when given, receive the call's counts and the plan of its sides.
    std::vector<gm_wall_check_point> checkWallAlignment(const double pose[12], const gm_wall_check_params &prm,
                                                        gm_wall_alignment_check_info *info = nullptr,
                                                        gm_wall_alignment_add_info *plan = nullptr);
    // addToWallAlignment less the points the last checkWallAlignment of the newest frame selected
    // (gm_wall_alignment_add_frame_checked + gm_wall_alignment_get_add_checked).  info, when given, receives the call's counts
    // (and the call waits for them).  GM_ERR_NOT_READY without a check of this frame through the alignment.
    gm_wall_alignment_add_info addToWallAlignmentChecked(const double pose[12], const gm_wall_add_checked_params &prm,
                                                         gm_wall_add_checked_info *info = nullptr);
    // the objects of the last checkWallAlignment's changed points on the alignment's global station grid, ascending by
    // (label, sign) (gm_wall_alignment_check_objects: a count query, then the sized call; the rows stay on the device): an
    // object across a joint plane is one object, and station_min / station_max are global stations
    // (gm_wall_alignment_object_metrics gives the chainage and the elements).  The order per frame on an alignment:
    // locateWallAlignment, alignWallAlignment, checkWallAlignment, wallAlignmentCheckObjects, addToWallAlignmentChecked.
    std::vector<gm_wall_object> wallAlignmentCheckObjects(const gm_wall_object_params &prm, gm_wall_alignment_objects_info *info = nullptr);
    // the connected deviation regions of the alignment's global stations [station0, station0 + n)
    // (gm_wall_alignment_regions, without a baseline): wallRegions across joints -- a region that lies across a joint plane
    // is one record, with global stations and global cell indices; ascending by label.  A count query, then the sized call.
    std::vector<gm_wall_region> wallAlignmentRegions(const gm_wall_region_params &prm, uint32_t station0, uint32_t n,
                                                     gm_wall_alignment_regions_info *info = nullptr);
    gm_wall_alignment *wallAlignment() { return alignment_; }

    gm_ctx *ctx() { return ctx_; }

private:
    void check(gm_status s, const char *what);
    gm_ctx *ctx_;          // the context the stage calls run on (the group's first rank when there is a group)
    gm_group *grp_;        // several devices: owns the contexts
    gm_ctx *cur_;          // where the last completed frame's bulky outputs live ...
    unsigned cur_slot_;    // ... and in which slot
    unsigned n_slots_, next_slot_, pending_;   // single device: ring of slots
    gm_frame_result last_;                     // of the frame the accessors refer to
    gm_wall_map *wall_;                        // createWallMap (freed with the context)
    gm_wall_alignment *alignment_;             // createWallAlignment (freed with the context)
    int newest_slot_;                          // slot of the frame submitted last (-1: none yet)
    int check_slot_;                           // the slot of the last checkWallMap, -1 before it
    int al_check_slot_;                        // the slot of the last checkWallAlignment, -1 before it
    // enableCloudOutput: one per (device, slot).  `rows` receive the slot's frames from number `since` on (frames are
    // numbered in submission order, which is the order they are waited for in).  Rows that were replaced while a frame that
    // wrote into them could still be read are kept in `retired`, oldest first, and freed by a later growCloudOutput.
    struct CloudRows { float *rows; unsigned long long since; };
    struct CloudBuf { gm_ctx *ctx; unsigned slot; float *rows; unsigned cap; unsigned long long since; std::vector<CloudRows> retired; };
    std::vector<CloudBuf> cloud_bufs_;
    unsigned long long submitted_, waited_;    // frames handed to the library / taken back from it (the accessors' frame: waited_ - 1)
    void growCloudOutput(unsigned n_points);
    void freeRetiredCloudRows();
    Processor(const Processor &);
    Processor &operator=(const Processor &);
};

}  // namespace gm_host
#endif
