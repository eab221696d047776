"""ctypes binding of libgm_hip.so -- the C ABI declared in include/gm_hip.h.

There is deliberately NO fallback here: if the library is missing or does not
load, importing callers get an exception.  Nothing in this package imports
oracle/ (the CPU restatement is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgm_hip.so")
if os.environ.get("GM_LIB_PATH"):   # experiments only (tools/build_variants.sh): another build of the same library
    LIB_PATH = os.environ["GM_LIB_PATH"]
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gm_hip.h")

GM_OK = 0
GM_ERR_INVALID_ARG = 1
GM_ERR_TOO_FEW_POINTS = 2
GM_ERR_DEVICE = 3
GM_ERR_OOM = 4
GM_ERR_CAPACITY = 5
GM_ERR_NOT_READY = 6
GM_ERR_UNSUPPORTED = 7
GM_ERR_COMM = 8
GM_GROUP_LOOPBACK = 1
GM_GROUP_N_TIMINGS = 5

GM_CFG_VOXEL_GRID = 1 << 0
GM_CFG_NEAREST = 1 << 1
GM_CFG_RANSAC_PLANE = 1 << 2
GM_CFG_RANSAC_CYLINDER = 1 << 3
GM_CFG_STAGE_TIMING = 1 << 4
GM_CFG_KEEP_COUNTS = 1 << 5
GM_CFG_GRAPH = 1 << 6
GM_CFG_CYLINDER_FIT = 1 << 7
GM_CFG_SURFACE_MAP = 1 << 8
GM_CFG_DEFAULT = GM_CFG_VOXEL_GRID

GM_CLOUD_DEVICE = 1 << 0
GM_CLOUD_BIGENDIAN = 1 << 1
GM_CLOUD_PINNED = 1 << 2

GM_RES_VOXEL_PASSTHROUGH = 1 << 0

GM_FIT_OK = 0
GM_FIT_NO_MODEL = 1
GM_FIT_DEGENERATE = 2
GM_FIT_SINGULAR = 3
GM_FIT_FAILED_MASK = 0xFF
GM_FIT_NOT_CONVERGED = 1 << 8
GM_FIT_STEP_BOUND = 1e-2

GM_SURF_MAX_CELLS = 4096
GM_SURF_OK = 0
GM_SURF_NO_MODEL = 1
GM_SURF_UP_FALLBACK = 1 << 8

GM_WALL_MAX_CELLS = 1 << 24
GM_WALL_MAX_SECTORS = 4096
GM_WALL_REGION_TILE = (64, 64)   # stations x sectors: the labelling kernel's default tile

GM_WALL_OBJECT_MAX_BLOCKS = 1 << 20
GM_WALL_OBJECT_TILE = (64, 64)   # block rows x block columns: the object labelling kernel's default tile

GM_WALL_CHECK_MEAN, GM_WALL_CHECK_ENVELOPE = 0, 1
GM_WALL_SKIP_NEG, GM_WALL_SKIP_POS = 1, 2
GM_WALL_CLEAR_MIN, GM_WALL_CLEAR_MEAN = 0, 1
GM_WALL_CLEAR_MAX_GAUGES = 256
GM_SECTION_OK = 0
GM_SECTION_TOO_FEW, GM_SECTION_SINGULAR, GM_SECTION_UNBOUNDED = 1 << 0, 1 << 1, 1 << 2
GM_SECTION_FAILED_MASK = 0xFF
GM_SECTION_OPEN_ARC = 1 << 8
GM_WALL_SECTION_MAX_HARMONICS, GM_WALL_SECTION_MAX_PASSES = 4, 4
GM_WALL_GAUGE_MAX_VERTICES = 4096
GM_WALL_LOCATE_DESIGN, GM_WALL_LOCATE_MAP = 0, 1
GM_LOCATE_OK = 0
GM_LOCATE_DEGENERATE = 2
GM_LOCATE_SINGULAR = 3
GM_LOCATE_FAILED_MASK = 0xFF
GM_LOCATE_NOT_CONVERGED = 1 << 8
GM_LOCATE_PASSES = 3
GM_WALL_ALIGN_MAX_PATCH_CELLS = 8192
GM_WALL_ALIGN_MAX_SHIFT = 64
GM_WALL_ALIGN_MAX_SHIFTS = 4096
GM_ALIGN_OK = 0
GM_ALIGN_NO_OVERLAP = 2
GM_ALIGN_FAILED_MASK = 0xFF
GM_ALIGN_AMBIGUOUS = 1 << 8
GM_ALIGN_AT_BORDER = 1 << 9
(GM_WALL_CHECK_CLS_PLANE, GM_WALL_CHECK_CLS_BEYOND_GATE, GM_WALL_CHECK_CLS_OUTSIDE, GM_WALL_CHECK_CLS_UNSURVEYED,
 GM_WALL_CHECK_CLS_UNCHANGED, GM_WALL_CHECK_CLS_CHANGED_POS, GM_WALL_CHECK_CLS_CHANGED_NEG) = range(7)

GM_N_STAGES = 9
STAGE_NAMES = ("upload", "crop", "grid", "normals", "compact", "frame", "voxel", "ransac", "total")


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("boxFilterBound", C.c_double), ("voxelGridLeafSize", C.c_double),
                ("neighborRadius", C.c_double), ("weightingFactor", C.c_double),
                ("device", C.c_int32), ("n_slots", C.c_uint32), ("max_points", C.c_uint32),
                ("ransac_hypotheses", C.c_uint32), ("ransac_threshold", C.c_double),
                ("ransac_seed", C.c_uint64)]


class Cloud(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_points", C.c_uint32), ("point_step", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32), ("flags", C.c_uint32)]


class FrameResult(C.Structure):
    _fields_ = [("n_in", C.c_uint32), ("n_cropped", C.c_uint32), ("n_valid", C.c_uint32), ("n_voxels", C.c_uint32),
                ("eigenvalues", C.c_float * 3), ("eigenvectors", C.c_float * 9), ("center_axis", C.c_float * 3),
                ("status_flags", C.c_uint32), ("scatter", C.c_double * 6),
                ("plane_inliers", C.c_uint32), ("cylinder_inliers", C.c_uint32),
                ("plane", C.c_float * 4), ("cylinder", C.c_float * 7),
                ("plane_refit", C.c_double * 4), ("cylinder_axis_refit", C.c_double * 3),
                ("stage_ms", C.c_float * GM_N_STAGES), ("normals_kernel_ms", C.c_float)]


class CylinderFit(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("inliers", C.c_uint32), ("passes", C.c_uint32),
                ("point", C.c_double * 3), ("axis", C.c_double * 3), ("radius", C.c_double), ("rms", C.c_double),
                ("last_step", C.c_double), ("model", C.c_float * 7)]


class SurfaceParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32), ("reserved", C.c_uint32),
                ("station_length", C.c_double), ("t_min", C.c_double), ("gate", C.c_double),
                ("up", C.c_double * 3), ("forward", C.c_double * 3)]


class SurfaceCell(C.Structure):
    _fields_ = [("count", C.c_uint32), ("mean", C.c_float), ("min", C.c_float), ("max", C.c_float)]


class SurfaceInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("mapped", C.c_uint32), ("outside", C.c_uint32), ("beyond_gate", C.c_uint32), ("plane", C.c_uint32),
                ("cells_hit", C.c_uint32), ("reserved", C.c_uint32),
                ("o", C.c_float * 3), ("a", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("R", C.c_float), ("t_min", C.c_float), ("station_length", C.c_float), ("sector_angle", C.c_float)]


class WallArc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("curvature", C.c_double * 3),
                ("point_chainage", C.c_double)]


class WallArcAddInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("anchor_station", C.c_int64),
                ("sensor_chainage", C.c_double), ("anchor_chainage", C.c_double),
                ("o", C.c_float * 3), ("a", C.c_float * 3), ("n", C.c_float * 3), ("b", C.c_float * 3),
                ("kappa", C.c_float), ("un", C.c_float), ("ub", C.c_float), ("vn", C.c_float), ("vb", C.c_float),
                ("R", C.c_float), ("station_length", C.c_float), ("sector_angle", C.c_float), ("gate", C.c_float),
                ("reserved", C.c_uint32)]


class WallClothoid(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("normal", C.c_double * 3), ("curvature", C.c_double),
                ("rate", C.c_double), ("point_chainage", C.c_double)]


class WallClothoidAddInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("anchor_station", C.c_int64),
                ("sensor_chainage", C.c_double), ("anchor_chainage", C.c_double),
                ("o", C.c_float * 3), ("a", C.c_float * 3), ("n", C.c_float * 3), ("b", C.c_float * 3),
                ("kappa", C.c_float), ("un", C.c_float), ("ub", C.c_float), ("vn", C.c_float), ("vb", C.c_float),
                ("R", C.c_float), ("station_length", C.c_float), ("sector_angle", C.c_float), ("gate", C.c_float),
                ("rate", C.c_float), ("reserved", C.c_uint32 * 2)]


class WallElement(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("n_stations", C.c_uint32), ("reserved", C.c_uint32),
                ("turn", C.c_double * 2), ("curvature", C.c_double), ("rate", C.c_double)]


class WallAlignmentPiece(C.Structure):
    _fields_ = [("element", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("reserved", C.c_uint32)]


class WallAlignmentAddInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("element", C.c_uint32), ("n_sides", C.c_uint32),
                ("chainage", C.c_double), ("reach", C.c_double), ("side_element", C.c_uint32 * 4),
                ("side_anchor", C.c_int64 * 4), ("joint_o", (C.c_float * 3) * 3), ("joint_a", (C.c_float * 3) * 3),
                ("offset", C.c_double)]


class WallAlignmentTotals(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_elements", C.c_uint32), ("n_stations", C.c_uint64),
                ("chainage_min", C.c_double), ("chainage_max", C.c_double), ("frames", C.c_uint64),
                ("mapped", C.c_uint64), ("outside", C.c_uint64), ("beyond_gate", C.c_uint64), ("plane", C.c_uint64)]


class WallParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32), ("reserved", C.c_uint32),
                ("station_length", C.c_double), ("t_min", C.c_double), ("gate", C.c_double),
                ("point", C.c_double * 3), ("direction", C.c_double * 3), ("radius", C.c_double),
                ("up", C.c_double * 3), ("forward", C.c_double * 3)]


class WallRawCell(C.Structure):
    _fields_ = [("sum", C.c_int64), ("count", C.c_uint32), ("min_key", C.c_uint32), ("max_key", C.c_uint32),
                ("reserved", C.c_uint32)]


class WallAddInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("anchor_station", C.c_int64),
                ("o", C.c_float * 3), ("a", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("R", C.c_float), ("station_length", C.c_float), ("sector_angle", C.c_float), ("gate", C.c_float)]


class WallInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("frames", C.c_uint64), ("mapped", C.c_uint64), ("outside", C.c_uint64), ("beyond_gate", C.c_uint64),
                ("plane", C.c_uint64), ("cells_hit", C.c_uint64),
                ("o", C.c_double * 3), ("a", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3), ("R", C.c_double)]


class WallRegion(C.Structure):
    _fields_ = [("label", C.c_uint32), ("sign", C.c_int32), ("cells", C.c_uint32),
                ("station_min", C.c_uint32), ("station_max", C.c_uint32), ("sector_min", C.c_uint32), ("sector_max", C.c_uint32),
                ("sector_min_turned", C.c_uint32), ("sector_max_turned", C.c_uint32), ("peak_cell", C.c_uint32),
                ("peak", C.c_int64), ("sum_d", C.c_int64), ("points", C.c_uint64)]


class WallRegionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_count", C.c_uint32), ("min_cells", C.c_uint32), ("connectivity", C.c_uint32),
                ("threshold", C.c_double), ("reserved", C.c_uint64)]


class WallRegionsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("threshold_q", C.c_int64), ("flagged_pos", C.c_uint64), ("flagged_neg", C.c_uint64), ("unusable", C.c_uint64),
                ("empty", C.c_uint64), ("components", C.c_uint64), ("regions", C.c_uint64), ("cell_area", C.c_double)]


class WallRegionMetrics(C.Structure):
    _fields_ = [("area_m2", C.c_double), ("volume_m3", C.c_double), ("peak_m", C.c_double), ("mean_m", C.c_double),
                ("chainage_from", C.c_double), ("chainage_to", C.c_double), ("angle_from_deg", C.c_double),
                ("angle_to_deg", C.c_double)]


class WallCloudParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("block_stations", C.c_uint32), ("block_sectors", C.c_uint32),
                ("min_count", C.c_uint32), ("exaggeration", C.c_double), ("anchor", C.c_double * 3), ("reserved", C.c_uint64)]


class WallCloudPoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("mean", C.c_float), ("min", C.c_float),
                ("max", C.c_float), ("block", C.c_uint32), ("cells", C.c_uint32), ("count", C.c_uint64)]


class WallCloudInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("blocks_stations", C.c_uint32), ("blocks_sectors", C.c_uint32),
                ("blocks", C.c_uint64), ("points", C.c_uint64), ("below_min_count", C.c_uint64), ("empty", C.c_uint64)]


GM_WALL_MESH_OUTWARD = 1 << 0
GM_WALL_MESH_NO_WRAP = 1 << 1


class WallMeshParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("cloud", WallCloudParams), ("max_step", C.c_double),
                ("reserved", C.c_uint64)]


class WallMeshTriangle(C.Structure):
    _fields_ = [("v", C.c_uint32 * 3)]


class WallMeshInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("wrapped", C.c_uint32), ("cloud", WallCloudInfo), ("quads", C.c_uint64),
                ("quads_two", C.c_uint64), ("quads_one", C.c_uint64), ("quads_none", C.c_uint64), ("cut_by_step", C.c_uint64),
                ("triangles", C.c_uint64)]


class WallClearanceParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reference", C.c_uint32), ("min_count", C.c_uint32), ("reserved", C.c_uint32),
                ("margin", C.c_double)]


class WallClearanceStation(C.Structure):
    _fields_ = [("min_clearance", C.c_int64), ("min_sector", C.c_uint32), ("usable", C.c_uint32), ("tight", C.c_uint32),
                ("infringed", C.c_uint32), ("unsurveyed", C.c_uint32), ("gauge", C.c_uint32)]


class WallClearanceCell(C.Structure):
    _fields_ = [("cell", C.c_uint32), ("count", C.c_uint32), ("clearance", C.c_int64)]


class WallClearanceInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("margin_q", C.c_int64), ("radius_q", C.c_int64), ("ungauged", C.c_uint64), ("empty", C.c_uint64),
                ("unusable", C.c_uint64), ("infringed", C.c_uint64), ("tight", C.c_uint64), ("clear", C.c_uint64),
                ("stations_tight", C.c_uint32), ("stations_infringed", C.c_uint32), ("min_clearance", C.c_int64),
                ("min_cell", C.c_uint32), ("reserved", C.c_uint32)]


class WallClearanceRun(C.Structure):
    _fields_ = [("station_from", C.c_uint32), ("station_to", C.c_uint32), ("chainage_from", C.c_double),
                ("chainage_to", C.c_double), ("min_clearance", C.c_int64), ("min_clearance_m", C.c_double),
                ("min_station", C.c_uint32), ("min_sector", C.c_uint32), ("angle_deg", C.c_double), ("tight", C.c_uint64),
                ("infringed", C.c_uint64)]


class WallSectionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("section_stations", C.c_uint32), ("harmonics", C.c_uint32), ("passes", C.c_uint32),
                ("min_count", C.c_uint32), ("min_columns", C.c_uint32), ("max_gap_deg", C.c_double), ("reject", C.c_double)]


class WallSectionSums(C.Structure):
    _fields_ = [("N", C.c_int64 * 45), ("r", C.c_int64 * 9), ("fitted", C.c_uint32), ("largest_gap", C.c_uint32),
                ("points", C.c_uint64)]


class WallSection(C.Structure):
    _fields_ = [("station_from", C.c_uint32), ("stations", C.c_uint32), ("status", C.c_uint32), ("usable", C.c_uint32),
                ("fitted", C.c_uint32), ("accepted", C.c_uint32), ("rejected", C.c_uint32), ("largest_gap", C.c_uint32),
                ("points", C.c_uint64), ("coef_q", C.c_int64 * 9), ("rss", C.c_uint64), ("peak_out", C.c_int64),
                ("peak_in", C.c_int64), ("peak_out_sector", C.c_uint32), ("peak_in_sector", C.c_uint32)]


class WallSectionsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("section_stations", C.c_uint32), ("sections", C.c_uint32), ("harmonics", C.c_uint32), ("passes", C.c_uint32),
                ("reject_q", C.c_int64), ("max_gap_sectors", C.c_uint32), ("sections_ok", C.c_uint32),
                ("sections_failed", C.c_uint32), ("sections_open_arc", C.c_uint32), ("empty", C.c_uint64),
                ("unusable", C.c_uint64), ("usable", C.c_uint64), ("accepted", C.c_uint64), ("rejected", C.c_uint64)]


class WallSectionMetrics(C.Structure):
    _fields_ = [("chainage_from", C.c_double), ("chainage_to", C.c_double), ("radius_m", C.c_double), ("radial_m", C.c_double),
                ("centre_u", C.c_double), ("centre_v", C.c_double), ("centre", C.c_double * 3), ("oval_m", C.c_double),
                ("oval_angle_deg", C.c_double), ("diameter_max", C.c_double), ("diameter_min", C.c_double),
                ("rms_m", C.c_double), ("area_m2", C.c_double), ("coverage", C.c_double)]


class WallQuantityParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("section_stations", C.c_uint32), ("min_count", C.c_uint32), ("reserved", C.c_uint32)]


class WallQuantity(C.Structure):
    _fields_ = [("station_from", C.c_uint32), ("stations", C.c_uint32), ("zone", C.c_uint32), ("profile", C.c_uint32),
                ("under", C.c_uint32), ("within", C.c_uint32), ("over", C.c_uint32), ("unsurveyed", C.c_uint32),
                ("points", C.c_uint64), ("under_area", C.c_int64), ("over_area", C.c_int64), ("excess_area", C.c_int64),
                ("peak_under", C.c_int64), ("peak_over", C.c_int64), ("peak_under_sector", C.c_uint32),
                ("peak_over_sector", C.c_uint32)]


class WallQuantitiesInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32), ("n_sectors", C.c_uint32),
                ("section_stations", C.c_uint32), ("sections", C.c_uint32), ("n_zones", C.c_uint32), ("n_profiles", C.c_uint32),
                ("radius_q", C.c_int64), ("unmeasured", C.c_uint64), ("empty", C.c_uint64), ("unusable", C.c_uint64),
                ("under", C.c_uint64), ("over", C.c_uint64), ("within", C.c_uint64), ("sections_under", C.c_uint32),
                ("sections_over", C.c_uint32)]


class WallQuantityColumnResult(C.Structure):
    _fields_ = [("cls", C.c_uint32), ("v", C.c_int32), ("under_area", C.c_int64), ("over_area", C.c_int64),
                ("excess_area", C.c_int64), ("over_line", C.c_int64)]


class WallQuantityMetrics(C.Structure):
    _fields_ = [("chainage_from", C.c_double), ("chainage_to", C.c_double), ("length", C.c_double),
                ("under_area_m2", C.c_double), ("over_area_m2", C.c_double), ("excess_area_m2", C.c_double),
                ("paid_area_m2", C.c_double), ("under_volume_m3", C.c_double), ("over_volume_m3", C.c_double),
                ("excess_volume_m3", C.c_double), ("paid_volume_m3", C.c_double), ("peak_under_m", C.c_double),
                ("peak_over_m", C.c_double), ("peak_under_angle_deg", C.c_double), ("peak_over_angle_deg", C.c_double),
                ("coverage", C.c_double), ("reserved", C.c_double)]


class WallQuantityRun(C.Structure):
    _fields_ = [("station_from", C.c_uint32), ("stations", C.c_uint32), ("zone", C.c_uint32), ("sections", C.c_uint32),
                ("chainage_from", C.c_double), ("chainage_to", C.c_double), ("under", C.c_uint64), ("within", C.c_uint64),
                ("over", C.c_uint64), ("unsurveyed", C.c_uint64), ("points", C.c_uint64), ("under_volume_m3", C.c_double),
                ("over_volume_m3", C.c_double), ("excess_volume_m3", C.c_double), ("paid_volume_m3", C.c_double),
                ("peak_under", C.c_int64), ("peak_over", C.c_int64), ("peak_under_station", C.c_uint32),
                ("peak_under_sector", C.c_uint32), ("peak_over_station", C.c_uint32), ("peak_over_sector", C.c_uint32)]


class WallCheckParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reference", C.c_uint32), ("min_count", C.c_uint32), ("reserved", C.c_uint32),
                ("threshold", C.c_double), ("gate", C.c_double)]


class WallCheckPoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("delta", C.c_float), ("e", C.c_float),
                ("cell", C.c_int32), ("index", C.c_uint32), ("row", C.c_uint32)]


class WallCheckInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("threshold_q", C.c_int64), ("n_points", C.c_uint32),
                ("plane", C.c_uint32), ("beyond_gate", C.c_uint32), ("outside", C.c_uint32), ("unsurveyed", C.c_uint32),
                ("unchanged", C.c_uint32), ("changed_pos", C.c_uint32), ("changed_neg", C.c_uint32),
                ("peak_pos", C.c_int64), ("peak_neg", C.c_int64)]


class WallAlignmentCheckInfo(C.Structure):
    _fields_ = WallCheckInfo._fields_ + [("n_sides", C.c_uint32), ("reserved", C.c_uint32), ("side_class", (C.c_uint32 * 7) * 4)]


class WallAddCheckedParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("skip", C.c_uint32), ("min_delta", C.c_double)]


class WallAddCheckedInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("min_delta_q", C.c_int64), ("n_points", C.c_uint32),
                ("n_rows", C.c_uint32), ("rows_neg", C.c_uint32), ("rows_pos", C.c_uint32), ("rows_kept", C.c_uint32),
                ("rows_rejected", C.c_uint32), ("skipped", C.c_uint32), ("plane", C.c_uint32), ("beyond_gate", C.c_uint32),
                ("outside", C.c_uint32), ("mapped", C.c_uint32), ("reserved", C.c_uint32)]


class WallLocateParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reference", C.c_uint32), ("min_count", C.c_uint32), ("reserved", C.c_uint32),
                ("gate", C.c_double)]


class WallLocatePass(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("a", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("gate", C.c_float),
                ("plane", C.c_uint32), ("outside", C.c_uint32), ("unsurveyed", C.c_uint32), ("gated", C.c_uint32),
                ("used", C.c_uint32), ("rms", C.c_double), ("step", C.c_double * 4)]


class WallLocateInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("passes", C.c_uint32), ("n_points", C.c_uint32),
                ("anchor_station", C.c_int64), ("pose", C.c_double * 12), ("lateral", C.c_double * 2), ("tilt", C.c_double * 2),
                ("pass_", WallLocatePass * 3)]


class WallAlignmentLocatePass(C.Structure):
    _fields_ = WallLocatePass._fields_ + [("side", (C.c_float * 12) * 4), ("joint_o", (C.c_float * 3) * 3),
                                          ("joint_a", (C.c_float * 3) * 3)]


class WallAlignmentLocateInfo(C.Structure):
    _fields_ = WallLocateInfo._fields_[:-1] + [
        ("element", C.c_uint32), ("n_sides", C.c_uint32), ("side_element", C.c_uint32 * 4), ("side_kind", C.c_uint32 * 4),
        ("side_anchor", C.c_int64 * 4), ("side_axis", (C.c_float * 6) * 4), ("pass_", WallAlignmentLocatePass * 3)]


class WallAlignmentLocateStart(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("home", C.c_uint32), ("add", WallAlignmentAddInfo),
                ("c", C.c_double * 3), ("d", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3), ("s0", C.c_double),
                ("o_f", C.c_double * 3), ("a", C.c_double * 3), ("fu", C.c_double * 3), ("fv", C.c_double * 3),
                ("side", (C.c_double * 12) * 4), ("joint", (C.c_double * 6) * 3), ("side_axis", (C.c_float * 6) * 4),
                ("side_kind", C.c_uint32 * 4)]


class WallAlignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("half_patch_stations", C.c_uint32), ("max_station_shift", C.c_uint32),
                ("max_sector_shift", C.c_uint32), ("min_count", C.c_uint32), ("min_frame_count", C.c_uint32),
                ("min_overlap", C.c_uint32), ("reserved", C.c_uint32), ("gate", C.c_double), ("clip", C.c_double),
                ("min_distinction", C.c_double)]


class WallAlignScore(C.Structure):
    _fields_ = [("ssd", C.c_uint64), ("sum_d", C.c_int64), ("n", C.c_uint32), ("reserved", C.c_uint32)]


class WallAlignInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_uint32), ("n_points", C.c_uint32), ("plane", C.c_uint32),
                ("beyond_gate", C.c_uint32), ("outside_patch", C.c_uint32), ("binned", C.c_uint32),
                ("patch_cells_usable", C.c_uint32), ("anchor_station", C.c_int64), ("half_patch_stations", C.c_uint32),
                ("max_station_shift", C.c_uint32), ("max_sector_shift", C.c_uint32), ("overlap", C.c_uint32),
                ("best_station", C.c_int32), ("best_sector", C.c_int32), ("frac_station", C.c_double),
                ("frac_sector", C.c_double), ("shift_m", C.c_double), ("roll", C.c_double), ("bias_m", C.c_double),
                ("rms_best", C.c_double), ("rms_runner", C.c_double), ("distinction", C.c_double), ("pose", C.c_double * 12)]


class WallAlignmentAlignPiece(C.Structure):
    _fields_ = [("element", C.c_uint32), ("n_stations", C.c_uint32), ("first_row", C.c_int64)]


class WallAlignmentAlignPlan(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_pieces", C.c_uint32), ("add", WallAlignmentAddInfo),
                ("anchor_global", C.c_int64), ("total", C.c_int64), ("row0", C.c_int32 * 4), ("own", C.c_uint32),
                ("home", C.c_uint32), ("piece", WallAlignmentAlignPiece * 8)]


class WallAlignmentAlignInfo(C.Structure):
    _fields_ = WallAlignInfo._fields_ + [("element", C.c_uint32), ("n_sides", C.c_uint32), ("chainage", C.c_double),
                                         ("anchor_global", C.c_int64), ("side_class", (C.c_uint32 * 4) * 4),
                                         ("plan", WallAlignmentAddInfo)]


class WallObject(C.Structure):
    _fields_ = [("label", C.c_uint32), ("sign", C.c_int32), ("blocks", C.c_uint32), ("peak_index", C.c_uint32),
                ("station_min", C.c_uint32), ("station_max", C.c_uint32), ("sector_min", C.c_uint32), ("sector_max", C.c_uint32),
                ("sector_min_turned", C.c_uint32), ("sector_max_turned", C.c_uint32), ("points", C.c_uint64),
                ("peak", C.c_int64), ("sum_delta", C.c_int64), ("sum_x", C.c_int64), ("sum_y", C.c_int64), ("sum_z", C.c_int64),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("e_min", C.c_float), ("e_max", C.c_float),
                ("reserved", C.c_uint64)]


class WallObjectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("block_stations", C.c_uint32), ("block_sectors", C.c_uint32),
                ("min_block_points", C.c_uint32), ("min_points", C.c_uint32), ("connectivity", C.c_uint32),
                ("half_window_stations", C.c_uint32), ("reserved", C.c_uint32)]


class WallObjectsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_rows", C.c_uint32), ("station0", C.c_uint32), ("n_stations", C.c_uint32),
                ("blocks_stations", C.c_uint32), ("blocks_sectors", C.c_uint32), ("rejected", C.c_uint32),
                ("outside_window", C.c_uint32), ("sparse", C.c_uint32), ("small", C.c_uint32), ("in_object", C.c_uint32),
                ("flagged_pos", C.c_uint32), ("flagged_neg", C.c_uint32), ("components", C.c_uint32), ("objects", C.c_uint32),
                ("reserved", C.c_uint32)]


class WallObjectMetrics(C.Structure):
    _fields_ = [("centroid", C.c_double * 3), ("mean_m", C.c_double), ("peak_m", C.c_double), ("size", C.c_double * 3),
                ("chainage_from", C.c_double), ("chainage_to", C.c_double), ("angle_from_deg", C.c_double),
                ("angle_to_deg", C.c_double)]


class WallAlignmentObjectsInfo(C.Structure):
    _fields_ = WallObjectsInfo._fields_ + [("element", C.c_uint32), ("n_sides", C.c_uint32), ("anchor_global", C.c_int64),
                                           ("total", C.c_int64), ("side_element", C.c_uint32 * 4),
                                           ("side_first", C.c_uint32 * 4), ("side_rows", C.c_uint32 * 4)]


class WallAlignmentObjectMetrics(C.Structure):
    _fields_ = WallObjectMetrics._fields_ + [("element_from", C.c_uint32), ("element_to", C.c_uint32),
                                             ("station_from", C.c_uint32), ("station_to", C.c_uint32)]


class WallAlignmentRegionsInfo(C.Structure):
    _fields_ = WallRegionsInfo._fields_ + [("total", C.c_int64), ("n_pieces", C.c_uint32), ("element_from", C.c_uint32),
                                           ("element_to", C.c_uint32), ("station_from", C.c_uint32), ("station_to", C.c_uint32),
                                           ("reserved", C.c_uint32)]


class WallAlignmentRegionMetrics(C.Structure):
    _fields_ = WallRegionMetrics._fields_ + [("element_from", C.c_uint32), ("element_to", C.c_uint32),
                                             ("station_from", C.c_uint32), ("station_to", C.c_uint32),
                                             ("peak_element", C.c_uint32), ("peak_station", C.c_uint32),
                                             ("peak_sector", C.c_uint32), ("reserved", C.c_uint32), ("peak_point", C.c_double * 3)]


class GmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libgm_hip: status {status}: {message}")
        self.status = status


def info_fields(struct):
    """The field names an info or metrics dict carries: the struct's, less struct_size and reserved."""
    return tuple(k for k, _t in struct._fields_ if k not in ("struct_size", "reserved"))


def params(struct, default_fn, family, kw):
    """A parameter struct with the library's defaults (`default_fn`, its gm_*_default_params), then the keywords `kw`:
    a scalar field takes the value, an array field a sequence of floats.  struct_size, reserved and a name the struct
    does not have are a TypeError that names the `family`."""
    p = struct()
    getattr(load(), default_fn)(C.byref(p))
    fields = info_fields(struct)
    for k, v in kw.items():
        if k not in fields:
            raise TypeError(f"unknown {family} parameter {k!r}")
        if isinstance(getattr(p, k), C.Array):
            getattr(p, k)[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


_lib = None


def declared_symbols():
    """Every function name include/gm_hip.h declares (used by the ABI test)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", text)))


def _preload_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own
    libamdhip64.so (same SONAME as /opt/rocm's).  If libgm_hip.so pulled in the
    system copy first, a later `import torch` would load a SECOND runtime and see
    no GPU.  So when torch is installed, its copy is loaded first and libgm_hip
    binds to it by SONAME; a C++ host without torch simply uses /opt/rocm's."""
    if os.environ.get("GM_HIP_SYSTEM_RUNTIME") == "1":
        return None
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return None
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    # the same for RCCL (gm_group_*): torch's bundled librccl.so shares no SONAME with /opt/rocm's, so a process could
    # map both; libgm_hip.so dlopens the one named here (csrc/gm_group.hip)
    rccl = os.path.join(libdir, "librccl.so")
    if os.path.exists(rccl):
        os.environ.setdefault("GM_RCCL_PATH", rccl)
    path = os.path.join(libdir, "libamdhip64.so")
    if not os.path.exists(path):
        return None
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def load():
    """dlopen libgm_hip.so and attach prototypes.  Raises if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C geometric_mapping_amd/csrc).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    u32p, u64p, fp, dp, i32p, u8p = map(P, (C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_int32, C.c_uint8))
    cfgp, cloudp, resp, fitp = map(P, (Config, Cloud, FrameResult, CylinderFit))
    sprmp, scellp, sinfop = map(P, (SurfaceParams, SurfaceCell, SurfaceInfo))
    wprmp, wrawp, waddp, winfop = map(P, (WallParams, WallRawCell, WallAddInfo, WallInfo))
    warcp, warcaddp, wclp, wcladdp = map(P, (WallArc, WallArcAddInfo, WallClothoid, WallClothoidAddInfo))
    welp, wpcp, waladdp, waltotp = map(P, (WallElement, WallAlignmentPiece, WallAlignmentAddInfo, WallAlignmentTotals))
    wregp, wrprmp, wrinfop, wrmetp = map(P, (WallRegion, WallRegionParams, WallRegionsInfo, WallRegionMetrics))
    wcprmp, wcptp, wcinfop = map(P, (WallCloudParams, WallCloudPoint, WallCloudInfo))
    wmprmp, wmtrip, wminfop = map(P, (WallMeshParams, WallMeshTriangle, WallMeshInfo))
    wgprmp, wgstp, wgcellp, wginfop, wgrunp = map(P, (WallClearanceParams, WallClearanceStation, WallClearanceCell,
                                                      WallClearanceInfo, WallClearanceRun))
    wsprmp, wssump, wssecp, wsinfop, wsmetp = map(P, (WallSectionParams, WallSectionSums, WallSection, WallSectionsInfo,
                                                      WallSectionMetrics))
    wqprmp, wqrecp, wqinfop, wqcolp, wqmetp, wqrunp = map(P, (WallQuantityParams, WallQuantity, WallQuantitiesInfo,
                                                              WallQuantityColumnResult, WallQuantityMetrics, WallQuantityRun))
    wkprmp, wkptp, wkinfop = map(P, (WallCheckParams, WallCheckPoint, WallCheckInfo))
    wcaprmp, wcainfop, wlprmp, wlinfop = map(P, (WallAddCheckedParams, WallAddCheckedInfo, WallLocateParams, WallLocateInfo))
    waprmp, wascp, wainfop = map(P, (WallAlignParams, WallAlignScore, WallAlignInfo))
    woprmp, wobjp, woinfop, wometp = map(P, (WallObjectParams, WallObject, WallObjectsInfo, WallObjectMetrics))
    waloinfop, walometp = P(WallAlignmentObjectsInfo), P(WallAlignmentObjectMetrics)
    walrinfop, walrmetp = P(WallAlignmentRegionsInfo), P(WallAlignmentRegionMetrics)
    proto = {
        "gm_create": (C.c_int, [cfgp, C.POINTER(vp)]),
        "gm_destroy": (None, [vp]),
        "gm_default_config": (None, [cfgp]),
        "gm_host_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        "gm_host_free": (C.c_int, [vp, vp]),
        "gm_host_register": (C.c_int, [vp, vp, C.c_size_t]),
        "gm_host_unregister": (C.c_int, [vp, vp]),
        "gm_abi_version": (u32, []),
        "gm_debug_live_buffers": (C.c_longlong, []),
        "gm_status_string": (C.c_char_p, [C.c_int]),
        "gm_last_error": (C.c_char_p, [vp]),
        "gm_process_frame": (C.c_int, [vp, cloudp, resp]),
        "gm_submit_frame": (C.c_int, [vp, u32, cloudp]),
        "gm_wait_frame": (C.c_int, [vp, u32, resp]),
        "gm_poll_frame": (C.c_int, [vp, u32]),
        "gm_set_cloud_output": (C.c_int, [vp, u32, fp, u32]),
        "gm_get_cropped_xyz": (C.c_int, [vp, u32, fp, u32, u32p]),
        "gm_get_normals": (C.c_int, [vp, u32, fp, u32, u32p]),
        "gm_get_voxel_centroids": (C.c_int, [vp, u32, fp, u32, u32p]),
        "gm_get_voxel_nearest": (C.c_int, [vp, u32, i32p, u32, u32p]),
        "gm_get_voxel_normals": (C.c_int, [vp, u32, fp, u32, u32p]),
        "gm_get_neighbor_counts": (C.c_int, [vp, u32, i32p, u32, u32p]),
        "gm_get_labels": (C.c_int, [vp, u32, u8p, u32, u32p]),
        "gm_chop_cloud": (C.c_int, [vp, cloudp, C.c_double, fp, u32, u32p]),
        "gm_get_normals_stage": (C.c_int, [vp, fp, u32, C.c_double, fp, fp, u32, u32p]),
        "gm_get_local_frame": (C.c_int, [vp, fp, u32, C.c_double, fp, fp, dp]),
        "gm_compact_valid_stage": (C.c_int, [vp, fp, fp, u32, C.c_double, fp, fp, u32, u32p, dp]),
        "gm_voxel_grid": (C.c_int, [vp, fp, u32, C.c_double, fp, u32, u32p, u32p]),
        "gm_nearest": (C.c_int, [vp, fp, u32, fp, u32, i32p]),
        "gm_solve_local_frame": (C.c_int, [dp, fp, fp]),
        "gm_set_owned_range": (C.c_int, [vp, C.c_double, C.c_double]),
        "gm_ext_available": (C.c_int, []),
        "gm_score_frame": (C.c_int, [vp, u32, C.c_int, fp, u32, C.c_double, u32, i32p]),
        "gm_score_planes": (C.c_int, [vp, fp, u32, u8p, u32, fp, u32, C.c_double, i32p]),
        "gm_score_cylinders": (C.c_int, [vp, fp, u32, u8p, u32, fp, u32, C.c_double, i32p]),
        "gm_plane_hypotheses": (C.c_int, [vp, fp, u32, u8p, u32, C.c_uint64, u32, fp]),
        "gm_cylinder_hypotheses": (C.c_int, [vp, fp, fp, u32, u8p, u32, C.c_uint64, u32, fp]),
        "gm_segment_moments": (C.c_int, [vp, fp, fp, u8p, u32, u32, dp]),
        "gm_get_compressed_map": (C.c_int, [vp, u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "gm_get_cylinder_fit": (C.c_int, [vp, u32, fitp]),
        "gm_fit_cylinder": (C.c_int, [vp, fp, u32, u8p, u32, fp, C.c_double, fitp, u8p]),
        "gm_surface_default_params": (None, [sprmp]),
        "gm_set_surface_params": (C.c_int, [vp, sprmp]),
        "gm_get_surface_map": (C.c_int, [vp, u32, sinfop, scellp, u32, u32p]),
        "gm_get_surface_points": (C.c_int, [vp, u32, fp, i32p, u32, u32p]),
        "gm_surface_map": (C.c_int, [vp, fp, u32, u8p, fp, sprmp, sinfop, scellp, u32, fp, i32p]),
        "gm_wall_default_params": (None, [wprmp]),
        "gm_wall_map_create": (C.c_int, [vp, wprmp, C.POINTER(vp)]),
        "gm_wall_map_destroy": (None, [vp]),
        "gm_wall_map_create_arc": (C.c_int, [vp, wprmp, warcp, C.POINTER(vp)]),
        "gm_wall_map_get_arc": (C.c_int, [vp, warcp]),
        "gm_wall_arc_check_params": (C.c_int, [wprmp, warcp]),
        "gm_wall_arc_add_frame": (C.c_int, [wprmp, warcp, dp, warcaddp]),
        "gm_wall_arc_frame": (C.c_int, [wprmp, warcp, C.c_double, dp, dp, dp, dp]),
        "gm_wall_arc_project": (C.c_int, [wprmp, warcp, dp, dp, dp, dp]),
        "gm_wall_arc_point": (C.c_int, [wprmp, warcp, C.c_double, C.c_double, C.c_double, dp]),
        "gm_wall_map_create_clothoid": (C.c_int, [vp, wprmp, wclp, C.POINTER(vp)]),
        "gm_wall_map_get_clothoid": (C.c_int, [vp, wclp]),
        "gm_wall_clothoid_check_params": (C.c_int, [wprmp, wclp]),
        "gm_wall_clothoid_add_frame": (C.c_int, [wprmp, wclp, dp, wcladdp]),
        "gm_wall_clothoid_frame": (C.c_int, [wprmp, wclp, C.c_double, dp, dp, dp, dp, dp, dp]),
        "gm_wall_clothoid_project": (C.c_int, [wprmp, wclp, dp, dp, dp, dp]),
        "gm_wall_clothoid_point": (C.c_int, [wprmp, wclp, C.c_double, C.c_double, C.c_double, dp]),
        "gm_wall_alignment_check": (C.c_int, [wprmp, welp, u32]),
        "gm_wall_alignment_element_params": (C.c_int, [wprmp, welp, u32, u32, wprmp, warcp, wclp]),
        "gm_wall_alignment_project": (C.c_int, [wprmp, welp, u32, dp, u32p, dp, dp, dp]),
        "gm_wall_alignment_point": (C.c_int, [wprmp, welp, u32, C.c_double, C.c_double, C.c_double, dp]),
        "gm_wall_alignment_add_plan": (C.c_int, [wprmp, welp, u32, dp, C.c_double, waladdp]),
        "gm_wall_alignment_window": (C.c_int, [wprmp, welp, u32, C.c_double, C.c_double, wpcp, u32, u32p]),
        "gm_wall_alignment_create": (C.c_int, [vp, wprmp, welp, u32, C.POINTER(vp)]),
        "gm_wall_alignment_destroy": (None, [vp]),
        "gm_wall_alignment_map": (C.c_int, [vp, u32, C.POINTER(vp)]),
        "gm_wall_alignment_add_frame": (C.c_int, [vp, vp, u32, dp, waladdp]),
        "gm_wall_alignment_add_points": (C.c_int, [vp, fp, u32, u8p, dp, waladdp, fp, i32p, i32p]),
        "gm_wall_alignment_sync": (C.c_int, [vp]),
        "gm_wall_alignment_locate_plan": (C.c_int, [wprmp, welp, u32, dp, C.c_double, C.POINTER(WallAlignmentLocateStart)]),
        "gm_wall_alignment_locate_frame": (C.c_int, [vp, vp, u32, dp, wlprmp]),
        "gm_wall_alignment_get_locate": (C.c_int, [vp, u32, C.POINTER(WallAlignmentLocateInfo)]),
        "gm_wall_alignment_locate_points": (C.c_int, [vp, fp, u32, u8p, dp, wlprmp, C.POINTER(WallAlignmentLocateInfo), fp, i32p, i32p]),
        "gm_wall_alignment_align_plan": (C.c_int, [wprmp, welp, u32, dp, C.c_double, waprmp, C.POINTER(WallAlignmentAlignPlan)]),
        "gm_wall_alignment_align_select": (C.c_int, [wprmp, welp, u32, dp, C.c_double, waprmp, wascp, u32,
                                                     C.POINTER(WallAlignmentAlignInfo)]),
        "gm_wall_alignment_align_frame": (C.c_int, [vp, vp, u32, dp, waprmp, C.POINTER(WallAlignmentAlignPlan)]),
        "gm_wall_alignment_get_align": (C.c_int, [vp, u32, C.POINTER(WallAlignmentAlignInfo), wascp, u32, u32p]),
        "gm_wall_alignment_align_points": (C.c_int, [vp, fp, u32, u8p, dp, waprmp, C.POINTER(WallAlignmentAlignPlan),
                                                     C.POINTER(WallAlignmentAlignInfo), wascp, u32, u32p, fp, i32p, i32p]),
        "gm_wall_alignment_check_frame": (C.c_int, [vp, vp, u32, dp, wkprmp, waladdp]),
        "gm_wall_alignment_get_check": (C.c_int, [vp, u32, C.POINTER(WallAlignmentCheckInfo), wkptp, u32, u32p]),
        "gm_wall_alignment_check_points": (C.c_int, [vp, fp, u32, u8p, dp, wkprmp, waladdp, C.POINTER(WallAlignmentCheckInfo), wkptp,
                                                     u32, u32p, fp, i32p, i32p, u8p, i32p]),
        "gm_wall_alignment_add_frame_checked": (C.c_int, [vp, vp, u32, dp, wcaprmp, waladdp]),
        "gm_wall_alignment_get_add_checked": (C.c_int, [vp, u32, wcainfop]),
        "gm_wall_alignment_add_points_checked": (C.c_int, [vp, fp, u32, u8p, dp, wcaprmp, wkptp, u32, waladdp, wcainfop, fp, i32p,
                                                           i32p]),
        "gm_wall_alignment_check_objects": (C.c_int, [vp, u32, woprmp, waloinfop, wobjp, u32, u32p, i32p, u32]),
        "gm_wall_alignment_check_objects_rows": (C.c_int, [vp, wkptp, u32, waladdp, woprmp, waloinfop, wobjp, u32, u32p, i32p]),
        "gm_wall_alignment_object_window": (C.c_int, [wprmp, welp, u32, waladdp, woprmp, waloinfop]),
        "gm_wall_alignment_object_metrics": (C.c_int, [wprmp, welp, u32, woprmp, wobjp, walometp]),
        "gm_wall_alignment_regions": (C.c_int, [vp, vp, u32, u32, wrprmp, walrinfop, wregp, u32, u32p, i32p]),
        "gm_wall_alignment_region_window": (C.c_int, [wprmp, welp, u32, u32, u32, walrinfop]),
        "gm_wall_alignment_region_metrics": (C.c_int, [wprmp, welp, u32, wregp, walrmetp]),
        "gm_wall_alignment_info": (C.c_int, [vp, waltotp]),
        "gm_wall_map_add_frame": (C.c_int, [vp, vp, u32, dp, waddp]),
        "gm_wall_map_add_points": (C.c_int, [vp, fp, u32, u8p, dp, waddp, fp, i32p]),
        "gm_wall_map_sync": (C.c_int, [vp]),
        "gm_wall_map_info": (C.c_int, [vp, winfop]),
        "gm_wall_map_read": (C.c_int, [vp, u32, u32, scellp, u64, u64p]),
        "gm_wall_map_read_raw": (C.c_int, [vp, u32, u32, wrawp, u64, u64p]),
        "gm_wall_map_add_raw": (C.c_int, [vp, u32, u32, wrawp]),
        "gm_wall_map_clear": (C.c_int, [vp, u32, u32]),
        "gm_wall_region_default_params": (None, [wrprmp]),
        "gm_wall_map_regions": (C.c_int, [vp, vp, u32, u32, wrprmp, wrinfop, wregp, u32, u32p, i32p]),
        "gm_wall_region_metrics": (C.c_int, [wprmp, wregp, wrmetp]),
        "gm_wall_cloud_default_params": (None, [wcprmp]),
        "gm_wall_cloud_directions": (C.c_int, [wprmp, wcprmp, dp, u32, u32p]),
        "gm_wall_map_cloud": (C.c_int, [vp, u32, u32, wcprmp, wcinfop, wcptp, u64, u64p]),
        "gm_wall_mesh_default_params": (None, [wmprmp]),
        "gm_wall_map_mesh": (C.c_int, [vp, u32, u32, wmprmp, wminfop, wcptp, u64, wmtrip, u64, u64p, u64p]),
        "gm_wall_mesh_triangulate": (C.c_int, [u32, u32, wcptp, u64, u32, C.c_double, wminfop, wmtrip, u64, u64p]),
        "gm_wall_mesh_write_ply": (C.c_int, [C.c_char_p, wcptp, u64, wmtrip, u64]),
        "gm_wall_clearance_default_params": (None, [wgprmp]),
        "gm_wall_clearance_check_params": (C.c_int, [wprmp, wgprmp, i32p, u32, u8p, u32]),
        "gm_wall_map_clearance": (C.c_int, [vp, u32, u32, i32p, u32, u8p, wgprmp, wginfop, wgstp, u32, wgcellp, u64, u64p]),
        "gm_wall_gauge_from_polygon": (C.c_int, [wprmp, dp, u32, dp, i32p, u32, u32p]),
        "gm_wall_clearance_runs": (C.c_int, [wprmp, wgstp, u32, u32, u32, wgrunp, u32, u32p]),
        "gm_wall_section_default_params": (None, [wsprmp]),
        "gm_wall_section_check_params": (C.c_int, [wsprmp]),
        "gm_wall_section_basis": (C.c_int, [u32, u32, i32p, u32, u32p]),
        "gm_wall_section_solve": (C.c_int, [wssump, u32, u32, C.POINTER(C.c_int64), u32p]),
        "gm_wall_section_metrics": (C.c_int, [wprmp, wssecp, u32, wsmetp]),
        "gm_wall_map_sections": (C.c_int, [vp, vp, u32, u32, wsprmp, wsinfop, wssecp, u32, u32p, wssump]),
        "gm_wall_quantity_default_params": (None, [wqprmp]),
        "gm_wall_quantity_check_params": (C.c_int, [wprmp, wqprmp, i32p, i32p, u32, u8p, u32, u8p, u32]),
        "gm_wall_quantity_column": (C.c_int, [C.c_int64, u64, C.c_int64, C.c_int, u64, C.c_int64, u32, C.c_int32, C.c_int32, u32,
                                              wqcolp]),
        "gm_wall_quantity_metrics": (C.c_int, [wprmp, wqrecp, wqmetp]),
        "gm_wall_quantity_runs": (C.c_int, [wprmp, wqrecp, u32, u32, u32, u32, wqrunp, u32, u32p]),
        "gm_wall_map_quantities": (C.c_int, [vp, vp, u32, u32, i32p, i32p, u32, u8p, u8p, u32, wqprmp, wqinfop, wqrecp, u32, u32p,
                                             i32p]),
        "gm_wall_check_default_params": (None, [wkprmp]),
        "gm_wall_check_classify": (C.c_int, [wkprmp, wrawp, C.c_float, C.POINTER(C.c_int64), u32p]),
        "gm_wall_map_check_frame": (C.c_int, [vp, vp, u32, dp, wkprmp, waddp]),
        "gm_wall_map_get_check": (C.c_int, [vp, u32, wkinfop, wkptp, u32, u32p]),
        "gm_wall_map_check_points": (C.c_int, [vp, fp, u32, u8p, dp, wkprmp, waddp, wkinfop, wkptp, u32, u32p, fp, i32p, i32p, u8p]),
        "gm_wall_add_checked_default_params": (None, [wcaprmp]),
        "gm_wall_add_checked_check_params": (C.c_int, [wcaprmp]),
        "gm_wall_map_add_frame_checked": (C.c_int, [vp, vp, u32, dp, wcaprmp, waddp]),
        "gm_wall_map_get_add_checked": (C.c_int, [vp, u32, wcainfop]),
        "gm_wall_map_add_points_checked": (C.c_int, [vp, fp, u32, u8p, dp, wcaprmp, wkptp, u32, waddp, wcainfop, fp, i32p]),
        "gm_wall_locate_default_params": (None, [wlprmp]),
        "gm_wall_locate_check_params": (C.c_int, [wlprmp]),
        "gm_wall_map_locate_frame": (C.c_int, [vp, vp, u32, dp, wlprmp]),
        "gm_wall_map_get_locate": (C.c_int, [vp, u32, wlinfop]),
        "gm_wall_map_locate_points": (C.c_int, [vp, fp, u32, u8p, dp, wlprmp, wlinfop, fp, i32p]),
        "gm_wall_align_default_params": (None, [waprmp]),
        "gm_wall_align_check_params": (C.c_int, [waprmp, u32]),
        "gm_wall_align_select": (C.c_int, [C.POINTER(WallParams), waprmp, dp, wascp, u32, wainfop]),
        "gm_wall_map_align_frame": (C.c_int, [vp, vp, u32, dp, waprmp, waddp]),
        "gm_wall_map_get_align": (C.c_int, [vp, u32, wainfop, wascp, u32, u32p]),
        "gm_wall_map_align_points": (C.c_int, [vp, fp, u32, u8p, dp, waprmp, waddp, wainfop, wascp, u32, u32p, fp, i32p]),
        "gm_wall_object_default_params": (None, [woprmp]),
        "gm_wall_map_check_objects": (C.c_int, [vp, u32, woprmp, woinfop, wobjp, u32, u32p, i32p, u32]),
        "gm_wall_check_objects": (C.c_int, [vp, wkptp, u32, C.c_int64, woprmp, woinfop, wobjp, u32, u32p, i32p]),
        "gm_wall_object_metrics": (C.c_int, [wprmp, woprmp, wobjp, wometp]),
        "gm_group_create": (C.c_int, [cfgp, i32p, u32, u32, C.POINTER(vp)]),
        "gm_group_destroy": (None, [vp]),
        "gm_group_size": (u32, [vp]),
        "gm_group_ctx": (vp, [vp, u32]),
        "gm_group_last_error": (C.c_char_p, [vp]),
        "gm_group_process_frame": (C.c_int, [vp, cloudp, resp]),
        "gm_group_get_cropped_xyz": (C.c_int, [vp, fp, u32, u32p]),
        "gm_group_get_voxel_centroids": (C.c_int, [vp, fp, u32, u32p]),
        "gm_group_get_voxel_normals": (C.c_int, [vp, fp, u32, u32p]),
        "gm_group_get_voxel_nearest": (C.c_int, [vp, i32p, u32, u32p]),
        "gm_group_get_timing": (C.c_int, [vp, dp, u32]),
        "gm_group_get_edges": (C.c_int, [vp, dp, u32, u32p]),
        "gm_group_submit_frame": (C.c_int, [vp, cloudp]),
        "gm_group_wait_frame": (C.c_int, [vp, resp, u32p, u32p]),
        "gm_group_poll_frame": (C.c_int, [vp]),
        "gm_group_in_flight": (u32, [vp]),
        "gm_group_fit_cylinder": (C.c_int, [vp, fp, fitp]),
        "gm_group_get_cylinder_fit": (C.c_int, [vp, fitp]),
        "gm_group_get_labels": (C.c_int, [vp, u8p, u32, u32p]),
    }
    for name, (res, args) in proto.items():
        fn = getattr(L, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    L._gm_proto = proto
    _lib = L
    return L
