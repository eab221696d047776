"""Host-side mirror of the reference's processing interface, over the C ABI.

The reference's path is four C++ free functions
(/root/reference include/geometric_mapping/tunnel_processing.hpp:38-54,77-82)
driven by cloud_cb (/root/reference src/geometric_mapping.cpp:48-125).  This
module keeps their names, argument order and meaning so the parity tests read
like the reference's call sites; every method is a thin ctypes call into
libgm_hip.so (include/gm_hip.h) -- no arithmetic happens in Python.

Clouds are numpy float32 arrays [n,3]; normals are [n,4] = (nx,ny,nz,curvature).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (GM_CFG_CYLINDER_FIT, GM_CFG_DEFAULT, GM_CFG_KEEP_COUNTS, GM_CFG_STAGE_TIMING, GM_CFG_VOXEL_GRID,
                   GM_CLOUD_BIGENDIAN, GM_CLOUD_DEVICE, GM_CLOUD_PINNED, GM_ERR_CAPACITY, GM_ERR_NOT_READY, GM_OK, Cloud, Config,
                   CylinderFit, FrameResult, GmError, STAGE_NAMES)

__all__ = ["GeometricMapping", "GeometricMappingGroup", "WallMap", "GmError", "solve_local_frame", "decode_compressed_map",
           "GM_CFG_CYLINDER_FIT"]


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _rptr(a, struct):
    """The records of a numpy array as a pointer to their struct."""
    return a.ctypes.data_as(C.POINTER(struct))


def _ints(info, fields):
    return {k: int(getattr(info, k)) for k in fields}


def _stage_front(cloud, pose, labels):
    """The opening arguments of a stage call on a host cloud: (n, (xyz pointer, n, label pointer or None, pose pointer)),
    the pose pointer left out when `pose` is None.  The arrays live as long as the pointers: ndarray.ctypes.data_as
    keeps a reference to its array in the pointer it returns (numpy documents that), so nothing else need hold them."""
    xyz = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    tail = () if pose is None else (_dptr(WallMap._pose(pose)),)
    lab, lp = GeometricMapping._u8(labels)
    return len(xyz), (_f32(xyz), len(xyz), lp) + tail


class _PointOutputs:
    """The per-point outputs of one stage call, from an ordered (name, dtype) list: a buffer of max(n, 1) entries each
    when `outputs` is set, none otherwise (the ABI takes NULL for an output that is not wanted)."""

    def __init__(self, n, outputs, fields):
        self.n, self.fields = n, fields
        self.buf = {k: np.empty(max(n, 1), dtype=t) for k, t in fields} if outputs else None

    def ptrs(self):
        """One pointer, or None, per output in order."""
        if self.buf is None:
            return (None,) * len(self.fields)
        return tuple(b.ctypes.data_as(_OUT_PTR[b.dtype]) for b in self.buf.values())

    def tuple(self):
        """The outputs trimmed to n, copied, in order; None each without outputs."""
        if self.buf is None:
            return (None,) * len(self.fields)
        return tuple(b[:self.n].copy() for b in self.buf.values())

    def dict(self):
        """The same by name; None without outputs."""
        return {k: b[:self.n].copy() for k, b in self.buf.items()} if self.buf is not None else None


_OUT_PTR = {np.dtype(t): C.POINTER(c) for t, c in ((np.float32, C.c_float), (np.int32, C.c_int32), (np.uint8, C.c_uint8))}
_RES_CELL = (("res", np.float32), ("cell", np.int32))
_CHECK_OUT = (("e", np.float32), ("cell", np.int32), ("delta", np.int32), ("cls", np.uint8))
_ALIGN_OUT = (("e", np.float32), ("cell", np.int32))
_ELEMENT = (("element", np.int32),)


def _sized(call, struct, got, fetch):
    """A count query, then the sized call: call(records, capacity, sized) is the bound and checked ABI call, which leaves
    the count in `got` -- (None, 0, False) in the query, (the buffer, the count, True) in the sized call, so a caller whose
    other outputs travel with the sized call only picks them by `sized`; fetch(capacity) is the caller's rule for making
    the sized call at all.  Returns the records of `struct`, as many as `got` says."""
    call(None, 0, False)
    cap = int(got.value)
    rec = np.zeros(max(cap, 1), dtype=struct)
    if fetch(cap):
        call(_rptr(rec, struct), cap, True)
    return rec[:int(got.value)].copy()


class GeometricMapping:
    """One gm_ctx.  Parameter names and defaults are the node's
    (/root/reference launch/mapping.launch:7-10, paramHandler.hpp:26-29)."""

    def __init__(self, boxFilterBound=5.0, voxelGridLeafSize=0.5, neighborRadius=0.5, weightingFactor=0.2,
                 device=0, flags=GM_CFG_DEFAULT, n_slots=1, max_points=0,
                 ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=1):
        self._L = _lib.load()
        cfg = Config()
        self._L.gm_default_config(C.byref(cfg))
        cfg.flags = flags
        cfg.boxFilterBound = boxFilterBound
        cfg.voxelGridLeafSize = voxelGridLeafSize
        cfg.neighborRadius = neighborRadius
        cfg.weightingFactor = weightingFactor
        cfg.device = device
        cfg.n_slots = n_slots
        cfg.max_points = max_points
        cfg.ransac_hypotheses = ransac_hypotheses
        cfg.ransac_threshold = ransac_threshold
        cfg.ransac_seed = ransac_seed
        self.cfg = cfg
        self._ctx = C.c_void_p()
        self._pinned = []
        st = self._L.gm_create(C.byref(cfg), C.byref(self._ctx))
        if st != GM_OK:
            msg = self._L.gm_last_error(None).decode()
            self._ctx = None
            raise GmError(st, msg)
        self._keep = {}  # slot -> arrays that must outlive an async submit

    # ---- lifetime ----
    def close(self):
        if getattr(self, "_ctx", None):
            for slot in getattr(self, "_cloud_slots", []):   # (waits for a frame that still writes the buffer)
                self._L.gm_set_cloud_output(self._ctx, slot, None, 0)
            self._cloud_slots = []
            for a in getattr(self, "_registered", []):
                self._L.gm_host_unregister(self._ctx, a.ctypes.data)
            self._registered = []
            for p in getattr(self, "_pinned", []):
                self._L.gm_host_free(self._ctx, p)
            self._pinned = []
            for m in list(getattr(self, "_walls", [])):   # (gm_destroy frees the maps: their handles die here)
                m._map = None
            self._walls = []
            self._L.gm_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != GM_OK:
            raise GmError(st, self._L.gm_last_error(self._ctx).decode())

    # ---- cloud descriptors ----
    @staticmethod
    def _cloud_from_xyz(xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("cloud must be [n,3] or [n,4] float32")
        step = 4 * xyz.shape[1]
        c = Cloud(xyz.ctypes.data, xyz.shape[0], step, 0, 4, 8, 0)
        return c, xyz

    @staticmethod
    def cloud_from_rows(data, n_points, point_step, offsets=(0, 4, 8), bigendian=False):
        """PointCloud2-style rows held in a numpy uint8 buffer."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size < n_points * point_step:
            raise ValueError("row buffer smaller than n_points*point_step")
        c = Cloud(data.ctypes.data, n_points, point_step, offsets[0], offsets[1], offsets[2],
                  GM_CLOUD_BIGENDIAN if bigendian else 0)
        return c, data

    @staticmethod
    def cloud_from_device(ptr, n_points, point_step=16, offsets=(0, 4, 8)):
        """Rows already resident in this device's HBM (e.g. a torch tensor's data_ptr())."""
        return Cloud(int(ptr), n_points, point_step, offsets[0], offsets[1], offsets[2], GM_CLOUD_DEVICE), None

    def pinned_rows(self, n_points, point_step=12):
        """A page-locked row buffer (numpy uint8 view of gm_host_alloc memory) and a function that wraps it as a
        GM_CLOUD_PINNED cloud: frames submitted from it skip the staging copy.  Freed with the context."""
        ptr = C.c_void_p()
        nbytes = int(n_points) * int(point_step)
        self._check(self._L.gm_host_alloc(self._ctx, nbytes, C.byref(ptr)))
        self._pinned.append(ptr)
        buf = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]

        def as_cloud(n=n_points, offsets=(0, 4, 8), bigendian=False):
            return Cloud(ptr.value, int(n), int(point_step), offsets[0], offsets[1], offsets[2],
                         GM_CLOUD_PINNED | (GM_CLOUD_BIGENDIAN if bigendian else 0)), buf
        return buf, as_cloud

    def _as_cloud(self, cloud):
        if isinstance(cloud, tuple) and isinstance(cloud[0], Cloud):
            return cloud
        return self._cloud_from_xyz(cloud)

    @staticmethod
    def _result(res):
        ev = np.array(res.eigenvalues[:], dtype=np.float32)
        V = np.array(res.eigenvectors[:], dtype=np.float32).reshape(3, 3).T.copy()  # column-major -> [row, col]
        sc = np.array(res.scatter[:], dtype=np.float64)
        M = np.array([[sc[0], sc[1], sc[2]], [sc[1], sc[3], sc[4]], [sc[2], sc[4], sc[5]]])
        return dict(n_in=res.n_in, n_cropped=res.n_cropped, n_valid=res.n_valid, n_voxels=res.n_voxels,
                    eigenvalues=ev, eigenvectors=V, center_axis=np.array(res.center_axis[:], dtype=np.float32),
                    scatter=M, scatter6=sc, status_flags=res.status_flags,
                    stage_ms={k: float(res.stage_ms[i]) for i, k in enumerate(STAGE_NAMES)},
                    normals_kernel_ms=float(res.normals_kernel_ms),
                    plane=np.array(res.plane[:], dtype=np.float32), cylinder=np.array(res.cylinder[:], dtype=np.float32),
                    plane_inliers=res.plane_inliers, cylinder_inliers=res.cylinder_inliers,
                    plane_refit=np.array(res.plane_refit[:]), cylinder_axis_refit=np.array(res.cylinder_axis_refit[:]))

    # ---- the callback: src/geometric_mapping.cpp:55-92 ----
    def process_frame(self, cloud):
        c, keep = self._as_cloud(cloud)
        res = FrameResult()
        self._check(self._L.gm_process_frame(self._ctx, C.byref(c), C.byref(res)))
        return self._result(res)

    def submit_frame(self, slot, cloud):
        c, keep = self._as_cloud(cloud)
        self._check(self._L.gm_submit_frame(self._ctx, slot, C.byref(c)))

    def wait_frame(self, slot):
        res = FrameResult()
        self._check(self._L.gm_wait_frame(self._ctx, slot, C.byref(res)))
        return self._result(res)

    def poll_frame(self, slot):
        """True when the slot's submitted frame has finished (wait_frame returns at once); never blocks."""
        st = self._L.gm_poll_frame(self._ctx, slot)
        if st == GM_OK:
            return True
        if st == GM_ERR_NOT_READY:
            return False
        self._check(st)

    def cloud_output_into(self, slot, array):
        """The same into memory the caller owns: a C-contiguous float32 [capacity, 4] numpy array (e.g. the buffer a message
        is published from) is page-locked (gm_host_register) and registered as the slot's /choppedCloud output.  The array
        must outlive the context (or a cloud_output_into(slot, None))."""
        if array is None:
            self._check(self._L.gm_set_cloud_output(self._ctx, slot, None, 0))
            return None
        assert array.dtype == np.float32 and array.ndim == 2 and array.shape[1] == 4 and array.flags["C_CONTIGUOUS"]
        self._check(self._L.gm_host_register(self._ctx, array.ctypes.data, array.nbytes))
        self._registered = getattr(self, "_registered", []) + [array]
        self._check(self._L.gm_set_cloud_output(self._ctx, slot, array.ctypes.data_as(C.POINTER(C.c_float)), array.shape[0]))
        self._cloud_slots = getattr(self, "_cloud_slots", []) + [slot]
        return array

    def cloud_output(self, slot, capacity):
        """Registers a page-locked /choppedCloud buffer for the slot (gm_set_cloud_output): every later frame of the slot
        copies its valid cloud there while the rest of the frame runs.  Returns the float32 [capacity, 4] view
        (x, y, z, bits(input row)); rows [0, n_valid) are the frame's once wait_frame has returned."""
        ptr = C.c_void_p()
        self._check(self._L.gm_host_alloc(self._ctx, int(capacity) * 16, C.byref(ptr)))
        self._pinned.append(ptr)
        self._check(self._L.gm_set_cloud_output(self._ctx, slot, C.cast(ptr, C.POINTER(C.c_float)), int(capacity)))
        self._cloud_slots = getattr(self, "_cloud_slots", []) + [slot]
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(max(int(capacity), 1), 4))[:int(capacity)]

    def _fetch(self, fn, slot, width, dtype=np.float32):
        n = C.c_uint32(0)
        st = fn(self._ctx, slot, None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            self._check(st)
        out = np.empty((n.value, width) if width > 1 else (n.value,), dtype=dtype)
        if n.value:
            ptr = out.ctypes.data_as(fn.argtypes[2])
            self._check(fn(self._ctx, slot, ptr, n.value, C.byref(n)))
        return out

    def cropped_cloud(self, slot=0):
        """/choppedCloud: (xyz [n,3], input row index [n])."""
        a = self._fetch(self._L.gm_get_cropped_xyz, slot, 4)
        return a[:, :3].copy(), a[:, 3].copy().view(np.int32)

    def normals(self, slot=0):
        return self._fetch(self._L.gm_get_normals, slot, 4)

    def voxel_centroids(self, slot=0):
        """(centroids [V,3], points per voxel [V]) in ascending voxel-key order."""
        a = self._fetch(self._L.gm_get_voxel_centroids, slot, 4)
        return a[:, :3].copy(), a[:, 3].astype(np.int32)

    def neighbor_counts(self, slot=0):
        return self._fetch(self._L.gm_get_neighbor_counts, slot, 1, np.int32)

    def voxel_nearest(self, slot=0):
        """Index (into cropped_cloud()) of the nearest point of every voxel centroid (GM_CFG_NEAREST)."""
        return self._fetch(self._L.gm_get_voxel_nearest, slot, 1, np.int32)

    def voxel_normals(self, slot=0):
        """normals->at(kIndices[0]) per voxel centroid (tunnel_processing.cpp:247-249): [V,4], needs GM_CFG_NEAREST."""
        return self._fetch(self._L.gm_get_voxel_normals, slot, 4)

    def labels(self, slot=0):
        """Extension: segment label per valid point (0 none, 1 plane, 2 cylinder)."""
        return self._fetch(self._L.gm_get_labels, slot, 1, np.uint8)

    def compressed_map(self, slot=0):
        """Extension: raw bytes of the build-defined map record (see decode_compressed_map)."""
        n = C.c_size_t(0)
        st = self._L.gm_get_compressed_map(self._ctx, slot, None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            self._check(st)
        buf = np.zeros(n.value, dtype=np.uint8)
        self._check(self._L.gm_get_compressed_map(self._ctx, slot, buf.ctypes.data, n.value, C.byref(n)))
        return buf

    def set_owned_range(self, lo, hi):
        self._check(self._L.gm_set_owned_range(self._ctx, float(lo), float(hi)))

    # ---- the reference's stage functions (tunnel_processing.hpp) ----
    def chopCloud(self, bound, cloud):
        """tunnel_processing.hpp:38.  Returns (cloudChopped [n',3], kept input rows [n'])."""
        c, keep = self._as_cloud(cloud)
        cap = max(c.n_points, 1)
        out = np.empty((cap, 4), dtype=np.float32)
        n = C.c_uint32(0)
        self._check(self._L.gm_chop_cloud(self._ctx, C.byref(c), float(bound), _f32(out), cap, C.byref(n)))
        out = out[:n.value]
        return out[:, :3].copy(), out[:, 3].copy().view(np.int32)

    def getNormals(self, neighborRadius, cloud):
        """tunnel_processing.hpp:41-45.  The reference compacts `cloud` in place and
        returns the normals; here both come back: (normals [n'',4], cloud [n'',3], kept rows [n''])."""
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("cloud must be [n,3]")
        n0 = xyz.shape[0]
        cap = max(n0, 1)
        oc = np.empty((cap, 4), dtype=np.float32)
        on = np.empty((cap, 4), dtype=np.float32)
        n = C.c_uint32(0)
        self._check(self._L.gm_get_normals_stage(self._ctx, _f32(xyz), n0, float(neighborRadius), _f32(oc), _f32(on),
                                                 cap, C.byref(n)))
        oc, on = oc[:n.value], on[:n.value]
        return on.copy(), oc[:, :3].copy(), oc[:, 3].copy().view(np.int32)

    def getLocalFrame(self, cloudSize, weightingFactor, cloud_normals):
        """tunnel_processing.hpp:48-54.  Returns (eigenVals [3] ascending, eigenVecs [3,3] columns, M [3,3] fp64)."""
        nrm = np.ascontiguousarray(cloud_normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] != 4:
            raise ValueError("normals must be [n,4] (nx,ny,nz,curvature)")
        if cloudSize > nrm.shape[0]:
            raise ValueError("cloudSize exceeds the normals cloud (the reference's .at() would throw)")
        ev = np.zeros(3, dtype=np.float32)
        V = np.zeros(9, dtype=np.float32)
        sc = np.zeros(6, dtype=np.float64)
        self._check(self._L.gm_get_local_frame(self._ctx, _f32(nrm), int(cloudSize), float(weightingFactor), _f32(ev),
                                               _f32(V), sc.ctypes.data_as(C.POINTER(C.c_double))))
        M = np.array([[sc[0], sc[1], sc[2]], [sc[1], sc[3], sc[4]], [sc[2], sc[4], sc[5]]])
        return ev, V.reshape(3, 3).T.copy(), M

    def compactValid(self, weightingFactor, rows, normals):
        """The NaN-normal removal of getNormals and getLocalFrame's scatter sums on caller-supplied rows: rows [n,4]
        (x,y,z,pad) and normals [n,4] (nx,ny,nz,curvature) in.  Returns (rows [n',4], normals [n',4], scatter6 [6] fp64):
        the rows whose normal has three finite components, in order, bit for bit."""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        nr = np.ascontiguousarray(normals, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != 4 or nr.shape != r.shape:
            raise ValueError("rows and normals must both be [n,4]")
        n0 = r.shape[0]
        cap = max(n0, 1)
        oc = np.empty((cap, 4), dtype=np.float32)
        on = np.empty((cap, 4), dtype=np.float32)
        n = C.c_uint32(0)
        sc = np.zeros(6, dtype=np.float64)
        self._check(self._L.gm_compact_valid_stage(self._ctx, _f32(r), _f32(nr), n0, float(weightingFactor), _f32(oc),
                                                   _f32(on), cap, C.byref(n), sc.ctypes.data_as(C.POINTER(C.c_double))))
        return oc[:n.value].copy(), on[:n.value].copy(), sc

    def voxelGrid(self, leafSize, cloud):
        """The pcl::VoxelGrid half of rvizNormals (tunnel_processing.hpp:77-82).
        Returns (centroids [V,3], counts [V], passthrough flag)."""
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("cloud must be [n,3]")
        cap = max(xyz.shape[0], 1)
        out = np.empty((cap, 4), dtype=np.float32)
        n = C.c_uint32(0)
        fl = C.c_uint32(0)
        self._check(self._L.gm_voxel_grid(self._ctx, _f32(xyz), xyz.shape[0], float(leafSize), _f32(out), cap,
                                          C.byref(n), C.byref(fl)))
        out = out[:n.value]
        return out[:, :3].copy(), out[:, 3].astype(np.int32), bool(fl.value & _lib.GM_RES_VOXEL_PASSTHROUGH)


    # ---- extensions (no reference counterpart; SURVEY.md par. 8a-ext) ----
    @staticmethod
    def _u8(a):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.uint8)
        return a, a.ctypes.data_as(C.POINTER(C.c_uint8))

    def nearest(self, cloud, queries):
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        q = np.ascontiguousarray(queries, dtype=np.float32)
        idx = np.empty(max(len(q), 1), dtype=np.int32)
        self._check(self._L.gm_nearest(self._ctx, _f32(xyz), len(xyz), _f32(q), len(q),
                                       idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx[:len(q)].copy()

    def plane_hypotheses(self, cloud, seed, H, labels=None, want=0):
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        lab, lp = self._u8(labels)
        out = np.empty((H, 4), dtype=np.float32)
        self._check(self._L.gm_plane_hypotheses(self._ctx, _f32(xyz), len(xyz), lp, want, seed, H, _f32(out)))
        return out

    def cylinder_hypotheses(self, cloud, normals, seed, H, labels=None, want=0):
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        lab, lp = self._u8(labels)
        out = np.empty((H, 7), dtype=np.float32)
        self._check(self._L.gm_cylinder_hypotheses(self._ctx, _f32(xyz), _f32(nrm), len(xyz), lp, want, seed, H, _f32(out)))
        return out

    def _score(self, fn, cloud, hyp, tau, labels, want):
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        hyp = np.ascontiguousarray(hyp, dtype=np.float32)
        lab, lp = self._u8(labels)
        cnt = np.zeros(len(hyp), dtype=np.int32)
        self._check(fn(self._ctx, _f32(xyz), len(xyz), lp, want, _f32(hyp), len(hyp), float(tau),
                       cnt.ctypes.data_as(C.POINTER(C.c_int32))))
        return cnt

    def score_planes(self, cloud, hyp4, tau, labels=None, want=0):
        return self._score(self._L.gm_score_planes, cloud, hyp4, tau, labels, want)

    def score_cylinders(self, cloud, hyp7, tau, labels=None, want=0):
        return self._score(self._L.gm_score_cylinders, cloud, hyp7, tau, labels, want)

    def score_frame(self, model, hyp, tau, slot=0, unlabelled_only=False):
        """Inlier counts of caller-supplied hypotheses ([H,4] plane rows if model == 0, [H,7] cylinder rows if 1) on the
        valid cloud the last frame left in `slot` (owned points only when sharded): gm_score_frame."""
        w = 4 if model == 0 else 7
        hyp = np.ascontiguousarray(np.asarray(hyp, dtype=np.float32).reshape(-1, w))
        counts = np.zeros(max(len(hyp), 1), dtype=np.int32)
        if len(hyp):
            self._check(self._L.gm_score_frame(self._ctx, slot, int(model), _f32(hyp), len(hyp), float(tau),
                                               1 if unlabelled_only else 0, counts.ctypes.data_as(C.POINTER(C.c_int32))))
        return counts[:len(hyp)]

    def segment_moments(self, cloud, normals, labels, label):
        xyz = np.ascontiguousarray(cloud, dtype=np.float32)
        nrm = np.ascontiguousarray(normals, dtype=np.float32) if normals is not None else None
        lab, lp = self._u8(labels)
        mom = np.zeros(16, dtype=np.float64)
        self._check(self._L.gm_segment_moments(self._ctx, _f32(xyz), _f32(nrm) if nrm is not None else None, lp,
                                               len(xyz), label, mom.ctypes.data_as(C.POINTER(C.c_double))))
        return mom


    # ---- cylinder regression (GM_CFG_CYLINDER_FIT; getCylinder, tunnel_processing.hpp:56-59) ----
    @staticmethod
    def _fit(f):
        return dict(status=int(f.status), inliers=int(f.inliers), passes=int(f.passes),
                    point=np.array(f.point[:]), axis=np.array(f.axis[:]), radius=float(f.radius), rms=float(f.rms),
                    last_step=float(f.last_step), model=np.array(f.model[:], dtype=np.float32),
                    ok=(int(f.status) & _lib.GM_FIT_FAILED_MASK) == 0,
                    converged=(int(f.status) & _lib.GM_FIT_NOT_CONVERGED) == 0)

    def cylinder_fit(self, slot=0):
        """The least-squares cylinder of the slot's last frame (gm_get_cylinder_fit): dict with status, inliers, passes,
        point, axis, radius, rms, last_step, model (the fp32 row the labels were decided with), ok, converged."""
        f = CylinderFit()
        self._check(self._L.gm_get_cylinder_fit(self._ctx, slot, C.byref(f)))
        return self._fit(f)

    def getCylinder(self, cloud, init7, tau, labels=None, want=0):
        """tunnel_processing.hpp:56-59 (the reference's empty regression stub) as one stage call (gm_fit_cylinder):
        points with labels == want (all when labels is None), starting row init7 (point, direction, radius).
        Returns (fit dict as cylinder_fit, boolean inlier mask [n])."""
        n, head = _stage_front(cloud, None, labels)
        init = np.ascontiguousarray(np.asarray(init7, dtype=np.float32).reshape(7))
        mask = np.zeros(max(n, 1), dtype=np.uint8)
        f = CylinderFit()
        self._check(self._L.gm_fit_cylinder(self._ctx, *head, int(want), _f32(init), float(tau), C.byref(f),
                                            mask.ctypes.data_as(C.POINTER(C.c_uint8))))
        return self._fit(f), mask[:n].astype(bool)

    # ---- wall deviation map (GM_CFG_SURFACE_MAP; include/gm_hip.h states the semantics) ----
    @staticmethod
    def surface_params(**kw):
        """gm_surface_params with the library's defaults, then the keywords (n_stations, n_sectors, station_length, t_min,
        gate, up, forward)."""
        return _lib.params(_lib.SurfaceParams, "gm_surface_default_params", "surface", kw)

    def set_surface_params(self, **kw):
        """gm_set_surface_params: the map parameters of the frames submitted after the call."""
        p = self.surface_params(**kw)
        self._check(self._L.gm_set_surface_params(self._ctx, C.byref(p)))

    @staticmethod
    def _surface(info, cells):
        """(info dict, count, mean, min, max arrays shaped (n_stations, n_sectors))."""
        d = {k: int(getattr(info, k)) for k in ("struct_size", "status", "n_stations", "n_sectors", "mapped", "outside",
                                                  "beyond_gate", "plane", "cells_hit")}
        for k in ("o", "a", "u", "v"):
            d[k] = np.array(getattr(info, k)[:], dtype=np.float32)
        for k in ("R", "t_min", "station_length", "sector_angle"):
            d[k] = np.float32(getattr(info, k))
        shape = (d["n_stations"], d["n_sectors"])
        nc = shape[0] * shape[1]
        raw = np.frombuffer(bytes(cells), dtype=np.uint8)[:16 * nc].reshape(nc, 16)
        count = raw[:, 0:4].copy().view(np.uint32).reshape(shape)
        mean, mn, mx = (raw[:, 4 * k:4 * k + 4].copy().view(np.float32).reshape(shape) for k in (1, 2, 3))
        return d, count, mean, mn, mx

    def surface_map(self, slot=0):
        """The map of the slot's last frame (gm_get_surface_map): (info dict, count, mean, min, max), the arrays shaped
        (n_stations, n_sectors)."""
        info = _lib.SurfaceInfo()
        n = C.c_uint32(0)
        st = self._L.gm_get_surface_map(self._ctx, slot, C.byref(info), None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            self._check(st)
        cells = (_lib.SurfaceCell * max(n.value, 1))()
        self._check(self._L.gm_get_surface_map(self._ctx, slot, C.byref(info), cells, n.value, C.byref(n)))
        return self._surface(info, cells)

    def surface_points(self, slot=0):
        """Per valid point of the slot's last frame: (residual e [n] float32, cell index [n] int32; -1 unless mapped)."""
        n = C.c_uint32(0)
        st = self._L.gm_get_surface_points(self._ctx, slot, None, None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            self._check(st)
        res = np.empty(max(n.value, 1), dtype=np.float32)
        cell = np.empty(max(n.value, 1), dtype=np.int32)
        if n.value:
            self._check(self._L.gm_get_surface_points(self._ctx, slot, _f32(res), cell.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      n.value, C.byref(n)))
        return res[:n.value].copy(), cell[:n.value].copy()

    def surfaceMap(self, cloud, model7, labels=None, **params):
        """The map as one stage call (gm_surface_map) on a host cloud [n,3] against model7 = (c, d, R) (e.g. a frame's
        cylinder_fit()["model"]); labels None: no point is plane.  Returns (info, count, mean, min, max, residual, cell)."""
        n, head = _stage_front(cloud, None, labels)
        m = np.ascontiguousarray(np.asarray(model7, dtype=np.float32).reshape(7))
        p = self.surface_params(**params)
        info = _lib.SurfaceInfo()
        nc = int(p.n_stations) * int(p.n_sectors)
        cells = (_lib.SurfaceCell * max(nc, 1))()
        out = _PointOutputs(n, True, _RES_CELL)
        self._check(self._L.gm_surface_map(self._ctx, *head, _f32(m), C.byref(p), C.byref(info), cells, nc, *out.ptrs()))
        return (*self._surface(info, cells), *out.tuple())

    def wall_map(self, arc=None, clothoid=None, **params):
        """A persistent wall map owned by this context (gm_wall_map_create): WallMap.  Keywords: gm_wall_params fields
        (n_stations, n_sectors, station_length, t_min, gate, point, direction, radius, up, forward).
        arc=dict(curvature=(x, y, z), point_chainage=s0): a map on a circular-arc design axis (gm_wall_map_create_arc).
        clothoid=dict(normal=(x, y, z), curvature=k0, rate=c, point_chainage=s0): a map on a transition curve
        (gm_wall_map_create_clothoid); not together with arc."""
        return WallMap(self, arc=arc, clothoid=clothoid, **params)

    def wall_alignment(self, elements, **params):
        """A wall alignment owned by this context (gm_wall_alignment_create): WallAlignment.  elements: wall_element()
        structs or dicts of its keywords, in order; keywords: the template gm_wall_params of element 0 (n_stations is
        not read)."""
        return WallAlignment(self, elements, **params)


# every record dtype is its struct's: _lib.py states each layout once
RAW_CELL = np.dtype(_lib.WallRawCell)                           # gm_wall_raw_cell, 24 bytes
_CELL = np.dtype(_lib.SurfaceCell)                              # gm_surface_cell, 16 bytes
REGION = np.dtype(_lib.WallRegion)                              # gm_wall_region, 64 bytes
WALL_CLOUD_POINT = np.dtype(_lib.WallCloudPoint)                # gm_wall_cloud_point, 40 bytes
WALL_MESH_TRIANGLE = np.dtype("<u4")   # gm_wall_mesh_triangle is three of them: meshes are uint32 [nt, 3]
WALL_CHECK_POINT = np.dtype(_lib.WallCheckPoint)                # gm_wall_check_point, 32 bytes
WALL_OBJECT = np.dtype(_lib.WallObject)                         # gm_wall_object, 128 bytes
WALL_ALIGN_SCORE = np.dtype(_lib.WallAlignScore)                # gm_wall_align_score, 24 bytes
WALL_CLEARANCE_STATION = np.dtype(_lib.WallClearanceStation)    # gm_wall_clearance_station, 32 bytes
WALL_CLEARANCE_CELL = np.dtype(_lib.WallClearanceCell)          # gm_wall_clearance_cell, 16 bytes
WALL_CLEARANCE_RUN = np.dtype(_lib.WallClearanceRun)            # gm_wall_clearance_run, 72 bytes
WALL_QUANTITY = np.dtype(_lib.WallQuantity)                     # gm_wall_quantity, 88 bytes
WALL_QUANTITY_RUN = np.dtype(_lib.WallQuantityRun)              # gm_wall_quantity_run, 136 bytes
WALL_SECTION = np.dtype(_lib.WallSection)                       # gm_wall_section, 144 bytes
WALL_SECTION_SUMS = np.dtype(_lib.WallSectionSums)              # gm_wall_section_sums, 448 bytes
# the keys of an info dict are its struct's fields less struct_size and reserved, except where written out
_REGION_METRICS = _lib.info_fields(_lib.WallRegionMetrics)
_CLOUD_INFO = _lib.info_fields(_lib.WallCloudInfo)
_CHECK_INFO = _lib.info_fields(_lib.WallCheckInfo)
_OBJECTS_INFO = _lib.info_fields(_lib.WallObjectsInfo)
_CLEARANCE_INFO = _lib.info_fields(_lib.WallClearanceInfo)
_QUANTITIES_INFO = _lib.info_fields(_lib.WallQuantitiesInfo)
_SECTIONS_INFO = _lib.info_fields(_lib.WallSectionsInfo)
_WALL_VEC = ("point", "direction", "up", "forward")
_REGION_INFO = ("station0", "n_stations", "n_sectors", "threshold_q", "flagged_pos", "flagged_neg", "unusable", "empty",
                "components", "regions")
_MESH_INFO = ("wrapped", "quads", "quads_two", "quads_one", "quads_none", "cut_by_step", "triangles")
_ADD_CHECKED_INFO = ("status", "min_delta_q", "n_points", "n_rows", "rows_neg", "rows_pos", "rows_kept", "rows_rejected",
                     "skipped", "plane", "beyond_gate", "outside", "mapped", "reserved")
_ALIGN_INT = ("status", "n_points", "plane", "beyond_gate", "outside_patch", "binned", "patch_cells_usable", "anchor_station",
              "half_patch_stations", "max_station_shift", "max_sector_shift", "overlap", "best_station", "best_sector")
_ALIGN_F64 = ("frac_station", "frac_sector", "shift_m", "roll", "bias_m", "rms_best", "rms_runner", "distinction")


def _wall_params(**kw):
    return _lib.params(_lib.WallParams, "gm_wall_default_params", "wall map", kw)


def _wall_region_params(**kw):
    return _lib.params(_lib.WallRegionParams, "gm_wall_region_default_params", "region", kw)


def _wall_cloud_params(**kw):
    return _lib.params(_lib.WallCloudParams, "gm_wall_cloud_default_params", "cloud", kw)


def _wall_clearance_params(**kw):
    return _lib.params(_lib.WallClearanceParams, "gm_wall_clearance_default_params", "clearance", kw)


def _wall_section_params(**kw):
    return _lib.params(_lib.WallSectionParams, "gm_wall_section_default_params", "section", kw)


def _wall_quantity_params(**kw):
    return _lib.params(_lib.WallQuantityParams, "gm_wall_quantity_default_params", "quantity", kw)


def _wall_check_params(**kw):
    return _lib.params(_lib.WallCheckParams, "gm_wall_check_default_params", "check", kw)


def _wall_add_checked_params(**kw):
    return _lib.params(_lib.WallAddCheckedParams, "gm_wall_add_checked_default_params", "checked-add", kw)


def _wall_locate_params(**kw):
    return _lib.params(_lib.WallLocateParams, "gm_wall_locate_default_params", "locate", kw)


def _wall_align_params(**kw):
    return _lib.params(_lib.WallAlignParams, "gm_wall_align_default_params", "align", kw)


def _wall_object_params(**kw):
    return _lib.params(_lib.WallObjectParams, "gm_wall_object_default_params", "object", kw)


def wall_check_classify(raw_cell, e, **params):
    """gm_wall_check_classify (host only): (delta int, cls int) of one RAW_CELL record and one fp32 residual under the
    check parameters given as keywords.  plane and outside are not decidable from these inputs."""
    r = np.ascontiguousarray(np.asarray(raw_cell, dtype=RAW_CELL).reshape(1))
    p = _wall_check_params(**params)
    d, c = C.c_int64(0), C.c_uint32(0)
    st = _lib.load().gm_wall_check_classify(C.byref(p), r.ctypes.data_as(C.POINTER(_lib.WallRawCell)), C.c_float(float(np.float32(e))),
                                            C.byref(d), C.byref(c))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_check_classify refused the parameters")
    return int(d.value), int(c.value)


def _align_info(i):
    d = {k: int(getattr(i, k)) for k in _ALIGN_INT}
    d.update({k: float(getattr(i, k)) for k in _ALIGN_F64})
    d["pose"] = np.array(i.pose[:], dtype=np.float64).reshape(3, 4)
    d["bytes"] = bytes(i)
    return d


def align_select(wall_params, pose, table, **params):
    """gm_wall_align_select (host only): the info dict of the selection and the pose from a WALL_ALIGN_SCORE table of
    (2A + 1)(2B + 1) records, under the map parameters `wall_params` (a gm_wall_params, WallMap.params()) and the align
    parameters given as keywords.  The device's counts (n_points, the classes, patch_cells_usable) are 0."""
    t = np.ascontiguousarray(np.asarray(table, dtype=WALL_ALIGN_SCORE).reshape(-1))
    m = WallMap._pose(pose)
    p = _wall_align_params(**params)
    info = _lib.WallAlignInfo()
    st = _lib.load().gm_wall_align_select(C.byref(wall_params), C.byref(p), m.ctypes.data_as(C.POINTER(C.c_double)),
                                          t.ctypes.data_as(C.POINTER(_lib.WallAlignScore)), len(t), C.byref(info))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_align_select refused its arguments")
    return _align_info(info)


def object_metrics(prm, obj, **params):
    """gm_wall_object_metrics (host only): the fp64 metrics dict (centroid and size as float64 [3]) of one WALL_OBJECT
    record under the gm_wall_params `prm` and the object parameters given as keywords."""
    r = np.ascontiguousarray(np.asarray(obj, dtype=WALL_OBJECT).reshape(1))
    op = _wall_object_params(**params)
    out = _lib.WallObjectMetrics()
    st = _lib.load().gm_wall_object_metrics(C.byref(prm), C.byref(op), r.ctypes.data_as(C.POINTER(_lib.WallObject)), C.byref(out))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_object_metrics refused the record")
    return _metrics_dict(out)


def _metrics_dict(out):
    d = {k: (float if t is C.c_double else int)(getattr(out, k)) for k, t in out._fields_ if k not in ("centroid", "size")}
    d["centroid"] = np.array(out.centroid[:], dtype=np.float64)
    d["size"] = np.array(out.size[:], dtype=np.float64)
    return d


def _objects_request(ctx, call, n_rows, rows, info, info_dict, metrics):
    """A count query, then the sized call; call(info, objects, capacity, got, object_of_row) is the bound ABI call.
    Each of the two runs the whole device pipeline (the library keeps no result between calls), so this binding
    launches every kernel twice per request; a caller that minds sizes the record buffer itself and calls the ABI
    once, as tools/wall_objects_timing.py does.  info_dict(info) and metrics(record) shape the result."""
    got = C.c_uint32(0)
    of_row = np.full(max(n_rows, 1), -1, dtype=np.int32) if rows else None
    rowp = of_row.ctypes.data_as(C.POINTER(C.c_int32)) if rows else None
    obj = _sized(lambda rp, cap, sized: ctx._check(call(C.byref(info), rp, cap, C.byref(got), rowp if sized else None)),
                 _lib.WallObject, got, lambda cap: cap or rows)
    return info_dict(info), obj, [metrics(obj[i]) for i in range(len(obj))], (of_row[:n_rows].copy() if rows else None)


def wall_region_metrics(prm, region):
    """gm_wall_region_metrics (host only): the fp64 metrics dict of one REGION record under the gm_wall_params `prm`."""
    r = np.ascontiguousarray(np.asarray(region, dtype=REGION).reshape(1))
    out = _lib.WallRegionMetrics()
    st = _lib.load().gm_wall_region_metrics(C.byref(prm), r.ctypes.data_as(C.POINTER(_lib.WallRegion)), C.byref(out))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_region_metrics refused the record")
    return {k: float(getattr(out, k)) for k in _REGION_METRICS}


def _gauge_tables(gauge_q, n_sectors):
    g = np.ascontiguousarray(np.asarray(gauge_q, dtype=np.int32))
    if g.ndim == 1:
        g = g.reshape(1, -1)
    if g.ndim != 2 or g.shape[1] != n_sectors or g.shape[0] < 1:
        raise ValueError("gauge_q must be shaped (n_sectors,) or (n_gauges, n_sectors)")
    return g


def wall_gauge_from_polygon(prm, uv, offset=(0.0, 0.0)):
    """gm_wall_gauge_from_polygon (host only): the int32 [n_sectors] gauge table (units of 2^-20 m) of the closed simple
    polygon uv [n_vertices, 2] (along u, along v; metres about the design axis), shifted by `offset`, for a map with the
    gm_wall_params `prm`."""
    L = _lib.load()
    p = np.ascontiguousarray(np.asarray(uv, dtype=np.float64).reshape(-1, 2))
    off = np.ascontiguousarray(np.asarray(offset, dtype=np.float64).reshape(2))
    out = np.zeros(int(prm.n_sectors), dtype=np.int32)
    got = C.c_uint32(0)
    st = L.gm_wall_gauge_from_polygon(C.byref(prm), p.ctypes.data_as(C.POINTER(C.c_double)), len(p),
                                      off.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                      len(out), C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_gauge_from_polygon refused the polygon")
    return out


def wall_clearance_runs(prm, stations, station0=0, max_gap=0):
    """gm_wall_clearance_runs (host only): the WALL_CLEARANCE_RUN records of the WALL_CLEARANCE_STATION records of a
    window that starts at map station `station0`, flagged stations joined across at most `max_gap` quiet ones."""
    L = _lib.load()
    s = np.ascontiguousarray(np.asarray(stations, dtype=WALL_CLEARANCE_STATION).reshape(-1))
    sp = s.ctypes.data_as(C.POINTER(_lib.WallClearanceStation)) if len(s) else None
    got = C.c_uint32(0)
    st = L.gm_wall_clearance_runs(C.byref(prm), sp, len(s), int(station0), int(max_gap), None, 0, C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_clearance_runs refused its arguments")
    runs = np.zeros(max(int(got.value), 1), dtype=WALL_CLEARANCE_RUN)
    st = L.gm_wall_clearance_runs(C.byref(prm), sp, len(s), int(station0), int(max_gap),
                                  runs.ctypes.data_as(C.POINTER(_lib.WallClearanceRun)), len(runs), C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_clearance_runs failed")
    return runs[:int(got.value)].copy()


WALL_QUANTITY_UNMEASURED = 0xFF
WALL_QUANTITY_CLASSES = ("unmeasured", "empty", "unusable", "under", "over", "within")   # GM_WALL_QUANTITY_CLASS_* order
WALL_QUANTITY_RUNS_ALL_ZONES = 1


def _quantity_tables(lo_q, hi_q, n_sectors):
    lo, hi = _gauge_tables(lo_q, n_sectors), _gauge_tables(hi_q, n_sectors)
    if lo.shape != hi.shape:
        raise ValueError("lo_q and hi_q must have the same shape")
    return lo, hi


def _u8_or_none(a):
    """(the array kept alive, its uint8 pointer) of an optional uint8 vector."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(-1))
    return a, (a.ctypes.data_as(C.POINTER(C.c_uint8)) if len(a) else None)


def wall_quantity_check_params(prm, lo_q, hi_q, n=0, section_profile=None, zone=None, n_zones=1, params=None, n_profiles=None):
    """gm_wall_quantity_check_params (host only): the status for a map with the gm_wall_params `prm`, a window of `n`
    stations, the line tables lo_q / hi_q (int32 (n_sectors,) or (n_profiles, n_sectors), passed as they are; n_profiles
    None: their first dimension) and the optional tables; params: a gm_wall_quantity_params or None."""
    lo = np.ascontiguousarray(np.asarray(lo_q, dtype=np.int32))
    hi = np.ascontiguousarray(np.asarray(hi_q, dtype=np.int32))
    if n_profiles is None:
        n_profiles = lo.shape[0] if lo.ndim == 2 else 1
    sp, spp = _u8_or_none(section_profile)
    zn, znp = _u8_or_none(zone)
    return _lib.load().gm_wall_quantity_check_params(
        C.byref(prm), C.byref(params) if params is not None else None, lo.ctypes.data_as(C.POINTER(C.c_int32)),
        hi.ctypes.data_as(C.POINTER(C.c_int32)), n_profiles, spp, int(n), znp, int(n_zones))


def wall_quantity_column(radius_q, count, total, lo, hi, base=None, min_count=8, zone_entry=0):
    """gm_wall_quantity_column (host only): one column restated -- (count, total) its merged raw pair, base the
    baseline's (count, sum) or None.  Returns a dict: cls (an index into WALL_QUANTITY_CLASSES), v (None when the column
    is not usable), under_area, over_area, excess_area, over_line."""
    out = _lib.WallQuantityColumnResult()
    bc, bs = (int(base[0]), int(base[1])) if base is not None else (0, 0)
    st = _lib.load().gm_wall_quantity_column(int(radius_q), int(count), int(total), int(base is not None), bc, bs, int(min_count),
                                             int(lo), int(hi), int(zone_entry), C.byref(out))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_quantity_column refused its arguments")
    d = {k: int(getattr(out, k)) for k, _t in _lib.WallQuantityColumnResult._fields_}
    if d["v"] == -2 ** 31:
        d["v"] = None
    return d


def wall_quantity_metrics(prm, record):
    """gm_wall_quantity_metrics (host only): the fp64 metrics dict of one WALL_QUANTITY record under the gm_wall_params
    `prm`."""
    r = np.ascontiguousarray(np.asarray(record, dtype=WALL_QUANTITY).reshape(1))
    out = _lib.WallQuantityMetrics()
    st = _lib.load().gm_wall_quantity_metrics(C.byref(prm), r.ctypes.data_as(C.POINTER(_lib.WallQuantity)), C.byref(out))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_quantity_metrics refused the record")
    return {k: float(getattr(out, k)) for k, _t in _lib.WallQuantityMetrics._fields_ if k != "reserved"}


def wall_quantity_runs(prm, records, n_zones=1, run_sections=1, all_zones=False):
    """gm_wall_quantity_runs (host only): the WALL_QUANTITY_RUN records of the WALL_QUANTITY records [sections, n_zones]
    of one call, folded into pay intervals of `run_sections` sections, per zone or over all zones."""
    L = _lib.load()
    r = np.ascontiguousarray(np.asarray(records, dtype=WALL_QUANTITY).reshape(-1))
    if int(n_zones) < 1 or len(r) % int(n_zones):
        raise ValueError("records must hold n_zones records per section")
    rp = r.ctypes.data_as(C.POINTER(_lib.WallQuantity)) if len(r) else None
    ns, flags = len(r) // int(n_zones), WALL_QUANTITY_RUNS_ALL_ZONES if all_zones else 0
    got = C.c_uint32(0)
    st = L.gm_wall_quantity_runs(C.byref(prm), rp, ns, int(n_zones), int(run_sections), flags, None, 0, C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_quantity_runs refused its arguments")
    runs = np.zeros(max(int(got.value), 1), dtype=WALL_QUANTITY_RUN)
    st = L.gm_wall_quantity_runs(C.byref(prm), rp, ns, int(n_zones), int(run_sections), flags,
                                 runs.ctypes.data_as(C.POINTER(_lib.WallQuantityRun)), len(runs), C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_quantity_runs failed")
    return runs[:int(got.value)].copy()


def wall_section_basis(n_sectors, harmonics=2):
    """gm_wall_section_basis (host only): the int32 (n_sectors, 1 + 2 harmonics) table gm_wall_map_sections uses."""
    L = _lib.load()
    got = C.c_uint32(0)
    st = L.gm_wall_section_basis(int(n_sectors), int(harmonics), None, 0, C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_section_basis refused its arguments")
    out = np.zeros(int(got.value), dtype=np.int32)
    st = L.gm_wall_section_basis(int(n_sectors), int(harmonics), out.ctypes.data_as(C.POINTER(C.c_int32)), len(out), C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_section_basis failed")
    return out.reshape(int(n_sectors), 1 + 2 * int(harmonics))


def wall_section_solve(sums, harmonics=2, min_columns=24):
    """gm_wall_section_solve (host only): (coef_q int64 [9], status) of one WALL_SECTION_SUMS record."""
    s = np.ascontiguousarray(np.asarray(sums, dtype=WALL_SECTION_SUMS).reshape(1))
    cq = np.zeros(9, dtype=np.int64)
    status = C.c_uint32(0)
    st = _lib.load().gm_wall_section_solve(s.ctypes.data_as(C.POINTER(_lib.WallSectionSums)), int(harmonics), int(min_columns),
                                           cq.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(status))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_section_solve refused its arguments")
    return cq, int(status.value)


def wall_section_metrics(prm, section, harmonics=2):
    """gm_wall_section_metrics (host only): the fp64 metrics dict (centre as float64 [3]) of one WALL_SECTION record under
    the gm_wall_params `prm`."""
    r = np.ascontiguousarray(np.asarray(section, dtype=WALL_SECTION).reshape(1))
    out = _lib.WallSectionMetrics()
    st = _lib.load().gm_wall_section_metrics(C.byref(prm), r.ctypes.data_as(C.POINTER(_lib.WallSection)), int(harmonics),
                                             C.byref(out))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_section_metrics refused the record")
    d = {k: float(getattr(out, k)) for k, _t in _lib.WallSectionMetrics._fields_ if k != "centre"}
    d["centre"] = np.array(out.centre[:], dtype=np.float64)
    return d


def wall_cloud_directions(prm, **params):
    """gm_wall_cloud_directions (host only): the (NK, 2) float64 table of (cos, sin) that gm_wall_map_cloud uses on a map
    with the gm_wall_params `prm` under the cloud parameters given as keywords (block_sectors decides)."""
    L = _lib.load()
    c = _wall_cloud_params(**params)
    got = C.c_uint32(0)
    st = L.gm_wall_cloud_directions(C.byref(prm), C.byref(c), None, 0, C.byref(got))
    if st not in (_lib.GM_OK, _lib.GM_ERR_CAPACITY):
        raise _lib.GmError(st, "gm_wall_cloud_directions refused the parameters")
    out = np.empty((int(got.value), 2), dtype=np.float64)
    st = L.gm_wall_cloud_directions(C.byref(prm), C.byref(c), out.ctypes.data_as(C.POINTER(C.c_double)), len(out), C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_cloud_directions failed")
    return out


def wall_arc(curvature, point_chainage=0.0):
    """gm_wall_arc from its two fields."""
    a = _lib.WallArc()
    a.struct_size = C.sizeof(_lib.WallArc)
    a.curvature[:] = [float(x) for x in curvature]
    a.point_chainage = float(point_chainage)
    return a


def _arc_call(name, st):
    if st != _lib.GM_OK:
        raise _lib.GmError(st, f"{name} refused the arguments")


def _d3():
    return np.empty(3, dtype=np.float64)


def _axis_add_info(i):
    """A gm_wall_arc_add_info or gm_wall_clothoid_add_info as a dict (rate: where the struct has one)."""
    d = dict(status=int(i.status), anchor_station=int(i.anchor_station), sensor_chainage=float(i.sensor_chainage),
             anchor_chainage=float(i.anchor_chainage))
    for k in ("o", "a", "n", "b"):
        d[k] = np.array(getattr(i, k)[:], dtype=np.float32)
    for k in ("kappa", "rate", "un", "ub", "vn", "vb", "R", "station_length", "sector_angle", "gate"):
        if hasattr(i, k):
            d[k] = np.float32(getattr(i, k))
    return d


def _project_each(name, call, xyz):
    """The project entry `name` on map points [n, 3], one `call(x, chainage, angle, e)` per point: (chainage, angle, e),
    float64 [n] each."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(x), 3), dtype=np.float64)
    s, ph, e = C.c_double(), C.c_double(), C.c_double()
    for k in range(len(x)):
        _arc_call(name, call(_dptr(x[k]), C.byref(s), C.byref(ph), C.byref(e)))
        out[k] = (s.value, ph.value, e.value)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def _point_each(name, call, chainage, angle, rho):
    """The point entry `name` at (chainage, angle, rho), broadcast, one `call(chainage, angle, rho, xyz)` per point:
    float64 [n, 3]."""
    s, ph, r = np.broadcast_arrays(np.asarray(chainage, np.float64), np.asarray(angle, np.float64), np.asarray(rho, np.float64))
    s, ph, r = s.reshape(-1), ph.reshape(-1), r.reshape(-1)
    out = np.empty((len(s), 3), dtype=np.float64)
    for k in range(len(s)):
        _arc_call(name, call(float(s[k]), float(ph[k]), float(r[k]), _dptr(out[k])))
    return out


def wall_arc_add_frame(prm, arc, pose):
    """gm_wall_arc_add_frame (host only): the per-add frame of an arc map with the gm_wall_params `prm` and the gm_wall_arc
    `arc` under `pose`: dict of anchor_station, sensor_chainage, anchor_chainage, o, a, n, b (float32 [3]) and the fp32
    constants kappa, un, ub, vn, vb, R, station_length, sector_angle, gate."""
    m = WallMap._pose(pose)
    i = _lib.WallArcAddInfo()
    _arc_call("gm_wall_arc_add_frame", _lib.load().gm_wall_arc_add_frame(C.byref(prm), C.byref(arc), _dptr(m), C.byref(i)))
    return _axis_add_info(i)


def wall_arc_frame(prm, arc, chainage):
    """gm_wall_arc_frame (host only): the design frame (o, a, u, v) at `chainage`, float64 [3] each."""
    o, a, u, v = _d3(), _d3(), _d3(), _d3()
    _arc_call("gm_wall_arc_frame", _lib.load().gm_wall_arc_frame(C.byref(prm), C.byref(arc), float(chainage), _dptr(o), _dptr(a),
                                                                 _dptr(u), _dptr(v)))
    return o, a, u, v


def wall_arc_project(prm, arc, xyz):
    """gm_wall_arc_project (host only) on map points [n, 3]: (chainage, angle, e), float64 [n] each."""
    L = _lib.load()
    return _project_each("gm_wall_arc_project", lambda *a: L.gm_wall_arc_project(C.byref(prm), C.byref(arc), *a), xyz)


def wall_arc_point(prm, arc, chainage, angle, rho):
    """gm_wall_arc_point (host only): the map points at (chainage, angle, rho), broadcast; float64 [n, 3]."""
    L = _lib.load()
    return _point_each("gm_wall_arc_point", lambda *a: L.gm_wall_arc_point(C.byref(prm), C.byref(arc), *a), chainage, angle, rho)


def wall_clothoid(normal, curvature=0.0, rate=0.0, point_chainage=0.0):
    """gm_wall_clothoid from its four fields."""
    c = _lib.WallClothoid()
    c.struct_size = C.sizeof(_lib.WallClothoid)
    c.normal[:] = [float(x) for x in normal]
    c.curvature, c.rate, c.point_chainage = float(curvature), float(rate), float(point_chainage)
    return c


def wall_clothoid_check_params(prm, clothoid):
    """gm_wall_clothoid_check_params (host only): the status (GM_OK or GM_ERR_INVALID_ARG)."""
    return int(_lib.load().gm_wall_clothoid_check_params(C.byref(prm), C.byref(clothoid)))


def wall_clothoid_add_frame(prm, clothoid, pose):
    """gm_wall_clothoid_add_frame (host only): the per-add frame of a clothoid map with the gm_wall_params `prm` and the
    gm_wall_clothoid `clothoid` under `pose`: wall_arc_add_frame's dict, kappa being the curvature at the anchor section,
    plus rate."""
    m = WallMap._pose(pose)
    i = _lib.WallClothoidAddInfo()
    _arc_call("gm_wall_clothoid_add_frame",
              _lib.load().gm_wall_clothoid_add_frame(C.byref(prm), C.byref(clothoid), _dptr(m), C.byref(i)))
    return _axis_add_info(i)


def wall_clothoid_frame(prm, clothoid, chainage):
    """gm_wall_clothoid_frame (host only): the design frame (o, a, u, v) at `chainage`, float64 [3] each, the signed
    curvature there and the normal n(s) it turns toward."""
    o, a, u, v, n = _d3(), _d3(), _d3(), _d3(), _d3()
    k = C.c_double()
    _arc_call("gm_wall_clothoid_frame",
              _lib.load().gm_wall_clothoid_frame(C.byref(prm), C.byref(clothoid), float(chainage), _dptr(o), _dptr(a), _dptr(u),
                                                 _dptr(v), C.byref(k), _dptr(n)))
    return o, a, u, v, float(k.value), n


def wall_clothoid_project(prm, clothoid, xyz):
    """gm_wall_clothoid_project (host only) on map points [n, 3]: (chainage, angle, e), float64 [n] each."""
    L = _lib.load()
    return _project_each("gm_wall_clothoid_project", lambda *a: L.gm_wall_clothoid_project(C.byref(prm), C.byref(clothoid), *a), xyz)


def wall_clothoid_point(prm, clothoid, chainage, angle, rho):
    """gm_wall_clothoid_point (host only): the map points at (chainage, angle, rho), broadcast; float64 [n, 3]."""
    L = _lib.load()
    return _point_each("gm_wall_clothoid_point", lambda *a: L.gm_wall_clothoid_point(C.byref(prm), C.byref(clothoid), *a),
                       chainage, angle, rho)


def _wall_mesh_info(info):
    d = _ints(info, _MESH_INFO)
    d["cloud"] = _ints(info.cloud, _CLOUD_INFO)
    return d


def _wall_mesh_rows(vertices):
    v = np.ascontiguousarray(vertices, dtype=WALL_CLOUD_POINT).reshape(-1)
    return v, (v.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)) if len(v) else None)


def wall_mesh_triangulate(NJ, NK, vertices, flags=0, max_step=0.0):
    """gm_wall_mesh_triangulate (host only): the mesh's triangle rule on a vertex list -- WALL_CLOUD_POINT rows of a cloud
    of NJ x NK blocks.  Returns (info dict with the mesh's counts and the cloud's grid under "cloud", uint32 [nt, 3])."""
    L = _lib.load()
    v, vp = _wall_mesh_rows(vertices)
    info, got = _lib.WallMeshInfo(), C.c_uint64(0)
    args = (int(NJ), int(NK), vp, len(v), int(flags), float(max_step), C.byref(info))
    st = L.gm_wall_mesh_triangulate(*args, None, 0, C.byref(got))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, "gm_wall_mesh_triangulate refused the arguments")
    cap = int(got.value)
    tri = np.zeros((max(cap, 1), 3), dtype=WALL_MESH_TRIANGLE)
    if cap:
        st = L.gm_wall_mesh_triangulate(*args, tri.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle)), cap, C.byref(got))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_mesh_triangulate failed")
    return _wall_mesh_info(info), tri[:cap].copy()


def wall_mesh_write_ply(path, vertices, triangles):
    """gm_wall_mesh_write_ply (host only): the mesh as a binary little-endian PLY file (x, y, z, mean, min, max per vertex;
    uint vertex_indices per face)."""
    v, vp = _wall_mesh_rows(vertices)
    t = np.ascontiguousarray(triangles, dtype=WALL_MESH_TRIANGLE).reshape(-1, 3)
    tp = t.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle)) if len(t) else None
    st = _lib.load().gm_wall_mesh_write_ply(os.fsencode(path), vp, len(v), tp, len(t))
    if st != _lib.GM_OK:
        raise _lib.GmError(st, f"gm_wall_mesh_write_ply could not write {path!r}")


class _FrameLoop:
    """The frame loop of a wall map and of a wall alignment, written once: add, check, checked add, locate and align of
    a slot's frame (*_frame enqueues, *_result fetches) or of a host cloud (*_points).  The ABI entry of a method is
    `_prefix` + its name; a class states its structs and their converters to dicts:
      _Plan, _plan_info, _plan_key                  what an add, a check and a checked add return at once -- the map's add
                                                    info, the alignment's plan -- and its key in a *_points info dict
      _AlignPlan, _align_plan_info, _align_plan_key the same of an align
      _CheckInfo, _LocateInfo, _AlignInfo           the results (converters _check_info, _locate_info, _align_dict)
      _EXTRA                                        per-point outputs beyond the map's: the alignment's owner element"""

    def _abi(self, name, *args):
        self._ctx._check(getattr(self._L, self._prefix + name)(self._h(), *args))

    def _frame(self, name, slot, pose, *args):
        self._abi(name, self._ctx._ctx, slot, _dptr(WallMap._pose(pose)), *args)

    def add_frame(self, slot=0, pose=np.eye(4)[:3]):
        """*_add_frame: enqueue the slot's last submitted frame under `pose` (sensor -> map).  Returns the add info dict
        of a map, the plan dict of an alignment (computed on the host; the kernel may still be running)."""
        i = self._Plan()
        self._frame("add_frame", slot, pose, C.byref(i))
        return self._plan_info(i)

    def add_points(self, cloud, pose=np.eye(4)[:3], labels=None, outputs=True):
        """*_add_points on a host cloud [n,3]: (add info or plan, residual [n] float32, cell [n] int32 -- relative to the
        owner's map on an alignment, which adds element [n] int32); outputs False skips the per-point arrays (None each)."""
        n, head = _stage_front(cloud, pose, labels)
        i, out = self._Plan(), _PointOutputs(n, outputs, _RES_CELL + self._EXTRA)
        self._abi("add_points", *head, C.byref(i), *out.ptrs())
        return (self._plan_info(i), *out.tuple())

    def sync(self):
        self._abi("sync")

    def check_frame(self, slot=0, pose=np.eye(4)[:3], **params):
        """*_check_frame: enqueue the check of the slot's last submitted frame under `pose`, on an alignment every point
        against its owner's map (keywords: reference, min_count, threshold, gate).  Returns the add info dict (its gate is
        the check's) or the plan dict; check_result() fetches the result."""
        p, i = _wall_check_params(**params), self._Plan()
        self._frame("check_frame", slot, pose, C.byref(p), C.byref(i))
        return self._plan_info(i)

    def check_result(self, slot=0):
        """*_get_check: (info dict, WALL_CHECK_POINT records ascending by index) of the last check on the slot; on an
        alignment split_cell() splits their cell.  A count query first, then the sized call."""
        info, got = self._CheckInfo(), C.c_uint32(0)
        pts = _sized(lambda rp, cap, sized: self._abi("get_check", slot, C.byref(info), rp, cap, C.byref(got)), _lib.WallCheckPoint,
                     got, lambda cap: cap)
        return self._check_info(info), pts

    def check_points(self, cloud, pose=np.eye(4)[:3], labels=None, outputs=True, **params):
        """*_check_points on a host cloud [n,3]: (info dict with the add info under "add" or the plan under "plan",
        records, dict(e float32, cell int32, delta int32, cls uint8 and on an alignment element int32) or None without
        outputs).  The list buffer holds n rows: one call."""
        n, head = _stage_front(cloud, pose, labels)
        p = _wall_check_params(**params)
        plan, info, got = self._Plan(), self._CheckInfo(), C.c_uint32(0)
        pts = np.zeros(max(n, 1), dtype=WALL_CHECK_POINT)
        out = _PointOutputs(n, outputs, _CHECK_OUT + self._EXTRA)
        self._abi("check_points", *head, C.byref(p), C.byref(plan), C.byref(info), _rptr(pts, _lib.WallCheckPoint), n,
                  C.byref(got), *out.ptrs())
        d = self._check_info(info)
        d[self._plan_key] = self._plan_info(plan)
        return d, pts[:int(got.value)].copy(), out.dict()

    def add_frame_checked(self, slot=0, pose=np.eye(4)[:3], **params):
        """*_add_frame_checked: enqueue the add of the slot's last submitted frame under `pose`, less the points the slot's
        last check_frame on this object selected (keywords: skip, min_delta).  Returns the add info or plan dict;
        add_checked_result() fetches the counts."""
        p, i = _wall_add_checked_params(**params), self._Plan()
        self._frame("add_frame_checked", slot, pose, C.byref(p), C.byref(i))
        return self._plan_info(i)

    def add_checked_result(self, slot=0):
        """*_get_add_checked: the info dict of the last checked add on the slot (waits for that call only)."""
        info = _lib.WallAddCheckedInfo()
        self._abi("get_add_checked", slot, C.byref(info))
        return WallMap._add_checked_info(info)

    def add_points_checked(self, cloud, pose, rows, labels=None, outputs=True, **params):
        """*_add_points_checked on a host cloud [n,3] and WALL_CHECK_POINT rows (any order, duplicates allowed): (info
        dict with the add info under "add" or the plan under "plan", then add_points' per-point arrays)."""
        n, head = _stage_front(cloud, pose, labels)
        p = _wall_add_checked_params(**params)
        r = np.ascontiguousarray(np.asarray(rows, dtype=WALL_CHECK_POINT).reshape(-1))
        plan, info, out = self._Plan(), _lib.WallAddCheckedInfo(), _PointOutputs(n, outputs, _RES_CELL + self._EXTRA)
        self._abi("add_points_checked", *head, C.byref(p), _rptr(r, _lib.WallCheckPoint) if len(r) else None, len(r),
                  C.byref(plan), C.byref(info), *out.ptrs())
        d = WallMap._add_checked_info(info)
        d[self._plan_key] = self._plan_info(plan)
        return (d, *out.tuple())

    def locate_frame(self, slot=0, pose=np.eye(4)[:3], **params):
        """*_locate_frame: enqueue the correction of `pose` for the slot's last submitted frame (keywords: reference,
        min_count, gate).  Returns at once; locate_result() fetches the result."""
        p = _wall_locate_params(**params)
        self._frame("locate_frame", slot, pose, C.byref(p))

    def locate_result(self, slot=0):
        """*_get_locate: the info dict (_locate_info) of the last locate on the slot -- status, passes, n_points,
        anchor_station, pose (3, 4) float64 (NaN when status & GM_LOCATE_FAILED_MASK), lateral, tilt, pass (a list of three
        dicts: o, a, u, v, gate, the five class counts, rms, step) and bytes (the raw gm_wall_locate_info)."""
        info = self._LocateInfo()
        self._abi("get_locate", slot, C.byref(info))
        return self._locate_info(info)

    def locate_points(self, cloud, pose=np.eye(4)[:3], labels=None, outputs=True, **params):
        """*_locate_points on a host cloud [n,3]: (info dict, then add_points' per-point arrays of the last pass that ran,
        element being the owner under the caller's pose); outputs False skips the per-point arrays."""
        n, head = _stage_front(cloud, pose, labels)
        p = _wall_locate_params(**params)
        info, out = self._LocateInfo(), _PointOutputs(n, outputs, _RES_CELL + self._EXTRA)
        self._abi("locate_points", *head, C.byref(p), C.byref(info), *out.ptrs())
        return (self._locate_info(info), *out.tuple())

    def align_frame(self, slot=0, pose=np.eye(4)[:3], **params):
        """*_align_frame: enqueue the chainage and roll alignment of `pose` for the slot's last submitted frame (keywords:
        gm_wall_align_params').  Returns the add info dict (its gate is the align's) or the align's plan dict at once;
        align_result() fetches the result."""
        p, i = _wall_align_params(**params), self._AlignPlan()
        self._frame("align_frame", slot, pose, C.byref(p), C.byref(i))
        return self._align_plan_info(i)

    def align_result(self, slot=0):
        """*_get_align: (info dict, WALL_ALIGN_SCORE table shaped (2A + 1, 2B + 1)) of the last align on the slot.  The
        info holds status, the class counts, anchor_station, P, A, B as used, overlap, best_station, best_sector, the
        fractions, shift_m, roll, bias_m, rms_best, rms_runner, distinction, pose (3, 4) float64 (NaN when
        status & GM_ALIGN_FAILED_MASK) and bytes (the raw gm_wall_align_info).  A count query first, then the sized call."""
        info, got = self._AlignInfo(), C.c_uint32(0)
        t = _sized(lambda rp, cap, sized: self._abi("get_align", slot, C.byref(info) if sized else None, rp, cap,
                                                    C.byref(got)), _lib.WallAlignScore, got, lambda cap: True)
        d = self._align_dict(info)
        return d, t.reshape(2 * d["max_station_shift"] + 1, 2 * d["max_sector_shift"] + 1)

    def _align_points(self, cloud, pose, labels, outputs, params):
        """*_align_points: (info dict with the align's plan, table, the _PointOutputs)."""
        n, head = _stage_front(cloud, pose, labels)
        p = _wall_align_params(**params)
        plan, info, got = self._AlignPlan(), self._AlignInfo(), C.c_uint32(0)
        na, nb = 2 * int(p.max_station_shift) + 1, 2 * int(p.max_sector_shift) + 1
        t = np.zeros(na * nb, dtype=WALL_ALIGN_SCORE)
        out = _PointOutputs(n, outputs, _ALIGN_OUT + self._EXTRA)
        self._abi("align_points", *head, C.byref(p), C.byref(plan), C.byref(info), _rptr(t, _lib.WallAlignScore), len(t),
                  C.byref(got), *out.ptrs())
        d = self._align_dict(info)
        d[self._align_plan_key] = self._align_plan_info(plan)
        return d, t.reshape(na, nb), out


class WallMap(_FrameLoop):
    """One gm_wall_map: a device-resident developed wall map against a design cylinder, accumulated over posed frames
    (include/gm_hip.h states the rule).  Created by GeometricMapping.wall_map(); dies with its context.  The frame loop
    (add_*, check_*, add_*_checked, locate_*, align_*) is _FrameLoop's."""

    _prefix, _EXTRA = "gm_wall_map_", ()
    _Plan = _AlignPlan = _lib.WallAddInfo
    _plan_key = _align_plan_key = "add"
    _CheckInfo, _LocateInfo, _AlignInfo = _lib.WallCheckInfo, _lib.WallLocateInfo, _lib.WallAlignInfo

    def __init__(self, ctx, arc=None, clothoid=None, **params):
        self._ctx, self._L = ctx, ctx._L
        self._map = None
        p = self.params(**params)
        h = C.c_void_p()
        if arc is not None and clothoid is not None:
            raise ValueError("wall_map: arc= and clothoid= exclude each other")
        if clothoid is not None:
            cl = clothoid if isinstance(clothoid, _lib.WallClothoid) else wall_clothoid(**clothoid)
            ctx._check(self._L.gm_wall_map_create_clothoid(ctx._ctx, C.byref(p), C.byref(cl), C.byref(h)))
        elif arc is None:
            ctx._check(self._L.gm_wall_map_create(ctx._ctx, C.byref(p), C.byref(h)))
        else:
            a = arc if isinstance(arc, _lib.WallArc) else wall_arc(**arc)
            ctx._check(self._L.gm_wall_map_create_arc(ctx._ctx, C.byref(p), C.byref(a), C.byref(h)))
        self._map, self.prm = h, p
        self.n_stations, self.n_sectors = int(p.n_stations), int(p.n_sectors)
        if not hasattr(ctx, "_walls"):
            ctx._walls = []
        ctx._walls.append(self)

    @staticmethod
    def params(**kw):
        """gm_wall_params with the library's defaults, then the keywords."""
        return _wall_params(**kw)

    @property
    def arc(self):
        """gm_wall_map_get_arc: dict(curvature float64 [3], point_chainage), or None on a straight map."""
        a = self.arc_struct()
        c = np.array(a.curvature[:], dtype=np.float64)
        return dict(curvature=c, point_chainage=float(a.point_chainage)) if np.any(c != 0.0) else None

    def arc_struct(self):
        """The map's gm_wall_arc (curvature 0 on a straight map), as the host helpers wall_arc_* take it."""
        a = _lib.WallArc()
        self._ctx._check(self._L.gm_wall_map_get_arc(self._h(), C.byref(a)))
        return a

    @property
    def clothoid(self):
        """gm_wall_map_get_clothoid: dict(normal float64 [3], curvature, rate, point_chainage), or None on other maps."""
        c = self.clothoid_struct()
        if not c.struct_size:
            return None
        return dict(normal=np.array(c.normal[:], dtype=np.float64), curvature=float(c.curvature), rate=float(c.rate),
                    point_chainage=float(c.point_chainage))

    def clothoid_struct(self):
        """The map's gm_wall_clothoid (all-zero on other maps), as the host helpers wall_clothoid_* take it."""
        c = _lib.WallClothoid()
        self._ctx._check(self._L.gm_wall_map_get_clothoid(self._h(), C.byref(c)))
        return c

    @classmethod
    def _borrowed(cls, ctx, handle, prm):
        """A WallMap on a handle somebody else owns (an alignment's element map): close() leaves the map alone."""
        m = cls.__new__(cls)
        m._ctx, m._L, m._map, m.prm, m._owned = ctx, ctx._L, handle, prm, False
        m.n_stations, m.n_sectors = int(prm.n_stations), int(prm.n_sectors)
        if not hasattr(ctx, "_walls"):
            ctx._walls = []
        ctx._walls.append(m)
        return m

    def close(self):
        if self._map is not None:
            if getattr(self, "_owned", True):
                self._L.gm_wall_map_destroy(self._map)
            self._map = None
            if self in getattr(self._ctx, "_walls", []):
                self._ctx._walls.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _h(self):
        if self._map is None:
            raise ValueError("the wall map is closed (or its context is)")
        return self._map

    @staticmethod
    def _pose(pose):
        m = np.asarray(pose, dtype=np.float64)
        if m.shape == (4, 4):
            m = m[:3]
        if m.shape != (3, 4):
            raise ValueError("pose must be a (3, 4) or (4, 4) array")
        return np.ascontiguousarray(m)

    @staticmethod
    def _add_info(i):
        d = dict(status=int(i.status), anchor_station=int(i.anchor_station))
        for k in ("o", "a", "u", "v"):
            d[k] = np.array(getattr(i, k)[:], dtype=np.float32)
        for k in ("R", "station_length", "sector_angle", "gate"):
            d[k] = np.float32(getattr(i, k))
        return d

    _plan_info = _align_plan_info = _add_info
    _align_dict = staticmethod(_align_info)

    def info(self):
        i = _lib.WallInfo()
        self._ctx._check(self._L.gm_wall_map_info(self._h(), C.byref(i)))
        d = {k: int(getattr(i, k)) for k in ("status", "n_stations", "n_sectors", "frames", "mapped", "outside", "beyond_gate",
                                             "plane", "cells_hit")}
        for k in ("o", "a", "u", "v"):
            d[k] = np.array(getattr(i, k)[:], dtype=np.float64)
        d["R"] = float(i.R)
        return d

    def _window(self, station0, n):
        return int(station0), int(self.n_stations - station0 if n is None else n)

    def read(self, station0=0, n=None):
        """gm_wall_map_read: (count, mean, min, max) of stations [station0, station0 + n), each shaped (n, n_sectors)."""
        s0, n = self._window(station0, n)
        nc = n * self.n_sectors
        buf = np.empty(max(nc, 1), dtype=_CELL)
        got = C.c_uint64(0)
        self._ctx._check(self._L.gm_wall_map_read(self._h(), s0, n, buf.ctypes.data_as(C.POINTER(_lib.SurfaceCell)), nc,
                                                  C.byref(got)))
        b = buf[:nc].reshape(n, self.n_sectors)
        return tuple(np.ascontiguousarray(b[k]) for k in ("count", "mean", "min", "max"))

    def read_raw(self, station0=0, n=None):
        """gm_wall_map_read_raw: a structured array (RAW_CELL: sum, count, min_key, max_key, reserved) shaped (n, n_sectors)."""
        s0, n = self._window(station0, n)
        nc = n * self.n_sectors
        buf = np.zeros(max(nc, 1), dtype=RAW_CELL)
        got = C.c_uint64(0)
        self._ctx._check(self._L.gm_wall_map_read_raw(self._h(), s0, n, buf.ctypes.data_as(C.POINTER(_lib.WallRawCell)), nc,
                                                      C.byref(got)))
        return buf[:nc].reshape(n, self.n_sectors).copy()

    def add_raw(self, raw, station0=0):
        """gm_wall_map_add_raw: merge a (n, n_sectors) RAW_CELL window (counts and sums add, keys take the maximum)."""
        raw = np.ascontiguousarray(raw, dtype=RAW_CELL)
        if raw.ndim != 2 or raw.shape[1] != self.n_sectors:
            raise ValueError("raw must be shaped (n, n_sectors)")
        self._ctx._check(self._L.gm_wall_map_add_raw(self._h(), int(station0), raw.shape[0],
                                                     raw.ctypes.data_as(C.POINTER(_lib.WallRawCell))))

    def clear(self, station0=0, n=None):
        s0, n = self._window(station0, n)
        self._ctx._check(self._L.gm_wall_map_clear(self._h(), s0, n))

    @staticmethod
    def region_params(**kw):
        """gm_wall_region_params with the library's defaults, then the keywords (min_count, min_cells, connectivity,
        threshold)."""
        return _wall_region_params(**kw)

    def regions(self, station0=0, n=None, baseline=None, labels=False, **params):
        """gm_wall_map_regions: the connected deviation regions of stations [station0, station0 + n) against the design or,
        with `baseline` (another WallMap of this context on the same grid), against that earlier epoch.  Returns
        (info dict, regions REGION array ascending by label, metrics list of dicts, labels (n, n_sectors) int32 or None)."""
        s0, n = self._window(station0, n)
        p = self.region_params(**params)
        bh = baseline._h() if baseline is not None else None
        info, got = _lib.WallRegionsInfo(), C.c_uint32(0)
        lab = np.empty(max(n * self.n_sectors, 1), dtype=np.int32) if labels else None
        lp = lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None
        # a count query, then the list (the labels travel with the second call only)
        reg = _sized(lambda rp, cap, sized: self._abi("regions", bh, s0, n, C.byref(p), C.byref(info), rp, cap, C.byref(got),
                                                      lp if sized else None), _lib.WallRegion, got, lambda cap: cap or labels)
        d = _ints(info, _REGION_INFO)
        d["cell_area"] = float(info.cell_area)
        metrics = [wall_region_metrics(self.prm, reg[i]) for i in range(len(reg))]
        return d, reg, metrics, (lab[:n * self.n_sectors].reshape(n, self.n_sectors).copy() if labels else None)

    @staticmethod
    def cloud_params(**kw):
        """gm_wall_cloud_params with the library's defaults, then the keywords (block_stations, block_sectors, min_count,
        exaggeration, anchor)."""
        return _wall_cloud_params(**kw)

    def cloud(self, station0=0, n=None, **params):
        """gm_wall_map_cloud: stations [station0, station0 + n) as a point list, one WALL_CLOUD_POINT record per block of
        block_stations x block_sectors cells that holds min_count points, ascending by block.  Returns (info dict,
        records).  A count query first, then the sized call."""
        s0, n = self._window(station0, n)
        p = self.cloud_params(**params)
        info, got = _lib.WallCloudInfo(), C.c_uint64(0)
        pts = _sized(lambda rp, cap, sized: self._abi("cloud", s0, n, C.byref(p), C.byref(info), rp, cap, C.byref(got)),
                     _lib.WallCloudPoint, got, lambda cap: cap)
        return _ints(info, _CLOUD_INFO), pts

    def mesh(self, station0=0, n=None, flags=0, max_step=0.0, **cloud_params):
        """gm_wall_map_mesh: stations [station0, station0 + n) as an indexed triangle mesh.  The vertices are cloud()'s rows
        under the same cloud parameters; flags are GM_WALL_MESH_*; max_step > 0 drops triangles whose corners' means differ
        by more.  Returns (info dict with the cloud's under "cloud", vertices, uint32 [nt, 3]).  A count query first, then
        the sized call."""
        s0, n = self._window(station0, n)
        p = _lib.WallMeshParams()
        self._L.gm_wall_mesh_default_params(C.byref(p))
        p.flags, p.max_step, p.cloud = int(flags), float(max_step), self.cloud_params(**cloud_params)
        info = _lib.WallMeshInfo()
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        self._ctx._check(self._L.gm_wall_map_mesh(self._h(), s0, n, C.byref(p), C.byref(info), None, 0, None, 0, C.byref(nv),
                                                  C.byref(nt)))
        cv, ct = int(nv.value), int(nt.value)
        pts = np.zeros(max(cv, 1), dtype=WALL_CLOUD_POINT)
        tri = np.zeros((max(ct, 1), 3), dtype=WALL_MESH_TRIANGLE)
        if cv:
            self._ctx._check(self._L.gm_wall_map_mesh(
                self._h(), s0, n, C.byref(p), C.byref(info), pts.ctypes.data_as(C.POINTER(_lib.WallCloudPoint)), cv,
                tri.ctypes.data_as(C.POINTER(_lib.WallMeshTriangle)) if ct else None, ct, C.byref(nv), C.byref(nt)))
        return _wall_mesh_info(info), pts[:int(nv.value)].copy(), tri[:int(nt.value)].copy()

    @staticmethod
    def clearance_params(**kw):
        """gm_wall_clearance_params with the library's defaults, then the keywords (reference, min_count, margin)."""
        return _wall_clearance_params(**kw)

    def clearance(self, station0, n, gauge_q, station_gauge=None, **params):
        """gm_wall_map_clearance: stations [station0, station0 + n) (n None: to the end) against the gauge table(s)
        gauge_q, int32 (n_sectors,) or (n_gauges, n_sectors) in units of 2^-20 m; station_gauge (uint8 [n], optional)
        picks the table of each window station.  Returns (info dict, WALL_CLEARANCE_STATION records, WALL_CLEARANCE_CELL
        records ascending by cell).  A count query first, then the sized call."""
        s0, n = self._window(station0, n)
        p = self.clearance_params(**params)
        g = _gauge_tables(gauge_q, self.n_sectors)
        gp = g.ctypes.data_as(C.POINTER(C.c_int32))
        sg = sgp = None
        if station_gauge is not None:
            sg = np.ascontiguousarray(np.asarray(station_gauge, dtype=np.uint8).reshape(-1))
            if len(sg) != n:
                raise ValueError("station_gauge must hold one entry per window station")
            sgp = sg.ctypes.data_as(C.POINTER(C.c_uint8)) if n else None
        info, got = _lib.WallClearanceInfo(), C.c_uint64(0)
        st = np.zeros(max(n, 1), dtype=WALL_CLEARANCE_STATION)
        stp = _rptr(st, _lib.WallClearanceStation)

        def call(rp, cap, sized):   # the station records travel with the sized call, which a window with stations makes
            self._abi("clearance", s0, n, gp, g.shape[0], sgp, C.byref(p), C.byref(info), stp if sized else None,
                      n if sized else 0, rp, cap, C.byref(got))
        cells = _sized(call, _lib.WallClearanceCell, got, lambda cap: n)
        return _ints(info, _CLEARANCE_INFO), st[:n].copy(), cells

    @staticmethod
    def section_params(**kw):
        """gm_wall_section_params with the library's defaults, then the keywords (section_stations, harmonics, passes,
        min_count, min_columns, max_gap_deg, reject)."""
        return _wall_section_params(**kw)

    def sections(self, station0=0, n=None, baseline=None, sums=False, **params):
        """gm_wall_map_sections: the profile fit per section of stations [station0, station0 + n) against the design or,
        with `baseline` (another WallMap of this context on the same grid), against that earlier epoch.  Returns
        (info dict, WALL_SECTION records, WALL_SECTION_SUMS records of the last fitting pass or None)."""
        s0, n = self._window(station0, n)
        p = self.section_params(**params)
        bh = baseline._h() if baseline is not None else None
        info = _lib.WallSectionsInfo()
        got = C.c_uint32(0)
        S = max(int(p.section_stations), 1)
        cap = (n + S - 1) // S
        rec = np.zeros(max(cap, 1), dtype=WALL_SECTION)
        sm = np.zeros(max(cap, 1), dtype=WALL_SECTION_SUMS) if sums else None
        self._ctx._check(self._L.gm_wall_map_sections(
            self._h(), bh, s0, n, C.byref(p), C.byref(info), rec.ctypes.data_as(C.POINTER(_lib.WallSection)), cap, C.byref(got),
            sm.ctypes.data_as(C.POINTER(_lib.WallSectionSums)) if sums else None))
        ns = int(got.value)
        return _ints(info, _SECTIONS_INFO), rec[:ns].copy(), (sm[:ns].copy() if sums else None)

    def section_basis(self, harmonics=2):
        """gm_wall_section_basis for this map's n_sectors."""
        return wall_section_basis(self.n_sectors, harmonics)

    @staticmethod
    def section_solve(sums, harmonics=2, min_columns=24):
        """gm_wall_section_solve (host only)."""
        return wall_section_solve(sums, harmonics, min_columns)

    def section_metrics(self, section, harmonics=2):
        """gm_wall_section_metrics of one WALL_SECTION record under this map's parameters."""
        return wall_section_metrics(self.prm, section, harmonics)

    @staticmethod
    def quantity_params(**kw):
        """gm_wall_quantity_params with the library's defaults, then the keywords (section_stations, min_count)."""
        return _wall_quantity_params(**kw)

    def quantities(self, lo_q, hi_q, station0=0, n=None, baseline=None, section_profile=None, zone=None, n_zones=1,
                   profile_rows=False, **params):
        """gm_wall_map_quantities: under- and overbreak per section and zone of stations [station0, station0 + n) against
        the two lines lo_q / hi_q, int32 (n_sectors,) or (n_profiles, n_sectors), offsets in units of 2^-20 m from the
        design radius or, with `baseline` (another WallMap of this context on the same grid), from that earlier wall.
        section_profile (uint8 per section, optional) picks each section's table; zone (uint8 [n_sectors], optional, 0xFF:
        not measured) its sectors' zones.  Returns (info dict, WALL_QUANTITY records [sections, n_zones], the int32
        profile rows [sections, n_sectors] or None)."""
        s0, n = self._window(station0, n)
        p = self.quantity_params(**params)
        lo, hi = _quantity_tables(lo_q, hi_q, self.n_sectors)
        i32 = C.POINTER(C.c_int32)
        S = max(int(p.section_stations), 1)
        NS, nz = (n + S - 1) // S, int(n_zones)
        sp, spp = _u8_or_none(section_profile)
        zn, znp = _u8_or_none(zone)
        if sp is not None and len(sp) != NS:
            raise ValueError("section_profile must hold one entry per section")
        if zn is not None and len(zn) != self.n_sectors:
            raise ValueError("zone must hold one entry per sector")
        bh = baseline._h() if baseline is not None else None
        info = _lib.WallQuantitiesInfo()
        got = C.c_uint32(0)
        cap = NS * max(nz, 0)
        rec = np.zeros(max(cap, 1), dtype=WALL_QUANTITY)
        rows = np.zeros(max(NS * self.n_sectors, 1), dtype=np.int32) if profile_rows else None
        self._ctx._check(self._L.gm_wall_map_quantities(
            self._h(), bh, s0, n, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32), lo.shape[0], spp, znp, nz, C.byref(p),
            C.byref(info), rec.ctypes.data_as(C.POINTER(_lib.WallQuantity)), cap, C.byref(got),
            rows.ctypes.data_as(i32) if profile_rows else None))
        nr = int(got.value)
        out_rows = rows[:NS * self.n_sectors].reshape(NS, self.n_sectors).copy() if profile_rows else None
        return _ints(info, _QUANTITIES_INFO), rec[:nr].reshape(NS, nz).copy(), out_rows

    def quantity_metrics(self, record):
        """gm_wall_quantity_metrics of one WALL_QUANTITY record under this map's parameters."""
        return wall_quantity_metrics(self.prm, record)

    def quantity_runs(self, records, n_zones=1, run_sections=1, all_zones=False):
        """gm_wall_quantity_runs of one call's records under this map's parameters."""
        return wall_quantity_runs(self.prm, records, n_zones, run_sections, all_zones)

    @staticmethod
    def check_params(**kw):
        """gm_wall_check_params with the library's defaults, then the keywords (reference, min_count, threshold, gate)."""
        return _wall_check_params(**kw)

    @staticmethod
    def _check_info(i):
        return _ints(i, _CHECK_INFO)

    @staticmethod
    def add_checked_params(**kw):
        """gm_wall_add_checked_params with the library's defaults, then the keywords (skip, min_delta)."""
        return _wall_add_checked_params(**kw)

    @staticmethod
    def _add_checked_info(i):
        return _ints(i, _ADD_CHECKED_INFO)

    @staticmethod
    def locate_params(**kw):
        """gm_wall_locate_params with the library's defaults, then the keywords (reference, min_count, gate)."""
        return _wall_locate_params(**kw)

    @staticmethod
    def _locate_info(i):
        d = dict(status=int(i.status), passes=int(i.passes), n_points=int(i.n_points), anchor_station=int(i.anchor_station),
                 pose=np.array(i.pose[:], dtype=np.float64).reshape(3, 4), lateral=np.array(i.lateral[:], dtype=np.float64),
                 tilt=np.array(i.tilt[:], dtype=np.float64), bytes=bytes(i))
        d["pass"] = []
        for r in i.pass_:
            q = {k: np.array(getattr(r, k)[:], dtype=np.float32) for k in ("o", "a", "u", "v")}
            q["gate"] = np.float32(r.gate)
            q.update({k: int(getattr(r, k)) for k in ("plane", "outside", "unsurveyed", "gated", "used")})
            q["rms"] = float(r.rms)
            q["step"] = np.array(r.step[:], dtype=np.float64)
            d["pass"].append(q)
        return d

    @staticmethod
    def align_params(**kw):
        """gm_wall_align_params with the library's defaults, then the keywords (half_patch_stations, max_station_shift,
        max_sector_shift, min_count, min_frame_count, min_overlap, gate, clip, min_distinction)."""
        return _wall_align_params(**kw)

    def align_points(self, cloud, pose=np.eye(4)[:3], labels=None, outputs=True, **params):
        """gm_wall_map_align_points on a host cloud [n,3]: (info dict with the add info under "add", table, residual [n]
        float32, cell [n] int32: jr * n_sectors + k of a binned point, else -1); outputs False skips the per-point arrays
        (None, None)."""
        d, t, out = self._align_points(cloud, pose, labels, outputs, params)
        return (d, t, *out.tuple())

    @staticmethod
    def object_params(**kw):
        """gm_wall_object_params with the library's defaults, then the keywords (block_stations, block_sectors,
        min_block_points, min_points, connectivity, half_window_stations)."""
        return _wall_object_params(**kw)

    def _objects(self, call, n_rows, rows, p):
        """_objects_request with this map's info and metrics."""
        return _objects_request(self._ctx, call, n_rows, rows, _lib.WallObjectsInfo(), lambda i: _ints(i, _OBJECTS_INFO),
                                lambda o: object_metrics(self.prm, o, **p))

    def check_objects(self, slot=0, rows=False, **params):
        """gm_wall_map_check_objects: the changed points of the last check on the slot grouped into objects on the device.
        Returns (info dict, WALL_OBJECT records ascending by (label, sign), metrics list of dicts, object_of_row int32 per
        changed row in check_result()'s order or None without rows).  Two device passes (see _objects); rows=True costs one
        further gm_wall_map_get_check count query for the row count."""
        p = self.object_params(**params)
        n_rows = 0
        if rows:
            got = C.c_uint32(0)
            self._ctx._check(self._L.gm_wall_map_get_check(self._h(), slot, None, None, 0, C.byref(got)))
            n_rows = int(got.value)

        def call(info, obj, cap, got, of_row):
            return self._L.gm_wall_map_check_objects(self._h(), slot, C.byref(p), info, obj, cap, got, of_row, n_rows if of_row else 0)
        return self._objects(call, n_rows, rows, params)

    def objects_of_rows(self, rows, anchor_station, **params):
        """gm_wall_check_objects: the same kernels on host rows (WALL_CHECK_POINT records in any order) around the anchor
        station.  Returns (info dict, WALL_OBJECT records, metrics list, object_of_row int32 [len(rows)])."""
        p = self.object_params(**params)
        r = np.ascontiguousarray(rows, dtype=WALL_CHECK_POINT).reshape(-1)
        rp = r.ctypes.data_as(C.POINTER(_lib.WallCheckPoint)) if len(r) else None

        def call(info, obj, cap, got, of_row):
            return self._L.gm_wall_check_objects(self._h(), rp, len(r), int(anchor_station), C.byref(p), info, obj, cap, got, of_row)
        return self._objects(call, len(r), True, params)

    def object_metrics(self, obj, **params):
        """gm_wall_object_metrics of one WALL_OBJECT record under this map's parameters."""
        return object_metrics(self.prm, obj, **params)

    def save(self, path):
        """The parameters, the arc or the clothoid of a map on one, and the raw cells as one .npz (numpy only)."""
        p = self.prm
        kw = {k: np.array(getattr(p, k)[:], dtype=np.float64) for k in _WALL_VEC}
        arc = self.arc
        if arc is not None:
            kw.update(arc_curvature=arc["curvature"], arc_point_chainage=np.float64(arc["point_chainage"]))
        cl = self.clothoid
        if cl is not None:
            kw.update(clothoid_normal=cl["normal"], clothoid_scalars=np.array([cl["curvature"], cl["rate"], cl["point_chainage"]],
                                                                              dtype=np.float64))
        np.savez_compressed(path, n_stations=np.uint32(p.n_stations), n_sectors=np.uint32(p.n_sectors),
                            station_length=np.float64(p.station_length), t_min=np.float64(p.t_min), gate=np.float64(p.gate),
                            radius=np.float64(p.radius), raw=self.read_raw(), **kw)

    @staticmethod
    def load(ctx, path):
        """A new map on ctx with the file's parameters and cells (the per-class totals are not part of a file)."""
        with np.load(path) as z:
            kw = {k: z[k].tolist() for k in _WALL_VEC}
            if "arc_curvature" in z.files:
                kw["arc"] = dict(curvature=z["arc_curvature"].tolist(), point_chainage=float(z["arc_point_chainage"]))
            if "clothoid_normal" in z.files:
                k0, rate, s0 = (float(x) for x in z["clothoid_scalars"])
                kw["clothoid"] = dict(normal=z["clothoid_normal"].tolist(), curvature=k0, rate=rate, point_chainage=s0)
            m = WallMap(ctx, n_stations=int(z["n_stations"]), n_sectors=int(z["n_sectors"]),
                        station_length=float(z["station_length"]), t_min=float(z["t_min"]), gate=float(z["gate"]),
                        radius=float(z["radius"]), **kw)
            m.add_raw(z["raw"].astype(RAW_CELL, copy=False))
        return m


WALL_ELEMENT_KINDS = dict(straight=0, arc=1, clothoid=2)


def wall_element(kind, n_stations, turn=(0.0, 0.0), curvature=0.0, rate=0.0):
    """gm_wall_element: kind "straight", "arc" or "clothoid" (or the GM_WALL_ELEMENT_* number)."""
    e = _lib.WallElement()
    e.struct_size = C.sizeof(_lib.WallElement)
    e.kind = WALL_ELEMENT_KINDS.get(kind, kind)
    e.n_stations = int(n_stations)
    e.turn[:] = [float(x) for x in turn]
    e.curvature, e.rate = float(curvature), float(rate)
    return e


def _wall_elements(elements):
    els = [e if isinstance(e, _lib.WallElement) else wall_element(**e) for e in elements]
    return (_lib.WallElement * max(len(els), 1))(*els), len(els)


def _alignment_add_info(i):
    ns = int(i.n_sides)
    return dict(status=int(i.status), element=int(i.element), n_sides=ns, chainage=float(i.chainage), reach=float(i.reach),
                offset=float(i.offset), side_element=[int(x) for x in i.side_element[:ns]],
                side_anchor=[int(x) for x in i.side_anchor[:ns]],
                joint_o=np.array([list(r) for r in i.joint_o], dtype=np.float32)[:max(ns - 1, 0)],
                joint_a=np.array([list(r) for r in i.joint_a], dtype=np.float32)[:max(ns - 1, 0)])


def _alignment_align_plan(p):
    """The dict of a gm_wall_alignment_align_plan_info: add (the add's plan dict), anchor_global (G_f), total, row0
    [n_sides] int32, own, home and pieces [(element, first_row, n_stations)]."""
    ns, npc = int(p.add.n_sides), int(p.n_pieces)
    return dict(add=_alignment_add_info(p.add), anchor_global=int(p.anchor_global), total=int(p.total),
                row0=np.array(p.row0[:ns], dtype=np.int32), own=int(p.own), home=int(p.home), n_pieces=npc,
                pieces=[(int(q.element), int(q.first_row), int(q.n_stations)) for q in p.piece[:npc]])


def _alignment_align_info(i):
    """The dict of a gm_wall_alignment_align_info: WallMap.align_result()'s keys (bytes: the raw shared head), element,
    n_sides, chainage, anchor_global, side_class [n_sides, 4] uint32 (plane, beyond_gate, outside_patch, binned) and plan."""
    d = _align_info(i)
    d["bytes"] = bytes(i)[:C.sizeof(_lib.WallAlignInfo)]
    ns = int(i.n_sides)
    d.update(element=int(i.element), n_sides=ns, chainage=float(i.chainage), anchor_global=int(i.anchor_global),
             side_class=np.array([list(r) for r in i.side_class], dtype=np.uint32)[:ns], plan=_alignment_add_info(i.plan))
    return d


def _alignment_plan_struct(plan):
    """A gm_wall_alignment_add_info from a plan dict (element, side_element, side_anchor: what the object calls read) or
    the struct itself."""
    if isinstance(plan, _lib.WallAlignmentAddInfo):
        return plan
    i = _lib.WallAlignmentAddInfo()
    i.struct_size = C.sizeof(_lib.WallAlignmentAddInfo)
    i.element, i.n_sides = int(plan["element"]), len(plan["side_element"])
    for k in range(min(i.n_sides, 4)):
        i.side_element[k], i.side_anchor[k] = int(plan["side_element"][k]), int(plan["side_anchor"][k])
    return i


def _alignment_objects_info(i):
    """The dict of a gm_wall_alignment_objects_info: WallMap.check_objects()'s keys (station0 / n_stations global),
    element, n_sides, anchor_global, total and side_element, side_first, side_rows [n_sides]."""
    d = _ints(i, _OBJECTS_INFO + ("element", "n_sides", "anchor_global", "total"))
    d.update({k: [int(x) for x in getattr(i, k)[:d["n_sides"]]] for k in ("side_element", "side_first", "side_rows")})
    return d


class _AlignmentObjects:
    """gm_wall_alignment_check_objects and its kin for one WallAlignmentRule or WallAlignment `al`.  The public methods
    here are bound onto the instance by its __init__ (al.object_window, al.object_metrics; on a WallAlignment also
    al.check_objects, al.objects_of_rows) instead of being class attributes: tests/test_api_calls.py holds every callable
    of the three classes to a recorded trace, and these calls' trace is tests/test_wall_alignment_objects_abi.py's."""

    RULE, DEVICE = ("object_window", "object_metrics"), ("check_objects", "objects_of_rows")

    def __init__(self, al):
        self._al = al
        self.bind(self.RULE)

    def bind(self, names):
        for k in names:
            setattr(self._al, k, getattr(self, k))

    def object_window(self, plan, **params):
        """gm_wall_alignment_object_window: the info dict (_alignment_objects_info, the counts 0) of the object calls for
        `plan` (a plan dict or struct) under the object parameters given as keywords; GmError with GM_ERR_UNSUPPORTED for
        an alignment beyond the size rule."""
        p, pl, info = _wall_object_params(**params), _alignment_plan_struct(plan), _lib.WallAlignmentObjectsInfo()
        st = self._al._L.gm_wall_alignment_object_window(*self._al._head(), C.byref(pl), C.byref(p), C.byref(info))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_object_window refused the arguments")
        return _alignment_objects_info(info)

    def object_metrics(self, obj, **params):
        """gm_wall_alignment_object_metrics of one WALL_OBJECT record on the global station grid: WallMap.object_metrics'
        keys in alignment chainage, and element_from, element_to, station_from, station_to."""
        r = np.ascontiguousarray(np.asarray(obj, dtype=WALL_OBJECT).reshape(1))
        op, out = _wall_object_params(**params), _lib.WallAlignmentObjectMetrics()
        st = self._al._L.gm_wall_alignment_object_metrics(*self._al._head(), C.byref(op), r.ctypes.data_as(C.POINTER(_lib.WallObject)),
                                                      C.byref(out))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_object_metrics refused the record")
        return _metrics_dict(out)

    def _objects(self, call, n_rows, rows, p):
        return _objects_request(self._al._ctx, call, n_rows, rows, _lib.WallAlignmentObjectsInfo(), _alignment_objects_info,
                                lambda o: self.object_metrics(o, **p))

    def check_objects(self, slot=0, rows=False, **params):
        """gm_wall_alignment_check_objects: the changed points of the last check through the alignment on the slot as
        objects on the global station grid.  Returns WallMap.check_objects' tuple: (info dict, WALL_OBJECT records
        ascending by (label, sign), metrics list of dicts, object_of_row int32 per changed row in check_result()'s order
        or None without rows).  Two device passes (_objects_request); rows=True costs one further
        gm_wall_alignment_get_check count query for the row count."""
        p = _wall_object_params(**params)
        n_rows = 0
        if rows:
            got = C.c_uint32(0)
            self._al._ctx._check(self._al._L.gm_wall_alignment_get_check(self._al._h(), slot, None, None, 0, C.byref(got)))
            n_rows = int(got.value)

        def call(info, obj, cap, got, of_row):
            return self._al._L.gm_wall_alignment_check_objects(self._al._h(), slot, C.byref(p), info, obj, cap, got, of_row,
                                                           n_rows if of_row else 0)
        return self._objects(call, n_rows, rows, params)

    def objects_of_rows(self, rows, plan, **params):
        """gm_wall_alignment_check_objects_rows: the same kernels on host rows (WALL_CHECK_POINT records in any order,
        cell = side << 24 | cell) under the sides and the anchor of `plan` (a check's plan dict, or the struct).  Returns
        (info dict, WALL_OBJECT records, metrics list, object_of_row int32 [len(rows)])."""
        p, pl = _wall_object_params(**params), _alignment_plan_struct(plan)
        r = np.ascontiguousarray(rows, dtype=WALL_CHECK_POINT).reshape(-1)
        rp = r.ctypes.data_as(C.POINTER(_lib.WallCheckPoint)) if len(r) else None

        def call(info, obj, cap, got, of_row):
            return self._al._L.gm_wall_alignment_check_objects_rows(self._al._h(), rp, len(r), C.byref(pl), C.byref(p), info, obj, cap, got,
                                                                of_row)
        return self._objects(call, len(r), True, params)


_ALIGNMENT_REGION_INFO = _REGION_INFO + ("total", "n_pieces", "element_from", "element_to", "station_from", "station_to")


def _alignment_regions_info(i):
    """The dict of a gm_wall_alignment_regions_info: WallMap.regions()'s keys (station0 / n_stations global) and total,
    n_pieces, element_from, element_to, station_from, station_to."""
    d = _ints(i, _ALIGNMENT_REGION_INFO)
    d["cell_area"] = float(i.cell_area)
    return d


class _AlignmentRegions:
    """gm_wall_alignment_regions and its kin for one WallAlignmentRule or WallAlignment `al`, bound onto the instance as
    _AlignmentObjects' methods are and for the same reason (al.region_window, al.region_metrics; on a WallAlignment also
    al.regions); these calls' trace is tests/test_wall_alignment_regions_abi.py's."""

    RULE, DEVICE = ("region_window", "region_metrics"), ("regions",)

    def __init__(self, al):
        self._al = al
        self.bind(self.RULE)

    def bind(self, names):
        for k in names:
            setattr(self._al, k, getattr(self, k))

    def total(self):
        return sum(int(self._al._els[i].n_stations) for i in range(self._al.n_elements))

    def region_window(self, station0, n):
        """gm_wall_alignment_region_window: the info dict (_alignment_regions_info, threshold_q and the counts 0) of
        gm_wall_alignment_regions on the global stations [station0, station0 + n); GmError with GM_ERR_UNSUPPORTED for
        an alignment or a window beyond the size rule."""
        info = _lib.WallAlignmentRegionsInfo()
        st = self._al._L.gm_wall_alignment_region_window(*self._al._head(), int(station0), int(n), C.byref(info))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_region_window refused the arguments")
        return _alignment_regions_info(info)

    def region_metrics(self, region):
        """gm_wall_alignment_region_metrics of one REGION record on the global station grid: wall_region_metrics' keys in
        alignment chainage, element_from, element_to, station_from, station_to, peak_element, peak_station, peak_sector
        and peak_point float64 [3], the design position of the peak."""
        r = np.ascontiguousarray(np.asarray(region, dtype=REGION).reshape(1))
        out = _lib.WallAlignmentRegionMetrics()
        st = self._al._L.gm_wall_alignment_region_metrics(*self._al._head(), r.ctypes.data_as(C.POINTER(_lib.WallRegion)), C.byref(out))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_region_metrics refused the record")
        d = {k: (float if t is C.c_double else int)(getattr(out, k)) for k, t in out._fields_ if k not in ("peak_point", "reserved")}
        d["peak_point"] = np.array(out.peak_point[:], dtype=np.float64)
        return d

    def regions(self, station0=0, n=None, baseline=None, labels=False, **params):
        """gm_wall_alignment_regions: the connected deviation regions of the global stations [station0, station0 + n)
        (n None: to the alignment's end) against the design or, with `baseline` (another WallAlignment of this context
        with the same template and elements), against that earlier epoch; a region across a joint is one region.  Returns
        WallMap.regions' tuple: (info dict, REGION records ascending by label, metrics list of dicts from region_metrics,
        labels (n, n_sectors) int32 or None)."""
        al = self._al
        s0 = int(station0)
        n = self.total() - s0 if n is None else int(n)
        if s0 < 0 or n < 0:
            raise ValueError("the window leaves the alignment")
        nsec = int(al.prm.n_sectors)
        p = _wall_region_params(**params)
        bh = baseline._h() if baseline is not None else None
        info, got = _lib.WallAlignmentRegionsInfo(), C.c_uint32(0)
        lab = np.empty(max(n * nsec, 1), dtype=np.int32) if labels else None
        lp = lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None
        # a count query, then the list (the labels travel with the second call only)
        reg = _sized(lambda rp, cap, sized: al._ctx._check(al._L.gm_wall_alignment_regions(
            al._h(), bh, s0, n, C.byref(p), C.byref(info), rp, cap, C.byref(got), lp if sized else None)),
            _lib.WallRegion, got, lambda cap: cap or labels)
        metrics = [self.region_metrics(reg[i]) for i in range(len(reg))]
        return _alignment_regions_info(info), reg, metrics, (lab[:n * nsec].reshape(n, nsec).copy() if labels else None)


class WallAlignmentRule:
    """The device-free half of a wall alignment (gm_wall_alignment_check, _element_params, _project, _point, _window,
    _add_plan; include/gm_hip.h states the rule): a template gm_wall_params and the elements.  Needs no context."""

    wall_element = staticmethod(wall_element)

    def __init__(self, elements, **params):
        self._L = _lib.load()
        self.prm = WallMap.params(**params)
        self._els, self.n_elements = _wall_elements(elements)
        self._object_calls = _AlignmentObjects(self)
        self._region_calls = _AlignmentRegions(self)

    def _head(self):
        return C.byref(self.prm), self._els, self.n_elements

    def check(self):
        """gm_wall_alignment_check: the status."""
        return int(self._L.gm_wall_alignment_check(*self._head()))

    def element_params(self, i):
        """gm_wall_alignment_element_params: (gm_wall_params, gm_wall_arc or None, gm_wall_clothoid or None) of element i,
        what GeometricMapping.wall_map(arc=, clothoid=, **params) takes for a bitwise-equal map."""
        p, a, c = _lib.WallParams(), _lib.WallArc(), _lib.WallClothoid()
        _arc_call("gm_wall_alignment_element_params",
                  self._L.gm_wall_alignment_element_params(*self._head(), int(i), C.byref(p), C.byref(a), C.byref(c)))
        return p, (a if a.struct_size else None), (c if c.struct_size else None)

    def project(self, xyz):
        """gm_wall_alignment_project on map points [n, 3]: (element int64 [n], chainage, angle, e float64 [n]).  One
        library call per point, and each call chains the alignment anew (include/gm_hip.h gives the cost): for poses,
        windows and synthetic frames, not for a cloud per frame."""
        k_, el = C.c_uint32(), []

        def call(x, *out):
            st = self._L.gm_wall_alignment_project(*self._head(), x, C.byref(k_), *out)
            el.append(k_.value)
            return st

        s, ph, e = _project_each("gm_wall_alignment_project", call, xyz)
        return np.array(el, dtype=np.int64), s, ph, e

    def point(self, chainage, angle, rho):
        """gm_wall_alignment_point: the map points at (chainage, angle, rho), broadcast; float64 [n, 3].  One library call
        per point, as project."""
        return _point_each("gm_wall_alignment_point", lambda *a: self._L.gm_wall_alignment_point(*self._head(), *a),
                           chainage, angle, rho)

    def window(self, s_from, s_to):
        """gm_wall_alignment_window: the pieces (element, station0, n_stations) of the chainage interval, in order."""
        got = C.c_uint32(0)
        st = self._L.gm_wall_alignment_window(*self._head(), float(s_from), float(s_to), None, 0, C.byref(got))
        if st not in (_lib.GM_OK, _lib.GM_ERR_CAPACITY):
            raise _lib.GmError(st, "gm_wall_alignment_window refused the arguments")
        buf = (_lib.WallAlignmentPiece * max(int(got.value), 1))()
        _arc_call("gm_wall_alignment_window",
                  self._L.gm_wall_alignment_window(*self._head(), float(s_from), float(s_to), buf, int(got.value), C.byref(got)))
        return [(int(b.element), int(b.station0), int(b.n_stations)) for b in buf[:int(got.value)]]

    def add_plan(self, pose, bound):
        """gm_wall_alignment_add_plan: the plan dict of an add under `pose` on a context whose boxFilterBound is `bound`;
        GmError with GM_ERR_UNSUPPORTED for more than four sides."""
        m = WallMap._pose(pose)
        i = _lib.WallAlignmentAddInfo()
        st = self._L.gm_wall_alignment_add_plan(*self._head(), _dptr(m), float(bound), C.byref(i))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_add_plan refused the arguments")
        return _alignment_add_info(i)

    def locate_plan(self, pose, bound):
        """gm_wall_alignment_locate_plan: what a locate under `pose` starts from -- home (index among the sides), add (the
        add's plan dict), the state c, d, u, v and s0, the home section o_f, a, fu, fv in map coordinates, side [n_sides, 4, 3]
        and joint [n_sides - 1, 2, 3] (the attached vectors in the home section), side_axis [n_sides, 6] float32 (kappa_f,
        rate, un, ub, vn, vb) and side_kind."""
        m = WallMap._pose(pose)
        s = _lib.WallAlignmentLocateStart()
        st = self._L.gm_wall_alignment_locate_plan(*self._head(), _dptr(m), float(bound), C.byref(s))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_locate_plan refused the arguments")
        ns = int(s.add.n_sides)
        d = {k: np.array(getattr(s, k)[:], dtype=np.float64) for k in ("c", "d", "u", "v", "o_f", "a", "fu", "fv")}
        d.update(home=int(s.home), add=_alignment_add_info(s.add), s0=float(s.s0),
                 side=np.array([list(r) for r in s.side], dtype=np.float64)[:ns].reshape(ns, 4, 3),
                 joint=np.array([list(r) for r in s.joint], dtype=np.float64)[:max(ns - 1, 0)].reshape(max(ns - 1, 0), 2, 3),
                 side_axis=np.array([list(r) for r in s.side_axis], dtype=np.float32)[:ns],
                 side_kind=[int(x) for x in s.side_kind[:ns]])
        return d

    def align_plan(self, pose, bound, **params):
        """gm_wall_alignment_align_plan: the plan dict of an align under `pose` (_alignment_align_plan) with the align
        parameters given as keywords; GmError with GM_ERR_UNSUPPORTED for too many sides or pieces."""
        m = WallMap._pose(pose)
        p = _wall_align_params(**params)
        i = _lib.WallAlignmentAlignPlan()
        st = self._L.gm_wall_alignment_align_plan(*self._head(), _dptr(m), float(bound), C.byref(p), C.byref(i))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_align_plan refused the arguments")
        return _alignment_align_plan(i)

    def align_select(self, pose, bound, table, **params):
        """gm_wall_alignment_align_select: the info dict of the selection and the pose from a WALL_ALIGN_SCORE table; the
        device's counts are 0."""
        t = np.ascontiguousarray(np.asarray(table, dtype=WALL_ALIGN_SCORE).reshape(-1))
        m = WallMap._pose(pose)
        p = _wall_align_params(**params)
        info = _lib.WallAlignmentAlignInfo()
        st = self._L.gm_wall_alignment_align_select(*self._head(), _dptr(m), float(bound), C.byref(p),
                                                    t.ctypes.data_as(C.POINTER(_lib.WallAlignScore)), len(t), C.byref(info))
        if st != _lib.GM_OK:
            raise _lib.GmError(st, "gm_wall_alignment_align_select refused its arguments")
        return _alignment_align_info(info)


class WallAlignment(WallAlignmentRule, _FrameLoop):
    """One gm_wall_alignment: the element maps of an alignment of straights, arcs and clothoids, chained end to end, and
    the add of a frame to the elements it reaches in one launch.  Created by GeometricMapping.wall_alignment(); dies with
    its context.  The frame loop is _FrameLoop's: where a map returns its add info, the alignment returns its plan, and
    every per-point output gains element [n] int32, the point's owner."""

    _prefix, _EXTRA = "gm_wall_alignment_", _ELEMENT
    _Plan, _plan_info, _plan_key = _lib.WallAlignmentAddInfo, staticmethod(_alignment_add_info), "plan"
    _AlignPlan, _align_plan_info, _align_plan_key = _lib.WallAlignmentAlignPlan, staticmethod(_alignment_align_plan), "align_plan"
    _CheckInfo, _LocateInfo, _AlignInfo = _lib.WallAlignmentCheckInfo, _lib.WallAlignmentLocateInfo, _lib.WallAlignmentAlignInfo
    _align_dict = staticmethod(_alignment_align_info)

    def __init__(self, ctx, elements, **params):
        super().__init__(elements, **params)
        self._ctx, self._al = ctx, None
        h = C.c_void_p()
        ctx._check(self._L.gm_wall_alignment_create(ctx._ctx, *self._head(), C.byref(h)))
        self._al = h
        self._maps = {}
        self._object_calls.bind(_AlignmentObjects.DEVICE)
        self._region_calls.bind(_AlignmentRegions.DEVICE)

    def _h(self):
        if self._al is None or not self._ctx._ctx:
            raise ValueError("the wall alignment is closed (or its context is)")
        return self._al

    def close(self):
        if self._al is not None:
            for m in self._maps.values():
                m.close()
            self._maps = {}
            if self._ctx._ctx:
                self._L.gm_wall_alignment_destroy(self._al)
            self._al = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def element(self, i):
        """gm_wall_alignment_map: element i's WallMap (non-owning: the alignment keeps the map)."""
        i = int(i)
        if i not in self._maps:
            h = C.c_void_p()
            self._ctx._check(self._L.gm_wall_alignment_map(self._h(), i, C.byref(h)))
            self._maps[i] = WallMap._borrowed(self._ctx, h, self.element_params(i)[0])
        return self._maps[i]

    def info(self):
        """gm_wall_alignment_info: n_elements, n_stations, chainage_min, chainage_max and the summed frames and classes."""
        i = _lib.WallAlignmentTotals()
        self._ctx._check(self._L.gm_wall_alignment_info(self._h(), C.byref(i)))
        d = {k: int(getattr(i, k)) for k in ("n_elements", "n_stations", "frames", "mapped", "outside", "beyond_gate", "plane")}
        d.update(chainage_min=float(i.chainage_min), chainage_max=float(i.chainage_max))
        return d

    def add_plan(self, pose, bound=None):
        return super().add_plan(pose, float(self._ctx.cfg.boxFilterBound) if bound is None else bound)

    def locate_plan(self, pose, bound=None):
        return super().locate_plan(pose, float(self._ctx.cfg.boxFilterBound) if bound is None else bound)

    @staticmethod
    def _locate_info(i):
        """The dict of a gm_wall_alignment_locate_info: WallMap.locate_result()'s keys, element, n_sides, side_element,
        side_kind, side_anchor, side_axis [n_sides, 6] float32, and in every pass side [n_sides, 4, 3] and joint_o, joint_a
        [n_sides - 1, 3] float32: the blocks the pass's points saw."""
        d = WallMap._locate_info(i)
        ns = int(i.n_sides)
        d.update(element=int(i.element), n_sides=ns, side_element=[int(x) for x in i.side_element[:ns]],
                 side_kind=[int(x) for x in i.side_kind[:ns]], side_anchor=[int(x) for x in i.side_anchor[:ns]],
                 side_axis=np.array([list(r) for r in i.side_axis], dtype=np.float32)[:ns])
        for q, r in zip(d["pass"], i.pass_):
            q["side"] = np.array([list(x) for x in r.side], dtype=np.float32)[:ns].reshape(ns, 4, 3)
            q["joint_o"] = np.array([list(x) for x in r.joint_o], dtype=np.float32)[:max(ns - 1, 0)]
            q["joint_a"] = np.array([list(x) for x in r.joint_a], dtype=np.float32)[:max(ns - 1, 0)]
        return d

    def align_plan(self, pose, bound=None, **params):
        return super().align_plan(pose, float(self._ctx.cfg.boxFilterBound) if bound is None else bound, **params)

    def align_select(self, pose, table, bound=None, **params):
        return super().align_select(pose, float(self._ctx.cfg.boxFilterBound) if bound is None else bound, table, **params)

    def align_points(self, cloud, pose=np.eye(4)[:3], labels=None, outputs=True, **params):
        """gm_wall_alignment_align_points on a host cloud [n,3]: (info dict with the align's plan under "align_plan", table,
        dict(e float32, cell int32: jr * n_sectors + k of a binned point, else -1, element int32) or None without
        outputs)."""
        d, t, out = self._align_points(cloud, pose, labels, outputs, params)
        return d, t, out.dict()

    @staticmethod
    def split_cell(rows):
        """(side, cell) of WALL_CHECK_POINT rows of a check through the alignment: cell holds side << 24 | cell, side indexes
        the check plan's side_element, cell is relative to that element's map."""
        c = np.asarray(rows["cell"]).view(np.uint32)
        return (c >> np.uint32(24)).astype(np.int32), (c & np.uint32(0xFFFFFF)).astype(np.int32)

    @staticmethod
    def _check_info(i):
        """The dict of a gm_wall_alignment_check_info: WallMap.check_result()'s keys, n_sides and side_class
        [n_sides, 7] uint32 in GM_WALL_CHECK_CLS_* order."""
        d = WallMap._check_info(i)
        ns = int(i.n_sides)
        d.update(n_sides=ns, side_class=np.array([list(r) for r in i.side_class], dtype=np.uint32)[:ns])
        return d


def decode_compressed_map(buf):
    """Parse gm_get_compressed_map bytes (gm_map_header / gm_map_primitive in include/gm_hip.h)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    if bytes(buf[:4]) != b"GMAP":
        raise ValueError("not a GMAP record")
    version, nprim, nvox = np.frombuffer(buf, np.uint32, 3, 4)
    leaf, bound = np.frombuffer(buf, np.float32, 2, 16)
    n_points = int(np.frombuffer(buf, np.uint32, 1, 24)[0])
    ev = np.frombuffer(buf, np.float32, 3, 32).copy()
    axis = np.frombuffer(buf, np.float32, 3, 44).copy()
    off = 56
    prims = []
    for _ in range(int(nprim)):
        typ, inl = np.frombuffer(buf, np.uint32, 2, off)
        params = np.frombuffer(buf, np.float32, 7, off + 8).copy()
        prims.append(dict(type=int(typ), inliers=int(inl), params=params))
        off += 40
    vox = np.frombuffer(buf, np.float32, 4 * int(nvox), off).reshape(-1, 4).copy()
    return dict(version=int(version), leaf=float(leaf), bound=float(bound), n_points=n_points, eigenvalues=ev,
                center_axis=axis, primitives=prims, voxels=vox)


class GeometricMappingGroup:
    """gm_group: one host thread driving every listed GPU; ONE frame sharded spatially across them with an in-library
    RCCL all-gather of the per-rank records (include/gm_hip.h, "multi-device group").  devices=[0, 0, ...] with
    loopback=True runs several ranks on one GPU (tests on a 1-GPU box): same code, records travel by device copies."""

    def __init__(self, devices, loopback=False, **cfg_kw):
        if not loopback:
            # the group loads RCCL (the copy PyTorch bundles when PyTorch is installed: _lib.py).  Observed on ROCm 7.2 /
            # torch 2.10: a process that initialises RCCL first and imports torch afterwards aborts at interpreter exit
            # ("double free or corruption"); the other order is clean.  So torch, if present, goes first.
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        self._L = _lib.load()
        cfg = Config()
        self._L.gm_default_config(C.byref(cfg))
        for k, v in cfg_kw.items():
            setattr(cfg, k, v)
        dev = (C.c_int32 * len(devices))(*devices)
        self._grp = C.c_void_p()
        st = self._L.gm_group_create(C.byref(cfg), dev, len(devices), _lib.GM_GROUP_LOOPBACK if loopback else 0, C.byref(self._grp))
        if st != GM_OK:
            msg = self._L.gm_group_last_error(None).decode()
            self._grp = None
            raise GmError(st, msg)

    def close(self):
        if getattr(self, "_grp", None):
            self._L.gm_group_destroy(self._grp)
            self._grp = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._L.gm_group_size(self._grp))

    def _check(self, st):
        if st != GM_OK:
            raise GmError(st, self._L.gm_group_last_error(self._grp).decode())

    def process_frame(self, cloud):
        c, keep = cloud if (isinstance(cloud, tuple) and isinstance(cloud[0], Cloud)) else GeometricMapping._cloud_from_xyz(cloud)
        res = FrameResult()
        self._check(self._L.gm_group_process_frame(self._grp, C.byref(c), C.byref(res)))
        return GeometricMapping._result(res)

    def _fetch(self, fn, width, dtype=np.float32):
        n = C.c_uint32(0)
        st = fn(self._grp, None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            self._check(st)
        out = np.empty((n.value, width) if width > 1 else (n.value,), dtype=dtype)
        if n.value:
            self._check(fn(self._grp, out.ctypes.data_as(fn.argtypes[1]), n.value, C.byref(n)))
        return out

    def cropped_cloud(self):
        """/choppedCloud of the sharded frame in the single-GPU order: (xyz [n,3], input row index [n])."""
        out = self._fetch(self._L.gm_group_get_cropped_xyz, 4)
        return out[:, :3].copy(), out[:, 3].copy().view(np.int32)

    def voxel_centroids(self):
        """(centroids [V,3], points per voxel [V]) of the sharded frame, ascending voxel-key order."""
        a = self._fetch(self._L.gm_group_get_voxel_centroids, 4)
        return a[:, :3].copy(), a[:, 3].astype(np.int32)

    def voxel_normals(self):
        """normals->at(kIndices[0]) per voxel centroid of the sharded frame: [V,4] (GM_CFG_NEAREST)."""
        return self._fetch(self._L.gm_group_get_voxel_normals, 4)

    def voxel_nearest(self):
        """Index (into cropped_cloud()) of the nearest valid point of every voxel centroid (GM_CFG_NEAREST)."""
        return self._fetch(self._L.gm_group_get_voxel_nearest, 1, np.int32)

    def labels(self):
        """Labels of the sharded frame, one per row of cropped_cloud() (uint8: 1 plane, 2 cylinder, 0 other)."""
        return self._fetch(self._L.gm_group_get_labels, 1, np.uint8)

    def fit_cylinder(self, init7=None):
        """Least-squares cylinder of the sharded frame over every rank's resident cloud (gm_group_fit_cylinder), started
        from init7 (point, direction, radius) or, when None, from the frame's published cylinder.  Relabels the frame:
        labels() afterwards are the published plane's (1) and the fit's (2).  Returns the dict of
        GeometricMapping.cylinder_fit."""
        init = None
        if init7 is not None:
            init = np.ascontiguousarray(np.asarray(init7, dtype=np.float32).reshape(7))
        f = CylinderFit()
        self._check(self._L.gm_group_fit_cylinder(self._grp, _f32(init) if init is not None else None, C.byref(f)))
        return GeometricMapping._fit(f)

    def last_cylinder_fit(self):
        """The last fit_cylinder result of the current sharded frame (gm_group_get_cylinder_fit)."""
        f = CylinderFit()
        st = self._L.gm_group_get_cylinder_fit(self._grp, C.byref(f))
        if st != GM_OK:
            raise GmError(st, "gm_group_get_cylinder_fit: no fit of the current sharded frame")
        return GeometricMapping._fit(f)

    def timing(self):
        """Wall-clock split of the last process_frame call, milliseconds."""
        t = (C.c_double * _lib.GM_GROUP_N_TIMINGS)()
        self._check(self._L.gm_group_get_timing(self._grp, t, _lib.GM_GROUP_N_TIMINGS))
        return dict(zip(("cut_ms", "submit_ms", "device_ms", "merge_ms", "total_ms"), (float(x) for x in t)))

    def edges(self):
        """(slab edges [n_ranks + 1], whether they lie on planes of the VoxelGrid lattice)."""
        e = (C.c_double * (len(self) + 1))()
        on = C.c_uint32(0)
        self._check(self._L.gm_group_get_edges(self._grp, e, len(self) + 1, C.byref(on)))
        return np.array(e[:]), bool(on.value)

    # ---- streaming: whole frames round-robin over the devices
    def submit_frame(self, cloud):
        c, keep = cloud if (isinstance(cloud, tuple) and isinstance(cloud[0], Cloud)) else GeometricMapping._cloud_from_xyz(cloud)
        self._check(self._L.gm_group_submit_frame(self._grp, C.byref(c)))

    def wait_frame(self):
        """The oldest frame in flight: (result, rank, slot)."""
        res = FrameResult()
        rank, slot = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.gm_group_wait_frame(self._grp, C.byref(res), C.byref(rank), C.byref(slot)))
        return GeometricMapping._result(res), int(rank.value), int(slot.value)

    def in_flight(self):
        return int(self._L.gm_group_in_flight(self._grp))

    def poll_frame(self):
        """True when the oldest frame in flight has finished (wait_frame returns at once); never blocks."""
        st = self._L.gm_group_poll_frame(self._grp)
        if st == GM_OK:
            return True
        if st == GM_ERR_NOT_READY:
            return False
        self._check(st)

    def cylinder_fit(self, rank, slot):
        """The cylinder regression of a streamed frame (GM_CFG_CYLINDER_FIT): gm_get_cylinder_fit on the rank's context."""
        ctx = self._L.gm_group_ctx(self._grp, rank)
        f = CylinderFit()
        st = self._L.gm_get_cylinder_fit(ctx, slot, C.byref(f))
        if st != GM_OK:
            raise GmError(st, self._L.gm_last_error(ctx).decode())
        return GeometricMapping._fit(f)

    def rank_fetch(self, rank, slot, what):
        """Bulky output of a streamed frame: what in {"cropped_xyz", "normals", "voxel_centroids"} -> float32 [n,4];
        "neighbor_counts" (GM_CFG_KEEP_COUNTS) -> int32 [n_cropped], one per row that passed the rank's crop, in the order
        the rows were sent (gm_get_neighbor_counts).  After process_frame, slot 0 of every rank holds that rank's slab of
        the sharded frame: the rows it was sent (its own and its halo), of which only the rows it owns are valid."""
        fn = getattr(self._L, "gm_get_" + what)
        ctx = self._L.gm_group_ctx(self._grp, rank)
        n = C.c_uint32(0)
        st = fn(ctx, slot, None, 0, C.byref(n))
        if st not in (GM_OK, GM_ERR_CAPACITY):
            raise GmError(st, self._L.gm_last_error(ctx).decode())
        counts = what == "neighbor_counts"
        out = np.empty((n.value,) if counts else (n.value, 4), dtype=np.int32 if counts else np.float32)
        if n.value:
            st = fn(ctx, slot, out.ctypes.data_as(fn.argtypes[2]), n.value, C.byref(n))
            if st != GM_OK:
                raise GmError(st, self._L.gm_last_error(ctx).decode())
        return out


def solve_local_frame(scatter6):
    """Eigen-solve a merged scatter matrix (multi-GPU merge unit)."""
    L = _lib.load()
    sc = np.ascontiguousarray(scatter6, dtype=np.float64)
    ev = np.zeros(3, dtype=np.float32)
    V = np.zeros(9, dtype=np.float32)
    st = L.gm_solve_local_frame(sc.ctypes.data_as(C.POINTER(C.c_double)), _f32(ev), _f32(V))
    if st != GM_OK:
        raise GmError(st, "gm_solve_local_frame")
    return ev, V.reshape(3, 3).T.copy()
