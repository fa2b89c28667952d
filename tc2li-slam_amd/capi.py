"""ctypes binding of include/tc2li_hip.h and thin classes that mirror the reference's C++ interface
(``ORBextractor`` -> :class:`OrbExtractor`).  Mirrors names, argument meaning and error behaviour of
SF/include/ORBextractor.h:46-121 so that the parity tests read like tests of the reference class."""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtc2li_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tc2li_hip.h")

_lib = None


class Tc2liError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("tc2li error %d: %s" % (code, text))
        self.code = code


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4")])


def lib():
    """Loads libtc2li_hip.so (built in-tree by ``__graft_entry__.build()``); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.  Importing torch first makes the
    # dynamic loader satisfy our DT_NEEDED libamdhip64.so.7 with that already-loaded copy, so device pointers and
    # streams can be shared with torch.  Without torch the system runtime under /opt/rocm is used.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional plumbing
        pass
    if not os.path.exists(LIB_PATH):
        raise Tc2liError(-3, "native library %s not built (run __graft_entry__.build()); there is no fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.tc2li_last_error.restype = C.c_char_p
    L.tc2li_orb_create.argtypes = [C.POINTER(OrbParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.tc2li_orb_destroy.argtypes = [C.c_void_p]
    L.tc2li_orb_destroy.restype = None
    L.tc2li_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p,
                                    C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.tc2li_orb_extract_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                          C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.tc2li_orb_levels.argtypes = [C.c_void_p]
    L.tc2li_orb_scale_factors.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.tc2li_orb_features_per_level.argtypes = [C.c_void_p, C.c_void_p]
    L.tc2li_orb_level_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tc2li_orb_download_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.tc2li_orb_download_blurred.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.tc2li_orb_download_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.tc2li_orb_last_timings.argtypes = [C.c_void_p, C.c_void_p]
    L.tc2li_orb_last_chunks.argtypes = [C.c_void_p]
    L.tc2li_orb_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.tc2li_host_distribute_quadtree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_int]
    L.tc2li_device_distribute_quadtree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.tc2li_stereo_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_stereo_match_batch.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p]
    L.tc2li_lidar_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.tc2li_lidar_destroy.argtypes = [C.c_void_p]
    L.tc2li_lidar_destroy.restype = None
    L.tc2li_lidar_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_void_p, C.c_int]
    L.tc2li_lidar_voxel_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    L.tc2li_lidar_set_preprocess_features.argtypes = [C.c_void_p, C.c_void_p]
    L.tc2li_lidar_corner_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.tc2li_lidar_point_labels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_lidar_map_create.argtypes = [C.POINTER(C.c_void_p)]
    L.tc2li_lidar_map_destroy.argtypes = [C.c_void_p]
    L.tc2li_lidar_map_destroy.restype = None
    L.tc2li_lidar_map_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_lidar_map_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_lidar_map_size.argtypes = [C.c_void_p]
    L.tc2li_lidar_feature_extraction.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 8 + [C.c_int]
    L.tc2li_lidar_frontend_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p]
    L.tc2li_pose_optimization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.tc2li_pose_optimization_batch.argtypes = [C.c_int] + [C.c_void_p] * 8
    L.tc2li_local_bundle_adjustment.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_local_lv_bundle_adjustment.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                   C.c_int, C.c_double] + [C.c_void_p] * 7
    L.tc2li_local_lv_bundle_adjustment_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                           C.c_int, C.c_double] + [C.c_void_p] * 8
    L.tc2li_ba_shard_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.tc2li_rccl_unique_id.argtypes = [C.c_void_p]
    L.tc2li_rccl_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.tc2li_rccl_comm_destroy.argtypes = [C.c_void_p]
    L.tc2li_rccl_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.tc2li_local_map_create.argtypes = [C.POINTER(C.c_void_p)]
    L.tc2li_local_map_destroy.argtypes = [C.c_void_p]
    L.tc2li_local_map_destroy.restype = None
    L.tc2li_local_map_set_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_local_map_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_local_map_device_points.argtypes = [C.c_void_p]
    L.tc2li_local_map_device_points.restype = C.c_void_p
    L.tc2li_lidar_window_evaluate.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.tc2li_track_motion_model_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_float, C.c_float] + [C.c_void_p] * 5
    L.tc2li_local_bundle_adjustment_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_local_bundle_adjustment_batch_group.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_ba_engine_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.tc2li_ba_engine_destroy.argtypes = [C.c_void_p]
    L.tc2li_ba_engine_destroy.restype = None
    L.tc2li_ba_engine_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_ba_engine_submit.restype = C.c_int64
    L.tc2li_ba_engine_wait.argtypes = [C.c_void_p, C.c_int64]
    L.tc2li_ba_engine_poll.argtypes = [C.c_void_p, C.c_int64]
    L.tc2li_lidar_last_timings.argtypes = [C.c_void_p, C.c_void_p]
    L.tc2li_imu_preintegrated_init.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]
    L.tc2li_imu_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    L.tc2li_imu_preintegrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double]
    L.tc2li_imu_delta.argtypes = [C.c_void_p] * 5
    L.tc2li_imu_predict_state.argtypes = [C.c_void_p] * 8
    L.tc2li_lidar_undistort.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_lidar_imu_propagate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_lidar_map_incremental.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_lidar_map_delete_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_lidar_map_delete_boxes_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc2li_lidar_map_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_lidar_fov_segment.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    L.tc2li_lidar_fov_segment_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.tc2li_local_inertial_bundle_adjustment.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 5
    L.tc2li_host_lidar_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tc2li_device_lidar_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.tc2li_search_by_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    L.tc2li_project_last_frame.argtypes = [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_void_p]
    L.tc2li_project_local_map.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.tc2li_device_time_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise Tc2liError(rc, lib().tc2li_last_error().decode("utf-8", "replace"))
    return rc


def abi_version():
    return lib().tc2li_abi_version()


def device_count():
    return lib().tc2li_device_count()


def set_hardware_queues(n):
    """tc2li_set_hardware_queues: only effective before the process's first HIP call."""
    _check(lib().tc2li_set_hardware_queues(int(n)))


def lib_loaded():
    return _lib is not None


def shutdown():
    """tc2li_shutdown: joins the library's worker pools and releases its process-wide work spaces; no other thread may be inside the
    library.  Handles stay valid, the next call that needs a pool makes it again."""
    _check(lib().tc2li_shutdown())


def set_host_thread_budget(threads):
    """tc2li_set_host_thread_budget: host threads this process may keep busy (cores / ranks per node); before the pools exist."""
    _check(lib().tc2li_set_host_thread_budget(int(threads)))


def host_threads():
    """{budget, extractor_pool, tracking_pool, lidar_pool, ba_group_pool, ba_groups_max}: the sizes the pools have (or will get)."""
    out = (C.c_int32 * 6)()
    _check(lib().tc2li_host_threads(out, 6))
    return dict(zip(("budget", "extractor_pool", "tracking_pool", "lidar_pool", "ba_group_pool", "ba_groups_max"), [int(v) for v in out]))


def exported_symbols():
    """Names of the functions include/tc2li_hip.h declares (used by the CPU-side ABI test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tc2li_[a-z0-9_]+)\s*\(", text)))


def diag_clocks():
    """(GHz inside the f64 MFMA loop, GHz inside the f64 FMA loop) of tc2li_diag_peaks' kernels."""
    a, b = C.c_double(0), C.c_double(0)
    _check(lib().tc2li_diag_clocks(C.byref(a), C.byref(b)))
    return a.value, b.value


def profile_enable(on=True):
    _check(lib().tc2li_profile_enable(int(bool(on))))


def ba_options():
    """tc2li_ba_options -> dict of the bundle-adjustment switches in effect."""
    import json
    f = lib().tc2li_ba_options
    f.argtypes = [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(512)
    f(buf, len(buf))
    return json.loads(buf.value.decode())


def profile_report():
    """{kernel name: (launches, total ms)} of the launches since the last report (call with idle streams)."""
    f = lib().tc2li_profile_report
    f.argtypes = [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 18)
    f(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split("\t")
        name = name.strip("() ").replace(" ", "")
        c0, m0 = out.get(name, (0, 0.0))
        out[name] = (c0 + int(calls), m0 + float(ms))
    return out


def diag_peaks():
    """(f64 MFMA TFLOP/s, f64 vector FMA TFLOP/s, HBM copy GB/s) measured on the current device."""
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    f = lib().tc2li_diag_peaks
    f.argtypes = [C.c_void_p] * 3
    _check(f(C.addressof(a), C.addressof(b), C.addressof(c)))
    return a.value, b.value, c.value


def distribute_quadtree_host(xyr, min_x, max_x, min_y, max_y, n_target):
    xyr = np.ascontiguousarray(xyr, dtype=np.float32).reshape(-1, 3)
    out = np.empty((max(len(xyr), 1), 3), np.float32)
    n = _check(lib().tc2li_host_distribute_quadtree(xyr.ctypes.data, len(xyr), min_x, max_x, min_y, max_y, n_target,
                                                    out.ctypes.data, len(out)))
    return out[:n].copy()


def distribute_quadtree_device(xyr, min_x, max_x, min_y, max_y, n_target, threads=0):
    """One job of the extractor's keypoint-distribution kernel (k_quadtree) on the given candidates."""
    xyr = np.ascontiguousarray(xyr, dtype=np.float32).reshape(-1, 3)
    out = np.empty((max(len(xyr), n_target + 16, 1), 3), np.float32)
    n = _check(lib().tc2li_device_distribute_quadtree(xyr.ctypes.data, len(xyr), min_x, max_x, min_y, max_y, n_target, out.ctypes.data, len(out),
                                                      threads))
    return out[:n].copy()


class OrbExtractor:
    """Mirror of ``TC2LI_SLAM::ORBextractor`` (SF/include/ORBextractor.h:46).

    ``extract(image)`` is ``operator()``: returns ``(monoIndex, keypoints, descriptors)``; an empty image gives
    ``(-1, [], [])`` like the reference (SF/src/ORBextractor.cc:1063-1064).
    """

    def __init__(self, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th_fast=20, min_th_fast=7,
                 max_width=1242, max_height=376, max_images=2):
        self._h = C.c_void_p()
        self.params = OrbParams(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast)
        self.capacity = nfeatures + 4 * nlevels
        self.max_images = max_images
        _check(lib().tc2li_orb_create(C.byref(self.params), max_width, max_height, max_images, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().tc2li_orb_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    # ---- accessors (ORBextractor.h:70-90) ----
    def GetLevels(self):
        return lib().tc2li_orb_levels(self._h)

    def _scales(self):
        n = self.GetLevels()
        arrs = [np.empty(n, np.float32) for _ in range(4)]
        _check(lib().tc2li_orb_scale_factors(self._h, *[a.ctypes.data for a in arrs]))
        return arrs

    def GetScaleFactors(self):
        return self._scales()[0]

    def GetInverseScaleFactors(self):
        return self._scales()[1]

    def GetScaleSigmaSquares(self):
        return self._scales()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._scales()[3]

    def features_per_level(self):
        a = np.empty(self.GetLevels(), np.int32)
        _check(lib().tc2li_orb_features_per_level(self._h, a.ctypes.data))
        return a

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _check(lib().tc2li_orb_level_size(self._h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    # ---- operator() ----
    def extract(self, image, lapping_area=(0, 0)):
        image = np.asarray(image)
        kps = np.zeros(self.capacity, KEYPOINT_DTYPE)
        desc = np.zeros((self.capacity, 32), np.uint8)
        n = C.c_int32(0)
        lap = (C.c_int32 * 2)(*lapping_area)
        if image.size == 0:
            rc = lib().tc2li_orb_extract(self._h, None, 0, 0, 0, lap, kps.ctypes.data, desc.ctypes.data, self.capacity,
                                         C.byref(n))
            return rc, kps[:0], desc[:0]
        assert image.dtype == np.uint8 and image.ndim == 2
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        rc = lib().tc2li_orb_extract(self._h, image.ctypes.data, image.shape[1], image.shape[0], image.strides[0], lap,
                                     kps.ctypes.data, desc.ctypes.data, self.capacity, C.byref(n))
        _check(rc)
        return rc, kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch_dev(self, dev_ptr, n_images, width, height, stride, image_pitch, stream=0, lapping_area=(0, 0),
                          out=None):
        """Images resident in device memory (``dev_ptr`` = integer device address). Returns per-image arrays."""
        if out is None:
            out = (np.zeros((n_images, self.capacity), KEYPOINT_DTYPE), np.zeros((n_images, self.capacity, 32), np.uint8),
                   np.zeros(n_images, np.int32), np.zeros(n_images, np.int32))
        kps, desc, counts, mono = out
        lap = (C.c_int32 * 2)(*lapping_area)
        _check(lib().tc2li_orb_extract_batch(self._h, C.c_void_p(dev_ptr), n_images, width, height, stride, image_pitch,
                                             lap, kps.ctypes.data, desc.ctypes.data, self.capacity, counts.ctypes.data,
                                             mono.ctypes.data, C.c_void_p(stream)))
        return kps, desc, counts, mono

    # ---- mvImagePyramid and diagnostics ----
    def pyramid_level(self, image_index, level):
        w, h = self.level_size(level)
        out = np.empty((h, w), np.uint8)
        _check(lib().tc2li_orb_download_level(self._h, image_index, level, out.ctypes.data))
        return out

    def blurred_level(self, image_index, level):
        w, h = self.level_size(level)
        out = np.empty((h, w), np.uint8)
        _check(lib().tc2li_orb_download_blurred(self._h, image_index, level, out.ctypes.data))
        return out

    def candidates(self, image_index, level):
        n = _check(lib().tc2li_orb_download_candidates(self._h, image_index, level, None, 0))
        out = np.empty((max(n, 1), 3), np.float32)
        n = _check(lib().tc2li_orb_download_candidates(self._h, image_index, level, out.ctypes.data, len(out)))
        return out[:n]

    def set_profiling(self, enabled):
        _check(lib().tc2li_orb_set_profiling(self._h, int(enabled)))

    def last_timings(self):
        t = np.zeros(8, np.float32)
        _check(lib().tc2li_orb_last_timings(self._h, t.ctypes.data))
        return t

    def last_chunks(self):
        """Chunks of images the last batch call was pipelined over (every device stage is launched once per chunk)."""
        return _check(lib().tc2li_orb_last_chunks(self._h))

    def match_grid_builds(self):
        """Feature-grid builds of the handle so far: one per extraction that a projection search followed (tc2li_orb_match_grid_builds)."""
        f = lib().tc2li_orb_match_grid_builds
        f.argtypes = [C.c_void_p]
        return _check(f(self._h))


def compute_stereo_matches(ext_left, ext_right, kps_l, desc_l, kps_r, desc_r, bf, b):
    """``Frame::ComputeStereoMatches`` (SF/src/Frame.cc:841): returns (mvuRight, mvDepth, bestSAD)."""
    kps_l = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE)
    kps_r = np.ascontiguousarray(kps_r, KEYPOINT_DTYPE)
    desc_l = np.ascontiguousarray(desc_l, np.uint8)
    desc_r = np.ascontiguousarray(desc_r, np.uint8)
    n = len(kps_l)
    u = np.full(max(n, 1), -1, np.float32)
    d = np.full(max(n, 1), -1, np.float32)
    s = np.full(max(n, 1), -1, np.int32)
    _check(lib().tc2li_stereo_match(ext_left._h, ext_right._h, kps_l.ctypes.data, desc_l.ctypes.data, n, kps_r.ctypes.data,
                                    desc_r.ctypes.data, len(kps_r), bf, b, u.ctypes.data, d.ctypes.data, s.ctypes.data))
    return u[:n], d[:n], s[:n]


def stereo_match_batch(ext, n_frames, bf, b, stream=0, out=None):
    """Batched stereo matching on the device-resident features of the preceding ``extract_batch_dev`` call."""
    if out is None:
        out = (np.full((n_frames, ext.capacity), -1, np.float32), np.full((n_frames, ext.capacity), -1, np.float32),
               np.full((n_frames, ext.capacity), -1, np.int32))
    u, d, s = out
    _check(lib().tc2li_stereo_match_batch(ext._h, n_frames, bf, b, u.ctypes.data, d.ctypes.data, s.ctypes.data, ext.capacity,
                                          C.c_void_p(stream)))
    return u, d, s


# ---- LiDAR front end ---------------------------------------------------------------------------------------------
VELODYNE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("intensity", "<f4"),
                           ("time", "<f4"), ("ring", "<u2"), ("pad1", "<u2"), ("pad2", "<f4")])
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("normal_x", "<f4"),
                        ("normal_y", "<f4"), ("normal_z", "<f4"), ("pad1", "<f4"), ("intensity", "<f4"),
                        ("curvature", "<f4"), ("pad2", "<f4"), ("pad3", "<f4")])


def pack_lidar_state(rot, pos, offset_r=None, offset_t=None):
    """tc2li_lidar_state as 24 float64 (rot row-major, pos, offset_R_L_I row-major, offset_T_L_I)."""
    offset_r = np.eye(3) if offset_r is None else offset_r
    offset_t = np.zeros(3) if offset_t is None else offset_t
    return np.ascontiguousarray(np.concatenate([np.ravel(rot), np.ravel(pos), np.ravel(offset_r), np.ravel(offset_t)]), np.float64)


class LidarMap:
    """The incremental LiDAR map (global ``ikdtree`` of LidarFrontEnd.cpp:96): Build / Add_Points / size."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().tc2li_lidar_map_create(C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().tc2li_lidar_map_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def Build(self, points):
        points = np.ascontiguousarray(points, POINT_DTYPE)
        return _check(lib().tc2li_lidar_map_build(self._h, points.ctypes.data, len(points)))

    def Add_Points(self, points):
        points = np.ascontiguousarray(points, POINT_DTYPE)
        return _check(lib().tc2li_lidar_map_add(self._h, points.ctypes.data, len(points)))

    def size(self):
        return _check(lib().tc2li_lidar_map_size(self._h))

    def points(self):
        n = self.size()
        out = np.zeros(max(n, 1), POINT_DTYPE)
        _check(lib().tc2li_lidar_map_download(self._h, out.ctypes.data, len(out)))
        return out[:n].copy()

    def stats(self):
        """tc2li_lidar_map_stats -> dict(points, slots, grid_builds, grid_updates, tombstones, cells)."""
        out = (C.c_int32 * 6)()
        f = lib().tc2li_lidar_map_stats
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _check(f(self._h, out, 6))
        return dict(zip(("points", "slots", "grid_builds", "grid_updates", "tombstones", "cells"), [int(v) for v in out]))

    def grid(self):
        """tc2li_lidar_map_grid_download: the grid walked and checked on the host -> (cells [n], point indices [n]) of its live entries."""
        n = self.size()
        cells, idx = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        f = lib().tc2li_lidar_map_grid_download
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        live = _check(f(self._h, cells.ctypes.data, idx.ctypes.data, len(cells)))
        if live != n:
            raise Tc2liError(-2, "the grid holds %d live entries for %d points" % (live, n))
        return cells[:n].copy(), idx[:n].copy()

    def Delete_Point_Boxes(self, boxes6, stream=0):
        """boxes6: [n, 6] = min x y z, max x y z; returns the number of removed points."""
        b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
        return _check(lib().tc2li_lidar_map_delete_boxes(self._h, b.ctypes.data, len(b), C.c_void_p(stream)))

    def map_incremental(self, front_end, scan, state24, ekf_inited=True, filter_size_map_min=0.5, stream=0):
        """``map_incremental()`` for scan slot ``scan`` of ``front_end``'s last feature extraction against this map ->
        (map size, n_to_add, n_no_need)."""
        st = np.ascontiguousarray(state24, np.float64)
        na, nn = C.c_int32(0), C.c_int32(0)
        n = _check(lib().tc2li_lidar_map_incremental(front_end._h, scan, self._h, st.ctypes.data, int(ekf_inited), filter_size_map_min,
                                                     C.addressof(na), C.addressof(nn), C.c_void_p(stream)))
        return n, na.value, nn.value


def delete_point_boxes_batch(maps, boxes_per_map, stream=0):
    """``Delete_Point_Boxes`` on several maps at once: ``boxes_per_map[i]`` = [k_i, 6] boxes of map i -> removed points per map."""
    n = len(maps)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(np.asarray(b).reshape(-1, 6)) for b in boxes_per_map])
    allb = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(-1, 6) for b in boxes_per_map] + [np.zeros((0, 6), np.float32)]), np.float32)
    handles = (C.c_void_p * max(n, 1))(*[m._h for m in maps])
    removed = np.zeros(max(n, 1), np.int32)
    _check(lib().tc2li_lidar_map_delete_boxes_batch(n, handles, allb.ctypes.data, offs.ctypes.data, removed.ctypes.data, C.c_void_p(stream)))
    return removed[:n]


def map_incremental_batch(front_end, scans, maps, states24, ekf_inited=True, filter_size_map_min=0.5, stream=0):
    """``tc2li_lidar_map_incremental_batch`` -> (n_to_add [n], n_no_need [n], map sizes [n])."""
    n = len(maps)
    sc = np.ascontiguousarray(scans, np.int32)
    st = np.ascontiguousarray(states24, np.float64).reshape(n, 24)
    handles = (C.c_void_p * n)(*[m._h for m in maps])
    na, nn, sz = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    f = lib().tc2li_lidar_map_incremental_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(front_end._h, n, sc.ctypes.data, handles, st.ctypes.data, int(ekf_inited), filter_size_map_min, na.ctypes.data, nn.ctypes.data,
             sz.ctypes.data, C.c_void_p(stream)))
    return na, nn, sz


# ---- pose plumbing between the camera thread and the LiDAR front end (row b4) ----
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def lidar_update_pose(Tcw_last7, velocity7, time_from_last_frame, Tcl7, state24):
    """``UpdateLidarPose`` -> (state24 with rot / pos replaced, pos_lid)."""
    st, pos = np.ascontiguousarray(state24, np.float64).copy(), np.zeros(3)
    f = lib().tc2li_lidar_update_pose
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(_f32(Tcw_last7).ctypes.data, _f32(velocity7).ctypes.data, time_from_last_frame, _f32(Tcl7).ctypes.data, st.ctypes.data, pos.ctypes.data))
    return st, pos


def se3_interpolate(a7, b7, t):
    out = np.zeros(7, np.float32)
    f = lib().tc2li_se3_interpolate
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    _check(f(_f32(a7).ctypes.data, _f32(b7).ctypes.data, t, out.ctypes.data))
    return out


def lidar_sync_transform(Tcw_frame7, Tcw_last7, Tcw_cur7, ratio, Tlc7, Tcl7):
    out = np.zeros(7, np.float32)
    f = lib().tc2li_lidar_sync_transform
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(_f32(Tcw_frame7).ctypes.data, _f32(Tcw_last7).ctypes.data, _f32(Tcw_cur7).ctypes.data, ratio, _f32(Tlc7).ctypes.data, _f32(Tcl7).ctypes.data,
             out.ctypes.data))
    return out


def lidar_keyframe_transform(Tcw_cur7, rel7, Tcw_refkf7, Tlc7, Tcl7):
    out = np.zeros(7, np.float32)
    f = lib().tc2li_lidar_keyframe_transform
    f.argtypes = [C.c_void_p] * 6
    _check(f(_f32(Tcw_cur7).ctypes.data, _f32(rel7).ctypes.data, _f32(Tcw_refkf7).ctypes.data, _f32(Tlc7).ctypes.data, _f32(Tcl7).ctypes.data, out.ctypes.data))
    return out


def transform_point_cloud(points, T7, stream=0):
    p = np.ascontiguousarray(points, POINT_DTYPE)
    out = np.zeros(len(p), POINT_DTYPE)
    f = lib().tc2li_transform_point_cloud
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(p.ctypes.data if len(p) else None, len(p), _f32(T7).ctypes.data, out.ctypes.data if len(p) else None, C.c_void_p(stream)))
    return out


def lidar_transform_features_batch(front_end, scans, T7, capacity=None, stream=0):
    """The selected feature clouds of scan slots ``scans`` of the last ``frontend_batch``, each moved by T7[i] -> list of POINT_DTYPE arrays."""
    sc = np.ascontiguousarray(scans, np.int32)
    T = _f32(T7).reshape(len(sc), 7)
    capacity = capacity or front_end.cap
    out = np.zeros((len(sc), capacity), POINT_DTYPE)
    npts = np.zeros(len(sc), np.int32)
    f = lib().tc2li_lidar_transform_features_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _check(f(front_end._h, len(sc), sc.ctypes.data, T.ctypes.data, out.ctypes.data, capacity, npts.ctypes.data, C.c_void_p(stream)))
    return [out[i, :npts[i]].copy() for i in range(len(sc))]


class LocalMapBox(C.Structure):
    _fields_ = [("vertex_min", C.c_float * 3), ("vertex_max", C.c_float * 3), ("initialized", C.c_int32)]


def lidar_fov_segment(local_map, pos_lid, cube_len=200.0, det_range=100.0):
    """``lasermap_fov_segment`` (host): updates ``local_map`` (a LocalMapBox) and returns the boxes [k, 6] to delete."""
    pos = np.ascontiguousarray(pos_lid, np.float64)
    boxes = np.zeros((3, 6), np.float32)
    k = _check(lib().tc2li_lidar_fov_segment(C.addressof(local_map), pos.ctypes.data, cube_len, det_range, boxes.ctypes.data))
    return boxes[:k].copy()


def host_reduced_solve(Hi, S, lam, rhs):
    """``tc2li_host_reduced_solve``: the host's envelope LDL^T of an inertial window's reduced system (no GPU) -> x, or None when a pivot fails."""
    Hi = np.ascontiguousarray(Hi, np.float64)
    S = np.ascontiguousarray(S, np.float64)
    rhs = np.ascontiguousarray(rhs, np.float64)
    n, npose = len(Hi), len(S)
    x = np.zeros(n)
    f = lib().tc2li_host_reduced_solve
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    ok = _check(f(Hi.ctypes.data, S.ctypes.data if npose else None, n, npose, float(lam), rhs.ctypes.data, x.ctypes.data))
    return x if ok else None


def host_fast_forms(v, p, th):
    """``tc2li_host_fast_forms``: the FAST kernel's per-pixel forms (csrc/fast_forms.hpp) on the host, for centres ``v`` [n] and circles
    ``p`` [n, 16] -> dict of pretest, mask_bright, mask_dark, polarity, score_dark, score_bright (arrays of n)."""
    v = np.ascontiguousarray(v, np.uint8).reshape(-1)
    p = np.ascontiguousarray(p, np.uint8).reshape(len(v), 16)
    out = {"pretest": np.zeros(len(v), np.uint8), "mask_bright": np.zeros(len(v), np.uint16), "mask_dark": np.zeros(len(v), np.uint16),
           "polarity": np.zeros(len(v), np.uint8), "score_dark": np.zeros(len(v), np.int16), "score_bright": np.zeros(len(v), np.int16)}
    f = lib().tc2li_host_fast_forms
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    _check(f(v.ctypes.data, p.ctypes.data, len(v), int(th), *[a.ctypes.data for a in out.values()]))
    return out


def device_reduced_solve(Hi, S, lam, rhs, stream=0):
    """``tc2li_device_reduced_solve``: the same system through k_lvi_solve -> x, or None when a pivot fails."""
    Hi = np.ascontiguousarray(Hi, np.float64)
    S = np.ascontiguousarray(S, np.float64)
    rhs = np.ascontiguousarray(rhs, np.float64)
    n, npose = len(Hi), len(S)
    x = np.zeros(n)
    f = lib().tc2li_device_reduced_solve
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    ok = _check(f(Hi.ctypes.data, S.ctypes.data, n, npose, float(lam), rhs.ctypes.data, x.ctypes.data, C.c_void_p(stream)))
    return x if ok else None


def lidar_fov_segment_batch(local_maps, pos_lid3, cube_len=200.0, det_range=100.0):
    """``lasermap_fov_segment`` for n sensors in one call: ``local_maps`` a ctypes array ``(LocalMapBox * n)()``, ``pos_lid3`` [n, 3]
    -> (boxes [n, 3, 6] float32, counts [n] int32)."""
    n = len(local_maps)
    pos = np.ascontiguousarray(pos_lid3, np.float64).reshape(n, 3)
    boxes = np.zeros((n, 3, 6), np.float32)
    counts = np.zeros(n, np.int32)
    _check(lib().tc2li_lidar_fov_segment_batch(C.addressof(local_maps), pos.ctypes.data, n, cube_len, det_range, boxes.ctypes.data, counts.ctypes.data))
    return boxes, counts


class PreprocessFeatures(C.Structure):
    _fields_ = [("n_lines", C.c_int32), ("reserved", C.c_int32), ("dis_b", C.c_double)]


class LidarFrontEnd:
    """Stage functions of the camera-LiDAR front end (Preprocess::process, VoxelGrid::filter, feature_extraction)."""

    def __init__(self, max_points_per_scan=140000, max_scans=1):
        self._h = C.c_void_p()
        self.cap = max_points_per_scan
        self.max_scans = max_scans
        _check(lib().tc2li_lidar_create(max_points_per_scan, max_scans, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().tc2li_lidar_destroy(self._h)
            self._h = C.c_void_p()

    def last_timings(self):
        """Device ms of the last frontend_batch: preprocess, voxel hashing, voxel centroids, 5-NN + plane fit, selection, total,
        then the 5-NN stage split into k_knn_plane and k_knn_hard."""
        t = np.zeros(8, np.float32)
        _check(lib().tc2li_lidar_last_timings(self._h, t.ctypes.data))
        return t

    __del__ = close

    def process(self, raw, point_filter_num=2, blind=2.0, time_unit_scale=1e-3):
        raw = np.ascontiguousarray(raw, VELODYNE_DTYPE)
        out = np.zeros(max(len(raw), 1), POINT_DTYPE)
        n = _check(lib().tc2li_lidar_preprocess(self._h, raw.ctypes.data, len(raw), point_filter_num, blind, time_unit_scale,
                                                out.ctypes.data, len(out)))
        return out[:n].copy()

    def set_features(self, n_lines=64, dis_b=0.0):
        """``Preprocess::feature_enabled``: every preprocess of this handle (process, frontend_batch, the inertial batch) takes the plane /
        edge classifier of ``give_feature`` with N_SCANS = n_lines; ``None``: off (the default)."""
        if n_lines is None:
            _check(lib().tc2li_lidar_set_preprocess_features(self._h, None))
            return
        f = PreprocessFeatures(int(n_lines), 0, float(dis_b))
        _check(lib().tc2li_lidar_set_preprocess_features(self._h, C.byref(f)))
        self._n_lines = int(n_lines)

    def corners(self, scan=0):
        """``pl_corn`` (Edge_Jump / Edge_Plane points) of scan slot `scan` of the last preprocess with the classifier on."""
        out = np.zeros(max(self.cap, 1), POINT_DTYPE)
        n = _check(lib().tc2li_lidar_corner_points(self._h, int(scan), out.ctypes.data, len(out)))
        return out[:n].copy()

    def labels(self, scan=0):
        """(Feature label per bucketed point in line order, the n_lines + 1 line offsets) of scan slot `scan` of the last preprocess with
        the classifier on."""
        ft = np.zeros(max(self.cap, 1), np.uint8)
        off = np.zeros(129, np.int32)
        n = _check(lib().tc2li_lidar_point_labels(self._h, int(scan), ft.ctypes.data, off.ctypes.data, len(ft)))
        return ft[:n].copy(), off[:self._n_lines + 1].copy()

    def voxel_filter(self, points, leaf=0.5):
        points = np.ascontiguousarray(points, POINT_DTYPE)
        out = np.zeros(max(len(points), 1), POINT_DTYPE)
        n = _check(lib().tc2li_lidar_voxel_filter(self._h, points.ctypes.data, len(points), leaf, out.ctypes.data, len(out)))
        return out[:n].copy()

    def undistort(self, points, imu_poses22, end_state24):
        """ImuProcess::UndistortPcl, the point part: time sort + compensation into the scan-end frame."""
        pts = np.ascontiguousarray(points, POINT_DTYPE).copy()
        poses = np.ascontiguousarray(imu_poses22, np.float64).reshape(-1, 22)
        st = np.ascontiguousarray(end_state24, np.float64)
        _check(lib().tc2li_lidar_undistort(self._h, pts.ctypes.data, len(pts), poses.ctypes.data, len(poses), st.ctypes.data))
        return pts

    def eskf_update(self, lidar_map, feats_down_body, state36, P, R=0.001, max_iter=4, limit=None, extrinsic_est_en=False):
        """``esekf::update_iterated_dyn_share_modified`` with ``h_share_model`` -> (state36, P [23, 23], EskfStats).  state36: pos 3,
        rot 9, vel 3, bg 3, ba 3, grav 3, offset_R_L_I 9, offset_T_L_I 3."""
        body = np.ascontiguousarray(feats_down_body, POINT_DTYPE)
        st = np.ascontiguousarray(state36, np.float64).copy()
        Pm = np.ascontiguousarray(P, np.float64).reshape(23, 23).copy()
        lim = np.ascontiguousarray(np.full(23, 0.001) if limit is None else limit, np.float64)
        stats = EskfStats()
        f = lib().tc2li_lidar_eskf_update
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._h, lidar_map._h, body.ctypes.data, len(body), st.ctypes.data, Pm.ctypes.data, R, max_iter, lim.ctypes.data,
                 int(extrinsic_est_en), C.addressof(stats)))
        return st, Pm, stats

    def time_sort(self, points, depth_limit=-1):
        """The permutation ``std::sort(points, time_list)`` leaves (UndistortPcl's time sort), computed by the device kernel of the
        inertial batch -> (perm [n], reached_depth_limit)."""
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        perm = np.zeros(max(len(pts), 1), np.int32)
        fb = _check(lib().tc2li_device_time_sort(self._h, pts.ctypes.data, len(pts), int(depth_limit), perm.ctypes.data))
        return perm[:len(pts)], bool(fb)

    def inertial_prepare_batch(self, dev_raw_ptr, raw_offsets, point_filter_num=2, blind=2.0, time_unit_scale=1e-3, stream=0):
        """``tc2li_lidar_inertial_prepare_batch``: Preprocess::process + the order of UndistortPcl's time sort for the scans, kept in this handle
        for the next ``inertial_frontend_batch(None, ...)``."""
        raw_offsets = np.ascontiguousarray(raw_offsets, np.int32)
        f = lib().tc2li_lidar_inertial_prepare_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_void_p]
        return _check(f(self._h, len(raw_offsets) - 1, C.c_void_p(dev_raw_ptr), raw_offsets.ctypes.data, point_filter_num, blind, time_unit_scale,
                        C.c_void_p(stream)))

    def inertial_frontend_batch(self, dev_raw_ptr, raw_offsets, maps, states36, Ps, imus, times, cov12, last6=None, point_filter_num=2, blind=2.0,
                                time_unit_scale=1e-3, leaf=0.5, R=0.001, max_iter=3, limit=None, extrinsic_est_en=False, stream=0):
        """``LidarInertialProcess`` for a batch of sequences (tc2li_lidar_inertial_frontend_batch).  states36 [S, 36] (pos 3, rot 9, vel 3, bg 3,
        ba 3, grav 3, offset_R_L_I 9, offset_T_L_I 3), Ps [S, 23, 23], imus: list of [K, 7] sample arrays (t, acc, gyr), times [S, 4] =
        pcl_beg_time, pcl_end_time, last_lidar_end_time, acc_scale, last6 [S, 6] = acc_s_last, angvel_last ->
        (states36, Ps, list of EskfStats, n_preprocessed, n_downsampled, last6).  dev_raw_ptr None: the scans inertial_prepare_batch left in
        this handle."""
        S = len(raw_offsets) - 1
        raw_offsets = np.ascontiguousarray(raw_offsets, np.int32)
        st = np.ascontiguousarray(states36, np.float64).reshape(S, 36).copy()
        Pm = np.ascontiguousarray(Ps, np.float64).reshape(S, 529).copy()
        times = np.ascontiguousarray(times, np.float64).reshape(S, 4)
        last = np.zeros((S, 6)) if last6 is None else np.ascontiguousarray(last6, np.float64).reshape(S, 6).copy()
        cov = np.ascontiguousarray(cov12, np.float64)
        lim = np.ascontiguousarray(np.full(23, 0.001) if limit is None else limit, np.float64)
        imus = [np.ascontiguousarray(x, np.float64).reshape(-1, 7) for x in imus]
        scans = (LidarInertialScan * S)()
        for s in range(S):
            sc = scans[s]
            sc.imu, sc.n_imu = imus[s].ctypes.data, len(imus[s])
            sc.pcl_beg_time, sc.pcl_end_time, sc.last_lidar_end_time, sc.acc_scale = [float(v) for v in times[s]]
            for k in range(3):
                sc.acc_s_last[k], sc.angvel_last[k] = last[s, k], last[s, 3 + k]
            C.memmove(C.addressof(sc.state), st[s].ctypes.data, 36 * 8)
            sc.P = Pm[s].ctypes.data
        handles = (C.c_void_p * S)(*[m._h for m in maps])
        f = lib().tc2li_lidar_inertial_frontend_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._h, S, C.c_void_p(dev_raw_ptr or 0), raw_offsets.ctypes.data, point_filter_num, blind, time_unit_scale, leaf, handles, scans,
                 cov.ctypes.data, R, max_iter, lim.ctypes.data, int(extrinsic_est_en), C.c_void_p(stream)))
        stats, n_pre, n_down = [], np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            sc = scans[s]
            C.memmove(st[s].ctypes.data, C.addressof(sc.state), 36 * 8)
            e = EskfStats()
            C.memmove(C.addressof(e), C.addressof(sc.stats), C.sizeof(EskfStats))
            stats.append(e)
            n_pre[s], n_down[s] = sc.n_preprocessed, sc.n_downsampled
            for k in range(3):
                last[s, k], last[s, 3 + k] = sc.acc_s_last[k], sc.angvel_last[k]
        return st, Pm.reshape(S, 23, 23), stats, n_pre, n_down, last

    def feature_extraction(self, lidar_map, feats_down_body, state24):
        body = np.ascontiguousarray(feats_down_body, POINT_DTYPE)
        n = len(body)
        m1 = max(n, 1)
        world = np.zeros(m1, POINT_DTYPE)
        sel = np.zeros(m1, np.uint8)
        normvec = np.zeros(m1, POINT_DTYPE)
        near = np.zeros((m1, 5), POINT_DTYPE)
        dist = np.zeros((m1, 5), np.float32)
        nfound = np.zeros(m1, np.int32)
        ori = np.zeros(m1, POINT_DTYPE)
        corr = np.zeros(m1, POINT_DTYPE)
        state24 = np.ascontiguousarray(state24, np.float64)
        m = _check(lib().tc2li_lidar_feature_extraction(self._h, lidar_map._h, body.ctypes.data, n, state24.ctypes.data,
                                                        world.ctypes.data, sel.ctypes.data, normvec.ctypes.data, near.ctypes.data,
                                                        dist.ctypes.data, nfound.ctypes.data, ori.ctypes.data, corr.ctypes.data, m1))
        return dict(world=world[:n], selected=sel[:n], normvec=normvec[:n], nearest=near[:n], sqdist=dist[:n], nfound=nfound[:n],
                    cloud_ori=ori[:m], corr_normvect=corr[:m], effct_feat_num=m)

    def frontend_batch(self, dev_raw_ptr, raw_offsets, maps, states, point_filter_num=2, blind=2.0, time_unit_scale=1e-3,
                       leaf=0.5, stream=0, want_points=True, capacity=None):
        n_scans = len(raw_offsets) - 1
        raw_offsets = np.ascontiguousarray(raw_offsets, np.int32)
        states = np.ascontiguousarray(states, np.float64).reshape(n_scans, 24)
        handles = (C.c_void_p * n_scans)(*[m._h for m in maps])
        counts = np.zeros((3, n_scans), np.int32)
        capacity = capacity or self.cap
        ori = corr = None
        if want_points:
            ori = np.zeros((n_scans, capacity), POINT_DTYPE)
            corr = np.zeros((n_scans, capacity), POINT_DTYPE)
        _check(lib().tc2li_lidar_frontend_batch(self._h, n_scans, C.c_void_p(dev_raw_ptr), raw_offsets.ctypes.data,
                                                point_filter_num, blind, time_unit_scale, leaf, handles, states.ctypes.data,
                                                counts[0].ctypes.data, counts[1].ctypes.data, counts[2].ctypes.data,
                                                ori.ctypes.data if want_points else None,
                                                corr.ctypes.data if want_points else None, capacity, C.c_void_p(stream)))
        return counts, ori, corr


# ---- optimisation back end ----------------------------------------------------------------------------------------
BA_EDGE_DTYPE = np.dtype([("point", "<i4"), ("pose", "<i4"), ("u", "<f8"), ("v", "<f8"), ("u_right", "<f8"), ("inv_sigma2", "<f8")])


def pack_ba_edges(edges6):
    """[E, 6] float array (point, pose, u, v, uR, invSigma2) -> structured tc2li_ba_edge array."""
    e = np.asarray(edges6, np.float64).reshape(-1, 6)
    out = np.zeros(len(e), BA_EDGE_DTYPE)
    out["point"], out["pose"] = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)
    out["u"], out["v"], out["u_right"], out["inv_sigma2"] = e[:, 2], e[:, 3], e[:, 4], e[:, 5]
    return out


def pose_optimization(pose7, Xw, edges, cam5):
    """``Optimizer::PoseOptimization`` -> (pose7, outlier mask, inliers)."""
    pose = np.ascontiguousarray(pose7, np.float64).copy()
    Xw = np.ascontiguousarray(Xw, np.float64)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    out = np.zeros(max(len(edges), 1), np.uint8)
    inl = _check(lib().tc2li_pose_optimization(pose.ctypes.data, Xw.ctypes.data, edges.ctypes.data, len(edges), cam5.ctypes.data,
                                               out.ctypes.data))
    return pose, out[:len(edges)], inl


def pose_optimization_batch(poses7, edge_offsets, Xw, edges, cam5, stream=0):
    poses = np.ascontiguousarray(poses7, np.float64).copy()
    offs = np.ascontiguousarray(edge_offsets, np.int32)
    Xw = np.ascontiguousarray(Xw, np.float64)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    n = len(offs) - 1
    out = np.zeros(max(len(edges), 1), np.uint8)
    inl = np.zeros(n, np.int32)
    _check(lib().tc2li_pose_optimization_batch(n, poses.ctypes.data, offs.ctypes.data, Xw.ctypes.data, edges.ctypes.data,
                                               cam5.ctypes.data, out.ctypes.data, inl.ctypes.data, C.c_void_p(stream)))
    return poses, out[:len(edges)], inl


def pose_optimization_limits():
    """tc2li_pose_optimization_limits -> {lds_max_edges, lds_granule, threads, last_form}: a batch whose largest frame has more than lds_max_edges
    correspondences runs the global-memory kernel; last_form is what the most recent pose optimisation launched (0 none, 1 LDS, 2 global,
    3 LDS in the compact layout after the public entries' device-side check; TC2LI_PO_COMPACT=0 keeps the 61-byte layout)."""
    out = (C.c_int32 * 4)()
    f = lib().tc2li_pose_optimization_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 4))
    return dict(zip(("lds_max_edges", "lds_granule", "threads", "last_form"), [int(v) for v in out]))


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("n_free_poses", C.c_int32), ("pad_", C.c_int32),
                ("initial_chi2", C.c_double), ("final_chi2", C.c_double), ("final_lambda", C.c_double)]


def local_bundle_adjustment(poses7, fixed, points3, edges, cam5, iterations=10, lambda_init=0.0, stop_flag=None, stream=0):
    """The optimisation of ``Optimizer::LocalBundleAdjustment`` -> (poses7, points3, chi2, depth_positive, stats)."""
    poses = np.ascontiguousarray(poses7, np.float64).copy()
    pts = np.ascontiguousarray(points3, np.float64).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    chi2 = np.zeros(max(len(edges), 1))
    dpos = np.zeros(max(len(edges), 1), np.uint8)
    stats = BaStats()
    stop_ptr = stop_flag.ctypes.data if stop_flag is not None else None
    _check(lib().tc2li_local_bundle_adjustment(poses.ctypes.data, fixed.ctypes.data, len(poses), pts.ctypes.data, len(pts),
                                               edges.ctypes.data, len(edges), cam5.ctypes.data, iterations, lambda_init, stop_ptr,
                                               chi2.ctypes.data, dpos.ctypes.data, C.byref(stats), C.c_void_p(stream)))
    return poses, pts, chi2[:len(edges)], dpos[:len(edges)], stats


# ---- IMU pre-integration (IMU::Preintegrated, Tracking::PreintegrateIMU / PredictStateIMU) -----------------------------
IMU_SAMPLE_DTYPE = np.dtype([("t", "<f8"), ("a", "<f4", (3,)), ("w", "<f4", (3,))])


class ImuBias(C.Structure):
    _fields_ = [("bax", C.c_float), ("bay", C.c_float), ("baz", C.c_float), ("bwx", C.c_float), ("bwy", C.c_float), ("bwz", C.c_float)]


class InertialInitStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("initial_chi2", C.c_double), ("final_chi2", C.c_double), ("final_lambda", C.c_double)]


def imu_init_gravity(Rwb, twb, pres):
    """First estimate of ``LocalMapping::InitializeIMU``: keyframes in temporal order, ``pres[i]`` = Preintegrated of keyframe i from i - 1
    (``pres[0]`` ignored) -> (velocities [N, 3] float32, Rwg [3, 3] float32)."""
    R, t = np.ascontiguousarray(Rwb, np.float32).reshape(-1, 9), np.ascontiguousarray(twb, np.float32).reshape(-1, 3)
    n = len(R)
    ptrs = (C.c_void_p * n)(*[None if (i == 0 or pres[i] is None) else C.addressof(pres[i].p) for i in range(n)])
    vel, Rwg = np.zeros((n, 3), np.float32), np.zeros(9, np.float32)
    f = lib().tc2li_imu_init_gravity
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(n, R.ctypes.data, t.ctypes.data, ptrs, vel.ctypes.data, Rwg.ctypes.data))
    return vel, Rwg.reshape(3, 3)


def inertial_scale_refinement(Rwb, twb, vel, bg, ba, pres, Rwg, scale, iterations=10):
    """``Optimizer::InertialOptimization(pMap, Rwg, scale)`` (ScaleRefinement) -> (Rwg, scale, iterations, (chi2 before, after))."""
    R, t = np.ascontiguousarray(Rwb, np.float64).reshape(-1, 9), np.ascontiguousarray(twb, np.float64).reshape(-1, 3)
    n = len(R)
    v, g, a = [np.ascontiguousarray(x, np.float64).reshape(n, 3) for x in (vel, bg, ba)]
    ptrs = (C.c_void_p * n)(*[None if (i == 0 or pres[i] is None) else C.addressof(pres[i].p) for i in range(n)])
    Rg, s, chi = np.ascontiguousarray(Rwg, np.float64).reshape(9).copy(), C.c_double(scale), np.zeros(2)
    f = lib().tc2li_inertial_scale_refinement
    f.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]
    it = _check(f(n, R.ctypes.data, t.ctypes.data, v.ctypes.data, g.ctypes.data, a.ctypes.data, ptrs, Rg.ctypes.data, C.addressof(s), iterations, chi.ctypes.data))
    return Rg.reshape(3, 3), s.value, it, (chi[0], chi[1])


def inertial_optimization(Rwb, twb, vel, pres, Rwg, scale, bg, ba, mono=False, fixed_vel=False, prior_g=1e2, prior_a=1e6, iterations=200):
    """``Optimizer::InertialOptimization`` (IMU initialisation) -> (velocities [N, 3], Rwg, scale, bg, ba, InertialInitStats)."""
    R, t = np.ascontiguousarray(Rwb, np.float64).reshape(-1, 9), np.ascontiguousarray(twb, np.float64).reshape(-1, 3)
    n = len(R)
    v = np.ascontiguousarray(vel, np.float64).reshape(n, 3).copy()
    ptrs = (C.c_void_p * n)(*[None if (i == 0 or pres[i] is None) else C.addressof(pres[i].p) for i in range(n)])
    Rg, g, a = np.ascontiguousarray(Rwg, np.float64).reshape(9).copy(), np.ascontiguousarray(bg, np.float64).copy(), np.ascontiguousarray(ba, np.float64).copy()
    s, st = C.c_double(scale), InertialInitStats()
    f = lib().tc2li_inertial_optimization
    f.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]
    _check(f(n, R.ctypes.data, t.ctypes.data, v.ctypes.data, ptrs, Rg.ctypes.data, C.addressof(s), g.ctypes.data, a.ctypes.data, int(mono), int(fixed_vel),
             prior_g, prior_a, iterations, C.addressof(st)))
    return v, Rg.reshape(3, 3), s.value, g, a, st


class PreintegratedPOD(C.Structure):
    _fields_ = [("dT", C.c_float), ("n_measurements", C.c_int32), ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3),
                ("JRg", C.c_float * 9), ("JVg", C.c_float * 9), ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9),
                ("avgA", C.c_float * 3), ("avgW", C.c_float * 3), ("C", C.c_float * 225), ("noise", C.c_float * 6),
                ("noise_walk", C.c_float * 6), ("bias", ImuBias)]


class Preintegrated:
    """Mirror of ``IMU::Preintegrated`` (SF/include/ImuTypes.h:141-235)."""

    def __init__(self, bias6, ng, na, ngw, naw):
        self.p = PreintegratedPOD()
        b = ImuBias(*[float(x) for x in bias6])
        _check(lib().tc2li_imu_preintegrated_init(C.addressof(self.p), C.addressof(b), ng, na, ngw, naw))

    def IntegrateNewMeasurement(self, acc, ang_vel, dt):
        a, w = np.ascontiguousarray(acc, np.float32), np.ascontiguousarray(ang_vel, np.float32)
        _check(lib().tc2li_imu_integrate(C.addressof(self.p), a.ctypes.data, w.ctypes.data, float(dt)))

    def preintegrate(self, samples, t_prev, t_cur):
        """The loop of Tracking::PreintegrateIMU over mvImuFromLastFrame -> number of integration steps."""
        s = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
        return _check(lib().tc2li_imu_preintegrate(C.addressof(self.p), s.ctypes.data, len(s), float(t_prev), float(t_cur)))

    def delta(self, bias6):
        """GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition at another bias."""
        b = ImuBias(*[float(x) for x in bias6])
        dR, dV, dP = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        _check(lib().tc2li_imu_delta(C.addressof(self.p), C.addressof(b), dR.ctypes.data, dV.ctypes.data, dP.ctypes.data))
        return dR.reshape(3, 3), dV, dP

    def predict_state(self, bias6, Rwb1, twb1, Vwb1):
        """Tracking::PredictStateIMU -> (Rwb2, twb2, Vwb2)."""
        b = ImuBias(*[float(x) for x in bias6])
        R1, t1, v1 = [np.ascontiguousarray(a, np.float32) for a in (Rwb1, twb1, Vwb1)]
        R2, t2, v2 = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        _check(lib().tc2li_imu_predict_state(C.addressof(self.p), C.addressof(b), R1.ctypes.data, t1.ctypes.data, v1.ctypes.data,
                                             R2.ctypes.data, t2.ctypes.data, v2.ctypes.data))
        return R2.reshape(3, 3), t2, v2

    def fields(self):
        g = lambda name, shape: np.array(getattr(self.p, name), np.float32).reshape(shape)
        return dict(dT=self.p.dT, dR=g("dR", (3, 3)), dV=g("dV", 3), dP=g("dP", 3), JRg=g("JRg", (3, 3)), JVg=g("JVg", (3, 3)),
                    JVa=g("JVa", (3, 3)), JPg=g("JPg", (3, 3)), JPa=g("JPa", (3, 3)), avgA=g("avgA", 3), avgW=g("avgW", 3), C=g("C", (15, 15)))


def lidar_imu_propagate(state36, imu7, beg, end, last_end, acc_scale, last6):
    """Forward propagation of UndistortPcl (host) -> (end state [36], poses [K, 22], updated last6)."""
    st = np.ascontiguousarray(state36, np.float64).copy()
    imu = np.ascontiguousarray(imu7, np.float64).reshape(-1, 7)
    last = np.ascontiguousarray(last6, np.float64).copy()
    poses = np.zeros((len(imu) + 2, 22))
    k = _check(lib().tc2li_lidar_imu_propagate(st.ctypes.data, imu.ctypes.data, len(imu), beg, end, last_end, acc_scale, last.ctypes.data,
                                               last.ctypes.data + 24, poses.ctypes.data, len(poses)))
    return st, poses[:k], last


class KeyframeView(C.Structure):
    """tc2li_keyframe_view"""
    _fields_ = [("n", C.c_int32), ("n_nodes", C.c_int32), ("keys", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p),
                ("depth", C.c_void_p), ("has_point", C.c_void_p), ("fv_node", C.c_void_p), ("fv_offset", C.c_void_p), ("fv_index", C.c_void_p),
                ("pose7", C.c_float * 7), ("pad_", C.c_float)]


class NewMapPoint(C.Structure):
    """tc2li_new_map_point"""
    _fields_ = [("idx1", C.c_int32), ("neighbour", C.c_int32), ("idx2", C.c_int32), ("stereo", C.c_int32), ("x3D", C.c_float * 3), ("pad_", C.c_float)]


NEW_MAP_POINT_DTYPE = np.dtype([("idx1", "<i4"), ("neighbour", "<i4"), ("idx2", "<i4"), ("stereo", "<i4"), ("x3D", "<f4", (3,)), ("pad_", "<f4")])
assert NEW_MAP_POINT_DTYPE.itemsize == C.sizeof(NewMapPoint)


def pack_keyframe_views(items):
    """items: dicts with keys (KEYPOINT_DTYPE), descriptors, u_right, depth, has_point, fv_node, fv_offset, fv_index, pose7 ->
    (ctypes array of tc2li_keyframe_view, keep-alive list)."""
    arr = (KeyframeView * max(len(items), 1))()
    keep = []
    for i, it in enumerate(items):
        k = np.ascontiguousarray(it["keys"], KEYPOINT_DTYPE)
        d = np.ascontiguousarray(it["descriptors"], np.uint8).reshape(-1, 32)
        ur, z = np.ascontiguousarray(it["u_right"], np.float32), np.ascontiguousarray(it["depth"], np.float32)
        hp = np.ascontiguousarray(it["has_point"], np.uint8)
        fn, fo, fi = [np.ascontiguousarray(it[f], np.int32) for f in ("fv_node", "fv_offset", "fv_index")]
        keep.append((k, d, ur, z, hp, fn, fo, fi))
        arr[i].n, arr[i].n_nodes = len(k), len(fn)
        arr[i].keys, arr[i].descriptors, arr[i].u_right, arr[i].depth, arr[i].has_point = (k.ctypes.data, d.ctypes.data, ur.ctypes.data, z.ctypes.data,
                                                                                          hp.ctypes.data)
        arr[i].fv_node, arr[i].fv_offset, arr[i].fv_index = fn.ctypes.data, fo.ctypes.data, fi.ctypes.data
        arr[i].pose7 = (C.c_float * 7)(*[float(v) for v in it["pose7"]])
    return arr, keep


def search_for_triangulation(kf1, kf2, cam5, scale_factors, level_sigma2, only_stereo=False, coarse=False, check_orientation=False, stream=0):
    """``ORBmatcher::SearchForTriangulation`` -> (nmatches, match12 [n1])."""
    arr, keep = pack_keyframe_views([kf1, kf2])
    cam5 = np.ascontiguousarray(cam5, np.float64)
    sf, sg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    match = np.full(max(arr[0].n, 1), -1, np.int32)
    f = lib().tc2li_search_for_triangulation
    f.argtypes = [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    n = _check(f(C.addressof(arr), C.addressof(arr) + C.sizeof(KeyframeView), cam5.ctypes.data, sf.ctypes.data, sg.ctypes.data, len(sf), int(only_stereo),
                 int(coarse), int(check_orientation), match.ctypes.data, C.c_void_p(stream)))
    del keep
    return n, match[:arr[0].n]


def create_new_map_points(cur, neighbours, cam5, mb, scale_factors, level_sigma2, scale_factor=1.2, inertial=False, far_points=False,
                          th_far_points=0.0, coarse=False, stream=0):
    """The geometric loop of ``LocalMapping::CreateNewMapPoints`` -> (idx [k, 4] = idx1, neighbour, idx2, stereo; x3D [k, 3])."""
    arr, keep = pack_keyframe_views([cur] + list(neighbours))
    cam5 = np.ascontiguousarray(cam5, np.float64)
    sf, sg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    cap = max(arr[0].n, 1)
    pts = (NewMapPoint * cap)()
    f = lib().tc2li_create_new_map_points
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float,
                  C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    n = _check(f(C.addressof(arr), C.addressof(arr) + C.sizeof(KeyframeView), len(neighbours), cam5.ctypes.data, mb, sf.ctypes.data, sg.ctypes.data,
                 len(sf), scale_factor, int(inertial), int(far_points), th_far_points, int(coarse), C.addressof(pts), cap, C.c_void_p(stream)))
    del keep
    idx = np.array([[pts[k].idx1, pts[k].neighbour, pts[k].idx2, pts[k].stereo] for k in range(n)], np.int32).reshape(-1, 4)
    x3D = np.array([list(pts[k].x3D) for k in range(n)], np.float32).reshape(-1, 3)
    return idx, x3D


def track_local_map_batch(ext, n_frames, keypoints, u_right, poses7, held, held_Xw, local_points, local_offsets, cam5, th=1.0, far_points=False,
                          th_far=0.0, stream=0, out=None):
    """``tc2li_track_local_map_batch`` on the features of the last ``extract_batch_dev`` call ->
    (poses7 double [F, 7], local_of_keypoint [F, cap], outlier [F, cap], n_matches [F], n_inliers [F])."""
    kps = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    cap = kps.shape[1]
    ur = np.ascontiguousarray(u_right, np.float32)
    p7 = np.ascontiguousarray(poses7, np.float32).reshape(n_frames, 7)
    h = np.ascontiguousarray(held, np.uint8).reshape(n_frames, cap)
    hx = np.ascontiguousarray(held_Xw, np.float32).reshape(n_frames, cap, 3)
    pts = np.ascontiguousarray(local_points, MAP_POINT_DTYPE)
    off = np.ascontiguousarray(local_offsets, np.int32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    if out is None:
        out = (np.zeros((n_frames, 7)), np.full((n_frames, cap), -1, np.int32), np.zeros((n_frames, cap), np.uint8), np.zeros(n_frames, np.int32),
               np.zeros(n_frames, np.int32))
    out_p, lk, ol, nm, inl = out
    f = lib().tc2li_track_local_map_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                  C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(ext._h, n_frames, kps.ctypes.data, ur.ctypes.data, cap, p7.ctypes.data, h.ctypes.data, hx.ctypes.data, pts.ctypes.data if len(pts) else None,
             off.ctypes.data, cam5.ctypes.data, th, int(far_points), th_far, out_p.ctypes.data, lk.ctypes.data, ol.ctypes.data, nm.ctypes.data,
             inl.ctypes.data, C.c_void_p(stream)))
    return out_p, lk, ol, nm, inl


def search_local_points_batch(ext, n_frames, keypoints, u_right, poses7, held, held_Xw, local_points, local_offsets, cam5, th=1.0, far_points=False,
                              th_far=0.0, stream=0, out=None):
    """``tc2li_search_local_points_batch`` (Tracking::SearchLocalPoints alone: the camera-LiDAR-inertial configuration's TrackLocalMap optimises with
    PoseInertialOptimization) on the features of the last ``extract_batch_dev`` call -> (local_of_keypoint [F, cap], n_matches [F])."""
    kps = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    cap = kps.shape[1]
    ur = np.ascontiguousarray(u_right, np.float32)
    p7 = np.ascontiguousarray(poses7, np.float32).reshape(n_frames, 7)
    h = np.ascontiguousarray(held, np.uint8).reshape(n_frames, cap)
    hx = np.ascontiguousarray(held_Xw, np.float32).reshape(n_frames, cap, 3)
    pts = np.ascontiguousarray(local_points, MAP_POINT_DTYPE)
    off = np.ascontiguousarray(local_offsets, np.int32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    if out is None:
        out = (np.full((n_frames, cap), -1, np.int32), np.zeros(n_frames, np.int32))
    lk, nm = out
    f = lib().tc2li_search_local_points_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                  C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(ext._h, n_frames, kps.ctypes.data, ur.ctypes.data, cap, p7.ctypes.data, h.ctypes.data, hx.ctypes.data, pts.ctypes.data if len(pts) else None,
             off.ctypes.data, cam5.ctypes.data, th, int(far_points), th_far, lk.ctypes.data, nm.ctypes.data, C.c_void_p(stream)))
    return lk, nm


def fuse_search(keys, desc, u_right, cols, rows, pose7, cam4, bf, scale_factors, inv_level_sigma2, log_scale_factor, points, valid, th=3.0, stream=0):
    """``ORBmatcher::Fuse``, the search part -> (n_fused, best_idx [m], best_dist [m]); points: MAP_POINT_DTYPE."""
    k = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8)
    ur = np.ascontiguousarray(u_right, np.float32)
    fv = FrameView(k.ctypes.data, d.ctypes.data, ur.ctypes.data, None, len(k), 0.0, float(cols), 0.0, float(rows))
    pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
    val = np.ascontiguousarray(valid, np.uint8)
    sf, isg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    p7, c4 = np.ascontiguousarray(pose7, np.float32), np.ascontiguousarray(cam4, np.float32)
    m = len(pts)
    bi, bd = np.full(max(m, 1), -1, np.int32), np.zeros(max(m, 1), np.int32)
    f = lib().tc2li_fuse_search
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    nf = _check(f(C.addressof(fv), p7.ctypes.data, c4.ctypes.data, bf, sf.ctypes.data, isg.ctypes.data, len(sf), log_scale_factor, pts.ctypes.data,
                  val.ctypes.data, m, th, bi.ctypes.data, bd.ctypes.data, C.c_void_p(stream)))
    return nf, bi[:m], bd[:m]


# ---- local mapping for many keyframes: keyframe store, CreateNewMapPoints / Fuse search in batches ---------------------------------------
class NewPointsProblem(C.Structure):
    """tc2li_new_points_problem"""
    _fields_ = [("current", C.c_int32), ("n_neighbours", C.c_int32), ("neighbours", C.c_void_p), ("poses7", C.c_void_p), ("has_point", C.c_void_p),
                ("inertial", C.c_uint8), ("far_points", C.c_uint8), ("coarse", C.c_uint8), ("pad_", C.c_uint8), ("th_far_points", C.c_float)]


class FuseItem(C.Structure):
    """tc2li_fuse_item"""
    _fields_ = [("keyframe", C.c_int32), ("first_point", C.c_int32), ("first_valid", C.c_int32), ("n_points", C.c_int32), ("pose7", C.c_float * 7),
                ("th", C.c_float)]


class KeyframeStore:
    """``tc2li_keyframe_store``: what a keyframe never changes after creation, resident on the device.  Slots are 0 .. max_keyframes - 1."""

    def __init__(self, max_keyframes, max_keypoints):
        self._h = C.c_void_p()
        f = lib().tc2li_keyframe_store_create
        f.argtypes = [C.c_int, C.c_int, C.c_void_p]
        _check(f(int(max_keyframes), int(max_keypoints), C.byref(self._h)))
        self.max_keyframes, self.max_keypoints = int(max_keyframes), int(max_keypoints)

    def _handle(self):
        if not self._h:
            raise Tc2liError(-1, "keyframe store is closed")
        return self._h

    def put_batch(self, slots, keyframes, bounds, n_levels=8, stream=0):
        """keyframes: the dicts ``pack_keyframe_views`` takes (``has_point`` / ``pose7`` may be absent: they are not stored);
        bounds: (min_x, max_x, min_y, max_y), one for all or one per keyframe."""
        items = []
        for kf in keyframes:
            it = dict(kf)
            it.setdefault("has_point", np.zeros(len(kf["keys"]), np.uint8))
            it.setdefault("pose7", np.float32([0, 0, 0, 1, 0, 0, 0]))
            items.append(it)
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        if len(sl) != len(items):
            raise ValueError("one slot per keyframe")
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, np.float32).reshape(-1, 4), (len(items), 4)), np.float32)
        arr, keep = pack_keyframe_views(items)
        f = lib().tc2li_keyframe_store_put_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._handle(), len(items), sl.ctypes.data, C.addressof(arr), b.ctypes.data, int(n_levels), C.c_void_p(stream)))
        del keep

    def erase(self, slot):
        f = lib().tc2li_keyframe_store_erase
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(self._handle(), int(slot)))

    def info(self, slot):
        """(n_keypoints, n_nodes) of the keyframe in the slot, (-1, -1) for an empty slot."""
        n, m = C.c_int32(0), C.c_int32(0)
        f = lib().tc2li_keyframe_store_info
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(self._handle(), int(slot), C.byref(n), C.byref(m)))
        return n.value, m.value

    def close(self):
        if self._h:
            f = lib().tc2li_keyframe_store_destroy
            f.argtypes = [C.c_void_p]
            f(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_new_points_problems(store, problems):
    """problems: dicts with current (slot), neighbours (slots), poses7 [1 + k, 7], has_point (1 + k arrays: of the current keyframe, then of
    each neighbour) and optionally inertial, far_points, th_far_points, coarse -> (ctypes array, keep-alive list, keypoints of each current)."""
    arr = (NewPointsProblem * max(len(problems), 1))()
    keep, n_cur = [], []
    for i, pr in enumerate(problems):
        nb = np.ascontiguousarray(pr["neighbours"], np.int32).reshape(-1)
        p7 = np.ascontiguousarray(pr["poses7"], np.float32).reshape(-1, 7)
        hps = [np.ascontiguousarray(h, np.uint8).reshape(-1) for h in pr["has_point"]]
        if len(p7) != 1 + len(nb) or len(hps) != 1 + len(nb):
            raise ValueError("problem %d: one pose and one has_point array for the current keyframe and for each neighbour" % i)
        for s, h in zip([int(pr["current"])] + [int(v) for v in nb], hps):
            n = store.info(s)[0] if 0 <= s < store.max_keyframes else -1
            if n >= 0 and len(h) != n:
                raise ValueError("problem %d: has_point of slot %d has %d entries, the keyframe %d keypoints" % (i, s, len(h), n))
        ptrs = (C.c_void_p * len(hps))(*[h.ctypes.data for h in hps])
        keep.append((nb, p7, hps, ptrs))
        arr[i].current, arr[i].n_neighbours = int(pr["current"]), len(nb)
        arr[i].neighbours, arr[i].poses7, arr[i].has_point = nb.ctypes.data, p7.ctypes.data, C.addressof(ptrs)
        arr[i].inertial, arr[i].far_points, arr[i].coarse = int(bool(pr.get("inertial", False))), int(bool(pr.get("far_points", False))), int(bool(pr.get("coarse", False)))
        arr[i].th_far_points = float(pr.get("th_far_points", 0.0))
        n0 = store.info(int(pr["current"]))[0] if 0 <= int(pr["current"]) < store.max_keyframes else 0
        n_cur.append(max(n0, 0))
    return arr, keep, n_cur


def create_new_map_points_batch(store, problems, cam5, mb, scale_factors, level_sigma2, scale_factor=1.2, capacities=None, stream=0, raw=False):
    """``tc2li_create_new_map_points_batch`` -> one (idx [k, 4] = idx1, neighbour, idx2, stereo; x3D [k, 3]) per problem, as
    ``create_new_map_points`` gives it.  capacities: room per problem (default: the keypoints of its current keyframe, which always
    suffices).  raw=True -> (return code, n_points [P], records) without raising on TC2LI_ERR_CAPACITY."""
    arr, keep, n_cur = pack_new_points_problems(store, problems)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    sf, sg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    caps = np.asarray(n_cur if capacities is None else capacities, np.int64).reshape(-1)
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
    pts = np.zeros(max(int(off[-1]), 1), NEW_MAP_POINT_DTYPE)
    cnt = np.zeros(max(len(problems), 1), np.int32)
    f = lib().tc2li_create_new_map_points_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p]
    rc = f(store._handle(), C.addressof(arr), len(problems), cam5.ctypes.data, mb, sf.ctypes.data, sg.ctypes.data, len(sf), scale_factor, pts.ctypes.data,
           off.ctypes.data, cnt.ctypes.data, C.c_void_p(stream))
    del keep
    cnt = cnt[:len(problems)]
    if raw:
        return rc, cnt, [pts[off[p]:off[p] + min(int(cnt[p]), int(caps[p]))] for p in range(len(problems))]
    _check(rc)
    out = []
    for p in range(len(problems)):
        r = pts[off[p]:off[p] + cnt[p]]
        out.append((np.stack([r["idx1"], r["neighbour"], r["idx2"], r["stereo"]], 1).astype(np.int32).reshape(-1, 4), r["x3D"].astype(np.float32).reshape(-1, 3)))
    return out


def fuse_search_batch(store, items, cam4, bf, scale_factors, inv_level_sigma2, log_scale_factor, points, valid, stream=0):
    """``tc2li_fuse_search_batch``.  items: dicts with keyframe (slot), first_point, first_valid, n_points, pose7, th; points:
    MAP_POINT_DTYPE (all lists, concatenated), valid: uint8 (one range per item) -> (n_fused [items], best_idx, best_dist), the last
    two indexed like ``valid``."""
    arr = (FuseItem * max(len(items), 1))()
    for i, it in enumerate(items):
        arr[i].keyframe, arr[i].first_point, arr[i].first_valid, arr[i].n_points = int(it["keyframe"]), int(it["first_point"]), int(it["first_valid"]), int(it["n_points"])
        arr[i].pose7 = (C.c_float * 7)(*[float(v) for v in it["pose7"]])
        arr[i].th = float(it.get("th", 3.0))
    pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
    val = np.ascontiguousarray(valid, np.uint8).reshape(-1)
    sf, isg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    c4 = np.ascontiguousarray(cam4, np.float32)
    m = len(val)
    bi, bd, nf = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), 256, np.int32), np.zeros(max(len(items), 1), np.int32)
    f = lib().tc2li_fuse_search_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(store._handle(), C.addressof(arr), len(items), c4.ctypes.data, bf, sf.ctypes.data, isg.ctypes.data, len(sf), log_scale_factor,
             pts.ctypes.data if len(pts) else None, len(pts), val.ctypes.data if m else None, m, bi.ctypes.data, bd.ctypes.data, nf.ctypes.data,
             C.c_void_p(stream)))
    return nf[:len(items)], bi[:m], bd[:m]


# ---- LocalMapping::SearchInNeighbors in the reference's order (tc2li_search_in_neighbors_batch) ------------------------------------------
_NEIGHBORS_INPUTS = (("kf_slot", np.int32), ("kf_flags", np.uint8), ("prev_kf", np.int32), ("poses7", np.float32), ("covis_offsets", np.int32),
                     ("covis", np.int32), ("slot_offsets", np.int32), ("slot_point", np.int32), ("points", None), ("point_flags", np.uint8),
                     ("point_nobs", np.int32), ("point_found", np.int32), ("point_visible", np.int32), ("point_ref_kf", np.int32),
                     ("point_ref_level_scale", np.float32), ("obs_offsets", np.int32), ("obs_kf", np.int32), ("obs_index", np.int32))
_NEIGHBORS_OUTPUTS = ("counts", "targets", "target_fused", "candidates", "ops", "slot_point_out", "point_bad_out", "point_replaced", "point_nobs_out",
                      "point_found_out", "point_visible_out", "obs_offsets_out", "obs_kf_out", "obs_index_out", "desc_kf", "desc_index", "refreshed",
                      "normals_out", "min_distance_out", "max_distance_out")
NEIGHBORS_OP_DTYPE = np.dtype([(k, "<i4") for k in ("kind", "stage_target", "point", "occupant", "winner", "kf", "idx", "pad_")])
NEIGHBORS_COUNTS = ("status", "targets", "candidates", "ops", "observations", "refreshed", "fused_stage1", "fused_current")
NEIGHBORS_ON_DEVICE, NEIGHBORS_ON_HOST, NEIGHBORS_ADD_OBSERVATION, NEIGHBORS_REPLACE, NEIGHBORS_MAX_TARGETS = 0, 1, 1, 2, 210


class NeighborsProblem(C.Structure):
    """tc2li_neighbors_problem"""
    _fields_ = [(k, C.c_void_p) for k, _ in _NEIGHBORS_INPUTS] + [(k, C.c_void_p) for k in _NEIGHBORS_OUTPUTS] \
        + [(k, C.c_int32) for k in ("n_keyframes", "n_points", "current", "target_capacity", "candidate_capacity", "op_capacity", "obs_capacity")] \
        + [("last_level_scale", C.c_float), ("inertial", C.c_uint8), ("abort", C.c_uint8), ("pad_", C.c_uint8 * 6)]


def search_in_neighbors_limits():
    """tc2li_search_in_neighbors_limits -> {observations, keypoints, lds_points, lds_keyframes, threads}: beyond the first four a problem
    of ``search_in_neighbors_batch`` is computed by the host twin inside the call."""
    out = np.zeros(8, np.int32)
    f = lib().tc2li_search_in_neighbors_limits
    f.argtypes = [C.c_void_p, C.c_int]
    n = _check(f(out.ctypes.data, len(out)))
    return dict(zip(("observations", "keypoints", "lds_points", "lds_keyframes", "threads"), [int(v) for v in out[:n]]))


def pack_neighbors_problems(problems, capacities=None):
    """The tc2li_neighbors_problem array of a batch with its output arrays -> (array, outputs per problem, what must stay alive).
    problems: dicts with the input arrays of tc2li_neighbors_problem (points: MAP_POINT_DTYPE; poses7 [n, 7]) and current, inertial, abort,
    last_level_scale.  capacities: per problem a dict with targets / candidates / ops / observations; default: what always suffices for
    targets (210) and candidates (n_points), and for ops and observations a guess that the caller enlarges from ``counts`` on
    TC2LI_ERR_CAPACITY (``search_in_neighbors_batch`` does)."""
    P = len(problems)
    arr, outs, keep = (NeighborsProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], MAP_POINT_DTYPE if t is None else t) for k, t in _NEIGHBORS_INPUTS}
        nk, npts = len(a["kf_slot"]), len(a["points"])
        if len(a["covis_offsets"]) != nk + 1 or len(a["slot_offsets"]) != nk + 1 or len(a["obs_offsets"]) != npts + 1 or a["poses7"].size != 7 * nk:
            raise ValueError("problem %d: offsets or poses do not fit the tables" % i)
        for k in ("kf_flags", "prev_kf"):
            if len(a[k]) != nk:
                raise ValueError("problem %d: %s has %d rows for %d keyframes" % (i, k, len(a[k]), nk))
        for k in ("point_flags", "point_nobs", "point_found", "point_visible", "point_ref_kf", "point_ref_level_scale"):
            if len(a[k]) != npts:
                raise ValueError("problem %d: %s has %d rows for %d points" % (i, k, len(a[k]), npts))
        ns, no = int(a["slot_offsets"][-1]), int(a["obs_offsets"][-1])
        if len(a["slot_point"]) < ns or len(a["covis"]) < int(a["covis_offsets"][-1]) or len(a["obs_kf"]) < no or len(a["obs_index"]) < no:
            raise ValueError("problem %d: slot, covisibility or observation arrays are shorter than their offsets say" % i)
        cap = dict(targets=NEIGHBORS_MAX_TARGETS, candidates=npts, ops=max(64, ns // 4), observations=2 * no + 64)
        cap.update((capacities[i] if capacities is not None else None) or {})
        o = dict(counts=np.zeros(len(NEIGHBORS_COUNTS), np.int32), targets=np.full(cap["targets"], -1, np.int32), target_fused=np.zeros(cap["targets"], np.int32),
                 candidates=np.full(cap["candidates"], -1, np.int32), ops=np.zeros(cap["ops"], NEIGHBORS_OP_DTYPE), slot_point_out=np.full(ns, -2, np.int32),
                 point_bad_out=np.zeros(npts, np.uint8), point_replaced=np.full(npts, -2, np.int32), point_nobs_out=np.zeros(npts, np.int32),
                 point_found_out=np.zeros(npts, np.int32), point_visible_out=np.zeros(npts, np.int32), obs_offsets_out=np.zeros(npts + 1, np.int32),
                 obs_kf_out=np.full(cap["observations"], -1, np.int32), obs_index_out=np.full(cap["observations"], -1, np.int32),
                 desc_kf=np.full(npts, -2, np.int32), desc_index=np.full(npts, -2, np.int32), refreshed=np.zeros(npts, np.uint8),
                 normals_out=np.zeros((npts, 3), np.float32), min_distance_out=np.zeros(npts, np.float32), max_distance_out=np.zeros(npts, np.float32))
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data if v.size else None)
        arr[i].n_keyframes, arr[i].n_points, arr[i].current = nk, npts, int(p["current"])
        arr[i].target_capacity, arr[i].candidate_capacity, arr[i].op_capacity, arr[i].obs_capacity = cap["targets"], cap["candidates"], cap["ops"], cap["observations"]
        arr[i].last_level_scale = float(p["last_level_scale"])
        arr[i].inertial, arr[i].abort = int(bool(p.get("inertial", False))), int(bool(p.get("abort", False)))
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def run_search_in_neighbors_batch(arr, n_problems, cam4, bf, scale_factors, inv_level_sigma2, log_scale_factor, store=None, views=None, bounds=None,
                                  stream=0):
    """tc2li_search_in_neighbors_batch on ``store`` or, with ``views`` (the dicts ``pack_keyframe_views`` takes) and ``bounds``,
    tc2li_host_search_in_neighbors_batch -> the call's return value (no exception: the caller reads the code)."""
    c4 = np.ascontiguousarray(cam4, np.float32)
    sf, isg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    tail = [C.addressof(arr), int(n_problems), c4.ctypes.data, float(bf), sf.ctypes.data, isg.ctypes.data, len(sf), float(log_scale_factor)]
    if store is not None:
        f = lib().tc2li_search_in_neighbors_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        return f(store._handle(), *tail, C.c_void_p(stream))
    items = []
    for kf in views:
        it = dict(kf)
        it.setdefault("has_point", np.zeros(len(kf["keys"]), np.uint8))
        it.setdefault("pose7", np.float32([0, 0, 0, 1, 0, 0, 0]))
        items.append(it)
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, np.float32).reshape(-1, 4), (len(items), 4)), np.float32)
    varr, keep = pack_keyframe_views(items)
    f = lib().tc2li_host_search_in_neighbors_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float]
    rc = f(C.addressof(varr), b.ctypes.data, len(items), *tail)
    del keep
    return rc


def _neighbors_results(outs):
    res = []
    for o in outs:
        c = dict(zip(NEIGHBORS_COUNTS, [int(v) for v in o["counts"]]))
        r = dict(o, counts=c, status=c["status"], targets=o["targets"][:c["targets"]], target_fused=o["target_fused"][:c["targets"]],
                 candidates=o["candidates"][:c["candidates"]], ops=o["ops"][:c["ops"]], obs_kf_out=o["obs_kf_out"][:c["observations"]],
                 obs_index_out=o["obs_index_out"][:c["observations"]], fused_current=c["fused_current"])
        res.append(r)
    return res


def search_in_neighbors_batch(problems, cam4, bf, scale_factors, inv_level_sigma2, log_scale_factor, store=None, views=None, bounds=None, stream=0,
                              capacities=None):
    """One ``LocalMapping::SearchInNeighbors`` per problem in the reference's order (``tc2li_search_in_neighbors_batch``; with ``views`` and
    ``bounds`` in place of ``store`` the host twin) -> one dict per problem: counts (dict), status, targets, target_fused, candidates, ops
    (NEIGHBORS_OP_DTYPE), fused_current and the end state (slot_point_out, point_bad_out, point_replaced, point_nobs_out, point_found_out,
    point_visible_out, obs_offsets_out, obs_kf_out, obs_index_out, desc_kf, desc_index, refreshed, normals_out, min_distance_out,
    max_distance_out).  On TC2LI_ERR_CAPACITY the call is repeated once with the sizes ``counts`` reports."""
    for attempt in range(2):
        arr, outs, keep = pack_neighbors_problems(problems, capacities)
        rc = run_search_in_neighbors_batch(arr, len(problems), cam4, bf, scale_factors, inv_level_sigma2, log_scale_factor, store, views, bounds, stream)
        del keep
        if rc == -5 and attempt == 0 and capacities is None:   # TC2LI_ERR_CAPACITY
            capacities = [dict(targets=max(int(o["counts"][1]), 1), candidates=max(int(o["counts"][2]), 1), ops=max(int(o["counts"][3]), 1),
                               observations=max(int(o["counts"][4]), 1)) for o in outs]
            continue
        _check(rc)
        return _neighbors_results(outs)


def map_points_refresh(obs_off, descriptors, centres, positions, ref_centres, level_scale, last_scale, stream=0):
    """``MapPoint::ComputeDistinctiveDescriptors`` + ``UpdateNormalAndDepth`` for a flat list of points ->
    (best_obs, normals [n, 3], min_distance, max_distance)."""
    off = np.ascontiguousarray(obs_off, np.int32)
    n = len(off) - 1
    d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
    c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    pos, ref = np.ascontiguousarray(positions, np.float32).reshape(-1, 3), np.ascontiguousarray(ref_centres, np.float32).reshape(-1, 3)
    ls = np.ascontiguousarray(level_scale, np.float32)
    best, normals, mn, mx = np.full(max(n, 1), -1, np.int32), np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    f = lib().tc2li_map_points_refresh
    f.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 5
    _check(f(n, off.ctypes.data, d.ctypes.data if len(d) else None, c.ctypes.data if len(c) else None, pos.ctypes.data, ref.ctypes.data, ls.ctypes.data,
             float(last_scale), best.ctypes.data, normals.ctypes.data, mn.ctypes.data, mx.ctypes.data, C.c_void_p(stream)))
    return best[:n], normals[:n], mn[:n], mx[:n]


class EskfStats(C.Structure):
    """tc2li_eskf_stats"""
    _fields_ = [("calls", C.c_int32), ("effct_feat_num", C.c_int32), ("searches", C.c_int32), ("converged", C.c_int32), ("finished", C.c_int32),
                ("pad_", C.c_int32), ("res_mean_last", C.c_double)]


class LidarInertialScan(C.Structure):
    """tc2li_lidar_inertial_scan (state = tc2li_imu_state: pos 3, rot 9, vel 3, bg 3, ba 3, grav 3, offset_R_L_I 9, offset_T_L_I 3)"""
    _fields_ = [("imu", C.c_void_p), ("n_imu", C.c_int32), ("pad_", C.c_int32), ("pcl_beg_time", C.c_double), ("pcl_end_time", C.c_double),
                ("last_lidar_end_time", C.c_double), ("acc_scale", C.c_double), ("acc_s_last", C.c_double * 3), ("angvel_last", C.c_double * 3),
                ("state", C.c_double * 36), ("P", C.c_void_p), ("stats", EskfStats), ("n_preprocessed", C.c_int32), ("n_downsampled", C.c_int32)]


def eskf_predict(state36, P, Q, acc, gyr, dt):
    """One ``esekf::predict`` step (host) -> (state36, P)."""
    st = np.ascontiguousarray(state36, np.float64).copy()
    Pm = np.ascontiguousarray(P, np.float64).reshape(23, 23).copy()
    Qm = np.ascontiguousarray(Q, np.float64).reshape(12, 12)
    a, g = np.ascontiguousarray(acc, np.float64), np.ascontiguousarray(gyr, np.float64)
    f = lib().tc2li_eskf_predict
    f.argtypes = [C.c_void_p] * 5 + [C.c_double]
    _check(f(st.ctypes.data, Pm.ctypes.data, Qm.ctypes.data, a.ctypes.data, g.ctypes.data, dt))
    return st, Pm


def lidar_imu_propagate_cov(state36, P, cov12, imu7, beg, end, last_end, acc_scale, last6):
    """Forward propagation of UndistortPcl with the covariance (host) -> (end state [36], P, poses [K, 22], updated last6)."""
    st = np.ascontiguousarray(state36, np.float64).copy()
    Pm = np.ascontiguousarray(P, np.float64).reshape(23, 23).copy()
    cov = np.ascontiguousarray(cov12, np.float64)
    imu = np.ascontiguousarray(imu7, np.float64).reshape(-1, 7)
    last = np.ascontiguousarray(last6, np.float64).copy()
    poses = np.zeros((len(imu) + 2, 22))
    f = lib().tc2li_lidar_imu_propagate_cov
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_int]
    k = _check(f(st.ctypes.data, Pm.ctypes.data, cov.ctypes.data, imu.ctypes.data, len(imu), beg, end, last_end, acc_scale, last.ctypes.data,
                 last.ctypes.data + 24, poses.ctypes.data, len(poses)))
    return st, Pm, poses[:k], last


class InertialLink(C.Structure):
    """tc2li_inertial_link"""
    _fields_ = [("kf1", C.c_int32), ("kf2", C.c_int32), ("robust", C.c_int32), ("pad_", C.c_int32), ("info_scale", C.c_double),
                ("preintegrated", C.c_void_p)]


def local_inertial_bundle_adjustment(kf33, fixed, has_imu, calib24, points3, edges, link4, preintegrated, cam5, iterations=10, lambda_init=1.0,
                                     stop_flag=None, stream=0):
    """The optimisation of ``Optimizer::LocalInertialBA``.  kf33: [K, 33] = Rcw 9, tcw 3, Rwb 9, twb 3, velocity 3, gyro bias 3,
    acc bias 3 per keyframe; link4: [L, 4] = kf1, kf2, robust, info_scale; preintegrated: list of ``Preintegrated`` (one per
    link) -> (kf33, points3, chi2, depth_positive, stats)."""
    kf = np.ascontiguousarray(kf33, np.float64).copy()
    pts = np.ascontiguousarray(points3, np.float64).copy()
    fixed, has_imu = np.ascontiguousarray(fixed, np.uint8), np.ascontiguousarray(has_imu, np.uint8)
    calib24, cam5 = np.ascontiguousarray(calib24, np.float64), np.ascontiguousarray(cam5, np.float64)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    link4 = np.ascontiguousarray(link4, np.float64).reshape(-1, 4)
    links = (InertialLink * max(len(link4), 1))()
    for l, row in enumerate(link4):
        links[l] = InertialLink(int(row[0]), int(row[1]), int(row[2] != 0), 0, float(row[3]), C.addressof(preintegrated[l].p))
    chi2 = np.zeros(max(len(edges), 1))
    dpos = np.zeros(max(len(edges), 1), np.uint8)
    stats = BaStats()
    stop_ptr = stop_flag.ctypes.data if stop_flag is not None else None
    _check(lib().tc2li_local_inertial_bundle_adjustment(kf.ctypes.data, fixed.ctypes.data, has_imu.ctypes.data, len(kf), calib24.ctypes.data,
                                                        pts.ctypes.data, len(pts), edges.ctypes.data, len(edges), C.addressof(links), len(link4),
                                                        cam5.ctypes.data, iterations, lambda_init, stop_ptr, chi2.ctypes.data, dpos.ctypes.data,
                                                        C.addressof(stats), C.c_void_p(stream)))
    return kf, pts, chi2[:len(edges)], dpos[:len(edges)], stats


class PoseImuPrior(C.Structure):
    """tc2li_pose_imu_prior"""
    _fields_ = [("Rwb", C.c_double * 9), ("twb", C.c_double * 3), ("vwb", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3),
                ("H", C.c_double * 225)]


class PoseInertialProblem(C.Structure):
    """tc2li_pose_inertial_problem"""
    _fields_ = [("frame", C.c_double * 33), ("other", C.c_double * 33), ("prior", C.c_void_p), ("preintegrated", C.c_void_p),
                ("preintegrated_rw", C.c_void_p), ("Xw", C.c_void_p), ("edges", C.c_void_p), ("close_point", C.c_void_p), ("outlier", C.c_void_p),
                ("prior_out", C.c_void_p), ("n_edges", C.c_int32), ("last_frame", C.c_int32), ("rec_init", C.c_int32), ("n_initial", C.c_int32),
                ("n_bad", C.c_int32), ("n_inliers", C.c_int32), ("solver_failed", C.c_int32), ("pad_", C.c_int32)]


def pose_inertial_optimization_batch(problems, calib24, cam5, stream=0):
    """``tc2li_pose_inertial_optimization_batch``.  problems: dicts with cur33, other33 (kf33 layout), last_frame, prior246 (or None),
    pre / pre_rw (``Preintegrated``), Xw [E, 3], edges (BA_EDGE_DTYPE), close [E], rec_init
    -> per frame (cur33, other33, outlier, prior246, return value, (n_initial, n_bad, n_inliers), solver_failed)."""
    n = len(problems)
    arr = (PoseInertialProblem * max(n, 1))()
    keep = []
    for f, pr in enumerate(problems):
        Xw = np.ascontiguousarray(pr["Xw"], np.float64).reshape(-1, 3)
        e = np.ascontiguousarray(pr["edges"], BA_EDGE_DTYPE)
        cl = np.ascontiguousarray(pr["close"], np.uint8)
        out = np.zeros(max(len(e), 1), np.uint8)
        prior_in, prior_out = PoseImuPrior(), PoseImuPrior()
        if pr.get("prior246") is not None:
            C.memmove(C.addressof(prior_in), np.ascontiguousarray(pr["prior246"], np.float64).ctypes.data, 246 * 8)
        keep.append((Xw, e, cl, out, prior_in, prior_out))
        a = arr[f]
        C.memmove(a.frame, np.ascontiguousarray(pr["cur33"], np.float64).ctypes.data, 33 * 8)
        C.memmove(a.other, np.ascontiguousarray(pr["other33"], np.float64).ctypes.data, 33 * 8)
        a.prior = C.addressof(prior_in) if pr.get("prior246") is not None else None
        a.preintegrated, a.preintegrated_rw = C.addressof(pr["pre"].p), C.addressof(pr.get("pre_rw", pr["pre"]).p)
        a.Xw, a.edges, a.close_point, a.outlier, a.prior_out = Xw.ctypes.data, e.ctypes.data, cl.ctypes.data, out.ctypes.data, C.addressof(prior_out)
        a.n_edges, a.last_frame, a.rec_init = len(e), int(bool(pr.get("last_frame"))), int(bool(pr.get("rec_init")))
    res = np.zeros(max(n, 1), np.int32)
    f_ = lib().tc2li_pose_inertial_optimization_batch
    f_.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f_(C.addressof(arr), n, np.ascontiguousarray(calib24, np.float64).ctypes.data, np.ascontiguousarray(cam5, np.float64).ctypes.data, res.ctypes.data,
              C.c_void_p(stream)))
    outs = []
    for f in range(n):
        a, (Xw, e, cl, out, prior_in, prior_out) = arr[f], keep[f]
        outs.append((np.array(a.frame), np.array(a.other), out[:len(e)].copy(), np.frombuffer(bytes(prior_out), np.float64).copy(), int(res[f]),
                     (a.n_initial, a.n_bad, a.n_inliers), bool(a.solver_failed)))
    return outs


class PoseInertialBatch:
    """The IMU pre-integration between two frames and ``PoseInertialOptimizationLastFrame / LastKeyFrame`` for one frame of each of n sequences,
    packed once: ``preintegrate()`` = tc2li_imu_preintegrate_frames, ``run()`` = tc2li_pose_inertial_optimization_batch from the initial states.
    problems: dicts as for pose_inertial_optimization_batch plus samples (IMU_SAMPLE_DTYPE), t1, t2, bias6; noise4 = ng, na, ngw, naw."""

    def __init__(self, problems, calib24, cam5, noise4):
        n = self.n = len(problems)
        self.calib24, self.cam5, self.noise4 = np.ascontiguousarray(calib24, np.float64), np.ascontiguousarray(cam5, np.float64), [float(v) for v in noise4]
        self.arr = (PoseInertialProblem * n)()
        self.pre = (PreintegratedPOD * n)()
        self.bias = (ImuBias * n)()
        self.samples = np.concatenate([np.ascontiguousarray(p["samples"], IMU_SAMPLE_DTYPE) for p in problems])
        self.offsets = np.concatenate([[0], np.cumsum([len(p["samples"]) for p in problems])]).astype(np.int32)
        self.t1, self.t2 = np.array([p["t1"] for p in problems], np.float64), np.array([p["t2"] for p in problems], np.float64)
        self.keep, self.init = [], []
        self.results = np.zeros(n, np.int32)
        for f, pr in enumerate(problems):
            Xw = np.ascontiguousarray(pr["Xw"], np.float64).reshape(-1, 3)
            e = np.ascontiguousarray(pr["edges"], BA_EDGE_DTYPE)
            cl = np.ascontiguousarray(pr["close"], np.uint8)
            out = np.zeros(max(len(e), 1), np.uint8)
            prior_in, prior_out = PoseImuPrior(), PoseImuPrior()
            if pr.get("prior246") is not None:
                C.memmove(C.addressof(prior_in), np.ascontiguousarray(pr["prior246"], np.float64).ctypes.data, 246 * 8)
            self.bias[f] = ImuBias(*[float(x) for x in pr["bias6"]])
            cur, oth = np.ascontiguousarray(pr["cur33"], np.float64).copy(), np.ascontiguousarray(pr["other33"], np.float64).copy()
            self.keep.append((Xw, e, cl, out, prior_in, prior_out))
            self.init.append((cur, oth))
            a = self.arr[f]
            a.prior = C.addressof(prior_in) if pr.get("prior246") is not None else None
            a.preintegrated = a.preintegrated_rw = C.addressof(self.pre) + f * C.sizeof(PreintegratedPOD)
            a.Xw, a.edges, a.close_point, a.outlier, a.prior_out = Xw.ctypes.data, e.ctypes.data, cl.ctypes.data, out.ctypes.data, C.addressof(prior_out)
            a.n_edges, a.last_frame, a.rec_init = len(e), int(bool(pr.get("last_frame"))), int(bool(pr.get("rec_init")))
        self.init33 = np.stack([np.concatenate(x) for x in self.init])  # [n, 66]

    def preintegrate(self):
        f = lib().tc2li_imu_preintegrate_frames
        f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        return _check(f(self.n, C.addressof(self.pre), C.addressof(self.bias), *self.noise4, self.samples.ctypes.data, self.offsets.ctypes.data,
                        self.t1.ctypes.data, self.t2.ctypes.data))

    def run(self, stream=0):
        """Resets every frame to its initial state and optimises all of them -> results [n] (initial correspondences - bad)."""
        frame_off, stride = PoseInertialProblem.frame.offset, C.sizeof(PoseInertialProblem)
        base = C.addressof(self.arr)
        # frame | other are adjacent: every record's 66 doubles in one strided assignment (a loop of memmoves was interpreter time on the stage thread)
        np.frombuffer(self.arr, np.uint8).reshape(self.n, stride)[:, frame_off:frame_off + 66 * 8] = np.ascontiguousarray(self.init33).view(np.uint8).reshape(self.n, 66 * 8)
        f_ = lib().tc2li_pose_inertial_optimization_batch
        f_.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f_(base, self.n, self.calib24.ctypes.data, self.cam5.ctypes.data, self.results.ctypes.data, C.c_void_p(stream)))
        return self.results

    def inliers(self):
        return np.array([self.arr[f].n_inliers for f in range(self.n)])


class LidarInertialBatch:
    """``tc2li_lidar_inertial_frontend_batch`` with its per-scan records packed once: ``run()`` starts every sequence from its initial filter
    state and covariance again (a benchmark's repeated step).  Arguments as LidarFrontEnd.inertial_frontend_batch."""

    def __init__(self, fe, raw_offsets, maps, states36, Ps, imus, times, cov12, R=0.001, max_iter=3, limit=None, extrinsic_est_en=False,
                 point_filter_num=2, blind=2.0, time_unit_scale=1e-3, leaf=0.5):
        S = self.S = len(raw_offsets) - 1
        self.fe = fe
        self.raw_offsets = np.ascontiguousarray(raw_offsets, np.int32)
        self.st0 = np.ascontiguousarray(states36, np.float64).reshape(S, 36).copy()
        self.P0 = np.ascontiguousarray(Ps, np.float64).reshape(S, 529).copy()
        self.P = self.P0.copy()
        self.cov, self.lim = np.ascontiguousarray(cov12, np.float64), np.ascontiguousarray(np.full(23, 0.001) if limit is None else limit, np.float64)
        self.imus = [np.ascontiguousarray(x, np.float64).reshape(-1, 7) for x in imus]
        times = np.ascontiguousarray(times, np.float64).reshape(S, 4)
        self.scans = (LidarInertialScan * S)()
        for s in range(S):
            sc = self.scans[s]
            sc.imu, sc.n_imu = self.imus[s].ctypes.data, len(self.imus[s])
            sc.pcl_beg_time, sc.pcl_end_time, sc.last_lidar_end_time, sc.acc_scale = [float(v) for v in times[s]]
            sc.P = self.P[s].ctypes.data
        self.handles = (C.c_void_p * S)(*[m._h for m in maps])
        self.args = (point_filter_num, blind, time_unit_scale, leaf)
        self.tail = (R, max_iter, int(extrinsic_est_en))
        self.state_off, self.stride = LidarInertialScan.state.offset, C.sizeof(LidarInertialScan)
        self.last_off = LidarInertialScan.acc_s_last.offset
        self.zero6 = np.zeros(6)

    def prepare(self, dev_raw_ptr, stream=0, fe=None):
        """Preprocess + time-sort order of the scans into the handle ``fe`` (default: the batch's own), ahead of ``run(None, ..., fe=fe)``."""
        point_filter_num, blind, time_unit_scale, _ = self.args
        return (fe or self.fe).inertial_prepare_batch(dev_raw_ptr, self.raw_offsets, point_filter_num, blind, time_unit_scale, stream)

    def run(self, dev_raw_ptr, stream=0, fe=None):
        """dev_raw_ptr None: the scans ``prepare`` left in the handle."""
        self.P[...] = self.P0
        raw = np.frombuffer(self.scans, np.uint8).reshape(self.S, self.stride)   # the records' bytes: states and last accelerations in two strided assignments
        raw[:, self.state_off:self.state_off + 36 * 8] = self.st0.view(np.uint8).reshape(self.S, 36 * 8)
        raw[:, self.last_off:self.last_off + 48] = 0
        f = lib().tc2li_lidar_inertial_frontend_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        R, max_iter, ext = self.tail
        return _check(f((fe or self.fe)._h, self.S, C.c_void_p(dev_raw_ptr or 0), self.raw_offsets.ctypes.data, *self.args, self.handles, self.scans,
                        self.cov.ctypes.data, R, max_iter, self.lim.ctypes.data, ext, C.c_void_p(stream)))

    def states36(self):
        raw = np.frombuffer(self.scans, np.uint8).reshape(self.S, self.stride)
        return np.ascontiguousarray(raw[:, self.state_off:self.state_off + 36 * 8]).view(np.float64).reshape(self.S, 36)

    def stats(self):
        return [(sc.stats.calls, sc.stats.searches, sc.stats.effct_feat_num, sc.n_preprocessed, sc.n_downsampled) for sc in self.scans]


class LastFrame(C.Structure):
    """tc2li_last_frame: what SearchByProjection(F, LastFrame) reads of mLastFrame."""
    _fields_ = [("n", C.c_int32), ("pad_", C.c_int32), ("has_point", C.c_void_p), ("outlier", C.c_void_p), ("Xw", C.c_void_p),
                ("keys", C.c_void_p), ("descriptors", C.c_void_p), ("pose7", C.c_float * 7), ("pad2_", C.c_float)]


def pack_last_frames(items):
    """items: list of dicts with has_point, outlier, Xw, keys, descriptors, pose7 -> (ctypes array, keep-alive list)."""
    arr = (LastFrame * len(items))()
    keep = []
    for i, it in enumerate(items):
        hp = np.ascontiguousarray(it["has_point"], np.uint8); ol = np.ascontiguousarray(it["outlier"], np.uint8)
        Xw = np.ascontiguousarray(it["Xw"], np.float32); keys = np.ascontiguousarray(it["keys"], KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(it["descriptors"], np.uint8)
        keep.append((hp, ol, Xw, keys, desc))
        arr[i] = LastFrame(len(keys), 0, hp.ctypes.data, ol.ctypes.data, Xw.ctypes.data, keys.ctypes.data, desc.ctypes.data,
                           (C.c_float * 7)(*[float(x) for x in it["pose7"]]), 0.0)
    return arr, keep


def track_motion_model_batch(ext, n_frames, keypoints, u_right, last_frames, pose_pred7, cam5, b, th=7.0, stream=0, out=None):
    """``Tracking::TrackWithMotionModel`` data path for the frames of the preceding ``extract_batch_dev`` /
    ``stereo_match_batch`` calls -> (poses7 [F, 7], map_point_of_keypoint [F, capacity], n_matches [F], n_inliers [F]).
    last_frames: result of ``pack_last_frames``."""
    keypoints = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    u_right = np.ascontiguousarray(u_right, np.float32)
    pp = np.ascontiguousarray(pose_pred7, np.float32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    cap = keypoints.shape[1]
    if out is None:
        out = (np.zeros((n_frames, 7)), np.full((n_frames, cap), -1, np.int32), np.zeros(n_frames, np.int32), np.zeros(n_frames, np.int32))
    poses, mp, nm, inl = out
    arr = last_frames[0] if isinstance(last_frames, tuple) else last_frames
    _check(lib().tc2li_track_motion_model_batch(ext._h, n_frames, keypoints.ctypes.data, u_right.ctypes.data, cap, C.addressof(arr),
                                                pp.ctypes.data, cam5.ctypes.data, b, th, poses.ctypes.data, mp.ctypes.data,
                                                nm.ctypes.data, inl.ctypes.data, C.c_void_p(stream)))
    return poses, mp, nm, inl


class LidarWindow(C.Structure):
    """tc2li_lidar_window: the co-visibility window of LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:226-260)."""
    _fields_ = [("n_keyframes", C.c_int32), ("pad_", C.c_int32), ("pose_index", C.c_void_p), ("cloud_xyz", C.c_void_p),
                ("cloud_offsets", C.c_void_p), ("Tcl", C.c_float * 7), ("pad2_", C.c_float), ("weight", C.c_double)]


class LidarBaStats(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("hessian_evaluations", C.c_int32), ("residual", C.c_double), ("chi2", C.c_double)]


def _pack_lidar_window(win_pose, clouds, Tcl7, weight):
    win = np.ascontiguousarray(win_pose, np.int32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    cl = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]), np.float32)
    w = LidarWindow(len(win), 0, win.ctypes.data, cl.ctypes.data, off.ctypes.data, (C.c_float * 7)(*[float(x) for x in Tcl7]), 0.0,
                    float(weight))
    return w, (win, off, cl)  # keep the arrays alive


def local_lv_bundle_adjustment(poses7, fixed, points3, edges, cam5, win_pose, clouds, Tcl7, weight, iterations=10, lambda_init=0.0,
                               stop_flag=None, stream=0):
    """``OptimizerWithLidar::LocalLVBundleAdjustment`` with the LiDAR edge over the keyframes ``win_pose`` (rows of
    poses7) and their surface clouds -> (poses7, points3, chi2, depth_positive, stats, lidar_stats)."""
    poses = np.ascontiguousarray(poses7, np.float64).copy()
    pts = np.ascontiguousarray(points3, np.float64).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    chi2 = np.zeros(max(len(edges), 1))
    dpos = np.zeros(max(len(edges), 1), np.uint8)
    stats, lstats = BaStats(), LidarBaStats()
    stop_ptr = stop_flag.ctypes.data if stop_flag is not None else None
    w, keep = _pack_lidar_window(win_pose, clouds, Tcl7, weight)
    _check(lib().tc2li_local_lv_bundle_adjustment(poses.ctypes.data, fixed.ctypes.data, len(poses), pts.ctypes.data, len(pts),
                                                  edges.ctypes.data, len(edges), cam5.ctypes.data, iterations, lambda_init, stop_ptr,
                                                  chi2.ctypes.data, dpos.ctypes.data, C.addressof(stats), C.addressof(w),
                                                  C.addressof(lstats), C.c_void_p(stream)))
    del keep
    return poses, pts, chi2[:len(edges)], dpos[:len(edges)], stats, lstats


REDUCE_SUM, REDUCE_MAX = 0, 1
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


class BaShard(C.Structure):
    """tc2li_ba_shard"""
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("allreduce", C.c_void_p), ("ctx", C.c_void_p)]


class RcclComm:
    """An RCCL communicator made by the library (``tc2li_rccl_comm_create``): rank 0 calls ``RcclComm.unique_id()`` and hands
    the 128 bytes to the other ranks (bench.py broadcasts them over torch.distributed)."""

    def __init__(self, unique_id, rank, world):
        uid = np.ascontiguousarray(np.frombuffer(bytes(unique_id), np.uint8))
        assert uid.size == 128
        self.rank, self.world = rank, world
        self.h = C.c_void_p()
        _check(lib().tc2li_rccl_comm_create(uid.ctypes.data, rank, world, C.byref(self.h)))

    @staticmethod
    def unique_id():
        uid = np.zeros(128, np.uint8)
        _check(lib().tc2li_rccl_unique_id(uid.ctypes.data))
        return uid.tobytes()

    def shard(self):
        """tc2li_ba_shard whose all-reduce is ``tc2li_rccl_allreduce`` on this communicator (no Python on the data path)."""
        fn = C.cast(lib().tc2li_rccl_allreduce, C.c_void_p).value
        return BaShard(self.rank, self.world, fn, self.h.value)

    def close(self):
        if self.h:
            lib().tc2li_rccl_comm_destroy(self.h)
            self.h = C.c_void_p()


def torch_allreduce_shard(rank, world, group=None):
    """tc2li_ba_shard whose all-reduce is ``torch.distributed.all_reduce`` (any backend that takes device tensors) -> (shard,
    keep-alive).  The library hands the callback a device pointer; the tensor that aliases it goes through
    ``__cuda_array_interface__``."""
    import torch
    import torch.distributed as dist

    class _Alias:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

    def cb(ctx, ptr, count, op, stream):
        try:
            ext = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
            rop = dist.ReduceOp.SUM if op == REDUCE_SUM else dist.ReduceOp.MAX
            with torch.cuda.stream(ext):
                t = torch.as_tensor(_Alias(ptr, count), device="cuda")
                if dist.get_backend(group) == "gloo":  # host collective: stage through host memory, in stream order
                    h = t.cpu()
                    dist.all_reduce(h, op=rop, group=group)
                    t.copy_(h)
                else:
                    dist.all_reduce(t, op=rop, group=group)
            return 0
        except Exception as e:  # the C side turns a non-zero return into TC2LI_ERR_COMM
            print("all-reduce callback failed:", repr(e))
            return 1

    fn = ALLREDUCE_FN(cb)
    return BaShard(rank, world, C.cast(fn, C.c_void_p).value, None), fn


def ba_shard_select(edges, n_points, rank, world):
    """``tc2li_ba_shard_select`` -> (landmark_owned, edge_owned) masks of the rank."""
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    lo, eo = np.zeros(max(n_points, 1), np.uint8), np.zeros(max(len(edges), 1), np.uint8)
    _check(lib().tc2li_ba_shard_select(edges.ctypes.data, len(edges), n_points, rank, world, lo.ctypes.data, eo.ctypes.data))
    return lo[:n_points].astype(bool), eo[:len(edges)].astype(bool)


def local_lv_bundle_adjustment_sharded(shard, poses7, fixed, points3, edges, cam5, win_pose=None, clouds=None, Tcl7=None, weight=1.0,
                                       iterations=10, lambda_init=0.0, stop_flag=None, stream=0):
    """One window split over the ranks of ``shard`` (landmark partition + all-reduce of the shared-pose blocks); every rank
    passes the whole window and receives the whole result -> (poses7, points3, chi2, depth_positive, stats, lidar_stats)."""
    poses = np.ascontiguousarray(poses7, np.float64).copy()
    pts = np.ascontiguousarray(points3, np.float64).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    chi2 = np.zeros(max(len(edges), 1))
    dpos = np.zeros(max(len(edges), 1), np.uint8)
    stats, lstats = BaStats(), LidarBaStats()
    stop_ptr = stop_flag.ctypes.data if stop_flag is not None else None
    w, keep = (None, None) if win_pose is None else _pack_lidar_window(win_pose, clouds, Tcl7, weight)
    _check(lib().tc2li_local_lv_bundle_adjustment_sharded(poses.ctypes.data, fixed.ctypes.data, len(poses), pts.ctypes.data, len(pts),
                                                          edges.ctypes.data, len(edges), cam5.ctypes.data, iterations, lambda_init, stop_ptr,
                                                          chi2.ctypes.data, dpos.ctypes.data, C.addressof(stats),
                                                          C.addressof(w) if w is not None else None, C.addressof(lstats),
                                                          C.addressof(shard), C.c_void_p(stream)))
    del keep
    return poses, pts, chi2[:len(edges)], dpos[:len(edges)], stats, lstats


class BaProblem(C.Structure):
    """tc2li_ba_problem"""
    _fields_ = [("poses7", C.c_void_p), ("fixed", C.c_void_p), ("points3", C.c_void_p), ("edges", C.c_void_p), ("n_poses", C.c_int32),
                ("n_points", C.c_int32), ("n_edges", C.c_int32), ("iterations", C.c_int32), ("lambda_init", C.c_double),
                ("stop_flag", C.c_void_p), ("edge_chi2", C.c_void_p), ("edge_depth_positive", C.c_void_p), ("stats", C.c_void_p),
                ("lidar", C.c_void_p), ("lidar_stats", C.c_void_p)]


class BaBatch:
    """A set of independent local-BA windows prepared once (arrays pinned down for the C side) and optimised together by
    ``tc2li_local_bundle_adjustment_batch``.  windows: dicts with poses, fixed, points, edges (BA_EDGE_DTYPE) and optionally
    win_pose, clouds, Tcl7, weight; iterations / lambda_init per window optional."""

    def __init__(self, windows, cam5):
        self.n = len(windows)
        self.cam5 = np.ascontiguousarray(cam5, np.float64)
        self.arr = (BaProblem * self.n)()
        self.init = []
        self.keep = []
        self.stats = (BaStats * self.n)()
        self.lstats = (LidarBaStats * self.n)()
        self.results = np.zeros(self.n, np.int32)
        for i, w in enumerate(windows):
            poses0 = np.ascontiguousarray(w["poses"], np.float64); pts0 = np.ascontiguousarray(w["points"], np.float64)
            poses, pts = poses0.copy(), pts0.copy()
            fixed = np.ascontiguousarray(w["fixed"], np.uint8)
            edges = np.ascontiguousarray(w["edges"], BA_EDGE_DTYPE)
            chi2, dpos = np.zeros(max(len(edges), 1)), np.zeros(max(len(edges), 1), np.uint8)
            lw = None
            if w.get("win_pose") is not None:
                lw = _pack_lidar_window(w["win_pose"], w["clouds"], w["Tcl7"], w.get("weight", 1.0))
            stop = w.get("stop_flag")   # (a uint8 array of one element the caller may set while the window is optimised: *pbStopFlag)
            self.init.append((poses0, pts0))
            self.keep.append((poses, pts, fixed, edges, chi2, dpos, lw, stop))
            self.arr[i] = BaProblem(poses.ctypes.data, fixed.ctypes.data, pts.ctypes.data, edges.ctypes.data, len(poses), len(pts), len(edges),
                                    int(w.get("iterations", 10)), float(w.get("lambda_init", 0.0)), stop.ctypes.data if stop is not None else None,
                                    chi2.ctypes.data, dpos.ctypes.data,
                                    C.addressof(self.stats) + i * C.sizeof(BaStats), C.addressof(lw[0]) if lw else None,
                                    C.addressof(self.lstats) + i * C.sizeof(LidarBaStats))

    def run(self, max_concurrency=8):
        """Resets every window to its initial estimate and optimises all of them -> number of successful windows."""
        for (p0, x0), k in zip(self.init, self.keep):
            k[0][...] = p0
            k[1][...] = x0
        return _check(lib().tc2li_local_bundle_adjustment_batch(C.addressof(self.arr), self.n, self.cam5.ctypes.data, max_concurrency,
                                                                self.results.ctypes.data))

    def run_group(self, group):
        """The same as ONE lock-step group on the library's context `group` (tc2li_local_bundle_adjustment_batch_group): for callers with
        several mapping workers, each on a group of its own."""
        for (p0, x0), k in zip(self.init, self.keep):
            k[0][...] = p0
            k[1][...] = x0
        return _check(lib().tc2li_local_bundle_adjustment_batch_group(C.addressof(self.arr), self.n, self.cam5.ctypes.data, int(group),
                                                                      self.results.ctypes.data))

    def reset(self):
        for (p0, x0), k in zip(self.init, self.keep):
            k[0][...] = p0
            k[1][...] = x0

    def result(self, i):
        k = self.keep[i]
        return k[0], k[1], k[4][:len(k[3])], k[5][:len(k[3])], self.stats[i], self.lstats[i]


class BaEngine:
    """``tc2li_ba_engine``: a running lock-step queue with up to ``max_windows`` local-BA windows in flight; windows join and leave it
    one by one.  submit(batch) -> ticket (the BaBatch's arrays must stay alive until wait(ticket))."""

    def __init__(self, cam5, max_windows=192):
        self.cam5 = np.ascontiguousarray(cam5, np.float64)
        self.h = C.c_void_p()
        _check(lib().tc2li_ba_engine_create(self.cam5.ctypes.data, int(max_windows), C.byref(self.h)))

    def submit(self, batch, first=0, count=None):
        """Resets the windows [first, first + count) of the BaBatch to their initial estimates and hands them to the engine."""
        count = batch.n - first if count is None else count
        for (p0, x0), k in zip(batch.init[first:first + count], batch.keep[first:first + count]):
            k[0][...] = p0
            k[1][...] = x0
        t = lib().tc2li_ba_engine_submit(self.h, C.addressof(batch.arr) + first * C.sizeof(BaProblem), count,
                                         batch.results.ctypes.data + 4 * first)
        if t < 0:
            _check(int(t))
        return t

    def wait(self, ticket):
        return _check(lib().tc2li_ba_engine_wait(self.h, ticket))

    def done(self, ticket):
        """True when wait(ticket) will not block."""
        return _check(lib().tc2li_ba_engine_poll(self.h, ticket)) == 1

    def close(self):
        if self.h:
            lib().tc2li_ba_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lidar_planes_host(poses7, win_pose, clouds, Tcl7, capacity=20000):
    """Host-only plane extraction of the LiDAR window -> (clusters [n, W, 10] = P00 P01 P02 P11 P12 P22 v N, coe [n])."""
    poses = np.ascontiguousarray(poses7, np.float64)
    w, keep = _pack_lidar_window(win_pose, clouds, Tcl7, 1.0)
    out, coe = np.zeros((capacity, w.n_keyframes, 10)), np.zeros(capacity)
    n = _check(lib().tc2li_host_lidar_planes(poses.ctypes.data, len(poses), C.addressof(w), out.ctypes.data, coe.ctypes.data, capacity))
    del keep
    return out[:n].copy(), coe[:n].copy()


def lidar_planes_device(poses7, win_pose, clouds, Tcl7, capacity=2048):
    """The same planes from the extraction kernels of the batched local BA (``tc2li_device_lidar_planes``) ->
    (clusters [n, W, 10], coe [n], info [4] = planes, declined, root voxels, planes found)."""
    poses = np.ascontiguousarray(poses7, np.float64)
    w, keep = _pack_lidar_window(win_pose, clouds, Tcl7, 1.0)
    out, coe, info = np.zeros((capacity, w.n_keyframes, 10)), np.zeros(capacity), np.zeros(4, np.int32)
    n = _check(lib().tc2li_device_lidar_planes(poses.ctypes.data, len(poses), C.addressof(w), out.ctypes.data, coe.ctypes.data, capacity, info.ctypes.data))
    del keep
    return out[:n].copy(), coe[:n].copy(), info


def local_lvi_bundle_adjustment(kf33, fixed, has_imu, calib24, points3, edges, link4, preintegrated, cam5, win_kf, clouds, Tcl7, Tbl7, weight,
                                iterations=10, lambda_init=1.0, stop_flag=None, stream=0):
    """``OptimizerWithLidar::LocalLVIBA``: local_inertial_bundle_adjustment plus the LiDAR edge over the keyframes ``win_kf``
    (rows of kf33) -> (kf33, points3, chi2, depth_positive, stats, lidar_stats)."""
    kf = np.ascontiguousarray(kf33, np.float64).copy()
    pts = np.ascontiguousarray(points3, np.float64).copy()
    fixed, has_imu = np.ascontiguousarray(fixed, np.uint8), np.ascontiguousarray(has_imu, np.uint8)
    calib24, cam5 = np.ascontiguousarray(calib24, np.float64), np.ascontiguousarray(cam5, np.float64)
    edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    link4 = np.ascontiguousarray(link4, np.float64).reshape(-1, 4)
    links = (InertialLink * max(len(link4), 1))()
    for l, row in enumerate(link4):
        links[l] = InertialLink(int(row[0]), int(row[1]), int(row[2] != 0), 0, float(row[3]), C.addressof(preintegrated[l].p))
    chi2 = np.zeros(max(len(edges), 1))
    dpos = np.zeros(max(len(edges), 1), np.uint8)
    stats, lstats = BaStats(), LidarBaStats()
    stop_ptr = stop_flag.ctypes.data if stop_flag is not None else None
    w, keep = _pack_lidar_window(win_kf, clouds, Tcl7, weight)
    tbl = np.ascontiguousarray(Tbl7, np.float32)
    f = lib().tc2li_local_lvi_bundle_adjustment
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(kf.ctypes.data, fixed.ctypes.data, has_imu.ctypes.data, len(kf), calib24.ctypes.data, pts.ctypes.data, len(pts), edges.ctypes.data,
             len(edges), C.addressof(links), len(link4), cam5.ctypes.data, iterations, lambda_init, stop_ptr, chi2.ctypes.data, dpos.ctypes.data,
             C.addressof(stats), C.addressof(w), tbl.ctypes.data, C.addressof(lstats), C.c_void_p(stream)))
    del keep
    return kf, pts, chi2[:len(edges)], dpos[:len(edges)], stats, lstats


class LviProblem(C.Structure):
    """tc2li_lvi_problem"""
    _fields_ = [("keyframes", C.c_void_p), ("fixed", C.c_void_p), ("has_imu", C.c_void_p), ("points3", C.c_void_p), ("edges", C.c_void_p), ("links", C.c_void_p),
                ("n_keyframes", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("n_links", C.c_int32), ("iterations", C.c_int32), ("pad_", C.c_int32),
                ("lambda_init", C.c_double), ("stop_flag", C.c_void_p), ("edge_chi2", C.c_void_p), ("edge_depth_positive", C.c_void_p), ("stats", C.c_void_p),
                ("lidar", C.c_void_p), ("Tbl", C.c_void_p), ("lidar_stats", C.c_void_p)]


class LviBatch:
    """A set of independent ``LocalLVIBA`` windows prepared once and optimised together by ``tc2li_local_lvi_bundle_adjustment_batch``.
    windows: dicts with kf33, fixed, has_imu, points, edges (BA_EDGE_DTYPE), link4, pre (list of Preintegrated) and optionally win_kf, clouds,
    Tcl7, Tbl7, weight; iterations / lambda_init per window optional (10, 1.0)."""

    def __init__(self, windows, calib24, cam5):
        self.n = len(windows)
        self.calib24, self.cam5 = np.ascontiguousarray(calib24, np.float64), np.ascontiguousarray(cam5, np.float64)
        self.arr = (LviProblem * self.n)()
        self.init, self.keep = [], []
        self.stats = (BaStats * self.n)()
        self.lstats = (LidarBaStats * self.n)()
        self.results = np.zeros(self.n, np.int32)
        for i, w in enumerate(windows):
            kf0, pts0 = np.ascontiguousarray(w["kf33"], np.float64), np.ascontiguousarray(w["points"], np.float64)
            kf, pts = kf0.copy(), pts0.copy()
            fixed, has_imu = np.ascontiguousarray(w["fixed"], np.uint8), np.ascontiguousarray(w["has_imu"], np.uint8)
            edges = np.ascontiguousarray(w["edges"], BA_EDGE_DTYPE)
            link4 = np.ascontiguousarray(w["link4"], np.float64).reshape(-1, 4)
            links = (InertialLink * max(len(link4), 1))()
            for l, row in enumerate(link4):
                links[l] = InertialLink(int(row[0]), int(row[1]), int(row[2] != 0), 0, float(row[3]), C.addressof(w["pre"][l].p))
            chi2, dpos = np.zeros(max(len(edges), 1)), np.zeros(max(len(edges), 1), np.uint8)
            lw, tbl = None, None
            if w.get("win_kf") is not None:
                lw = _pack_lidar_window(w["win_kf"], w["clouds"], w["Tcl7"], w.get("weight", 1.0))
                tbl = np.ascontiguousarray(w["Tbl7"], np.float32)
            self.init.append((kf0, pts0))
            self.keep.append((kf, pts, fixed, has_imu, edges, links, chi2, dpos, lw, tbl, w["pre"]))
            self.arr[i] = LviProblem(kf.ctypes.data, fixed.ctypes.data, has_imu.ctypes.data, pts.ctypes.data, edges.ctypes.data, C.addressof(links),
                                     len(kf), len(pts), len(edges), len(link4), int(w.get("iterations", 10)), 0, float(w.get("lambda_init", 1.0)), None,
                                     chi2.ctypes.data, dpos.ctypes.data, C.addressof(self.stats) + i * C.sizeof(BaStats),
                                     C.addressof(lw[0]) if lw else None, tbl.ctypes.data if lw else None,
                                     C.addressof(self.lstats) + i * C.sizeof(LidarBaStats))

    def run(self, max_concurrency=8):
        """Resets every window to its initial estimate and optimises all of them -> number of successful windows."""
        for (k0, x0), k in zip(self.init, self.keep):
            k[0][...] = k0
            k[1][...] = x0
        f = lib().tc2li_local_lvi_bundle_adjustment_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return _check(f(C.addressof(self.arr), self.n, self.calib24.ctypes.data, self.cam5.ctypes.data, max_concurrency, self.results.ctypes.data))

    def run_group(self, group):
        """The same as ONE lock-step group on the library's context `group` (tc2li_local_lvi_bundle_adjustment_batch_group): for callers with several
        mapping workers, each on a group of its own."""
        for (k0, x0), k in zip(self.init, self.keep):
            k[0][...] = k0
            k[1][...] = x0
        f = lib().tc2li_local_lvi_bundle_adjustment_batch_group
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return _check(f(C.addressof(self.arr), self.n, self.calib24.ctypes.data, self.cam5.ctypes.data, int(group), self.results.ctypes.data))

    def result(self, i):
        k = self.keep[i]
        return k[0], k[1], k[6][:len(k[4])], k[7][:len(k[4])], self.stats[i], self.lstats[i]


def lidar_window_evaluate(poses7, win_pose, clouds, Tcl7, derivatives=True):
    """The LiDAR edge alone -> (n_planes, residual, JacT [6W], Hessian [6W, 6W]) (ComputeError / ComputeJandHSE3)."""
    poses = np.ascontiguousarray(poses7, np.float64)
    w, keep = _pack_lidar_window(win_pose, clouds, Tcl7, 1.0)
    W = w.n_keyframes
    res = C.c_double(0)
    J, H = np.zeros(6 * W), np.zeros((6 * W, 6 * W))
    n = _check(lib().tc2li_lidar_window_evaluate(poses.ctypes.data, len(poses), C.addressof(w), C.addressof(res),
                                                 J.ctypes.data if derivatives else None, H.ctypes.data if derivatives else None, None))
    del keep
    return n, res.value, J, H


# ---- projection matching (ORBmatcher::SearchByProjection) ----------------------------------------------------------
QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("u_right", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                        ("angle", "<f4"), ("valid", "<i2"), ("has_observations", "<i2"), ("descriptor", "u1", (32,))])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                            ("max_distance_raw", "<f4"), ("descriptor", "u1", (32,))])


class FrameView(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p), ("occupied", C.c_void_p), ("n", C.c_int32),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


def search_by_projection(keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio=0.9, check_orientation=False):
    """The matching loops of both tracking overloads -> (nmatches, match_of_query, query_of_keypoint)."""
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    ur = np.ascontiguousarray(u_right, np.float32)
    occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
    queries = np.ascontiguousarray(queries, QUERY_DTYPE)
    fv = FrameView(keys.ctypes.data, desc.ctypes.data, ur.ctypes.data, None if occ is None else occ.ctypes.data, len(keys), 0.0,
                   float(cols), 0.0, float(rows))
    match = np.full(max(len(queries), 1), -1, np.int32)
    qok = np.full(max(len(keys), 1), -1, np.int32)
    n = _check(lib().tc2li_search_by_projection(C.byref(fv), queries.ctypes.data, len(queries), mode, nn_ratio, int(check_orientation),
                                                match.ctypes.data, qok.ctypes.data))
    return n, match[:len(queries)], qok[:len(keys)]


def project_last_frame(pose_cur7, pose_last7, cam4, b, bf, scales, cols, rows, has_point, outlier, Xw, last_keys, mp_desc, th, mono=False):
    pc, pl, cam4 = [np.ascontiguousarray(a, np.float32) for a in (pose_cur7, pose_last7, cam4)]
    scales = np.ascontiguousarray(scales, np.float32)
    hp, ol = np.ascontiguousarray(has_point, np.uint8), np.ascontiguousarray(outlier, np.uint8)
    Xw = np.ascontiguousarray(Xw, np.float32)
    last_keys = np.ascontiguousarray(last_keys, KEYPOINT_DTYPE)
    mp_desc = np.ascontiguousarray(mp_desc, np.uint8)
    out = np.zeros(max(len(last_keys), 1), QUERY_DTYPE)
    _check(lib().tc2li_project_last_frame(pc.ctypes.data, pl.ctypes.data, cam4.ctypes.data, b, bf, scales.ctypes.data, len(scales), cols,
                                          rows, len(last_keys), hp.ctypes.data, ol.ctypes.data, Xw.ctypes.data, last_keys.ctypes.data,
                                          mp_desc.ctypes.data, th, int(mono), out.ctypes.data))
    return out[:len(last_keys)]


def project_local_map(pose7, cam4, bf, scales, log_scale, cols, rows, points, th, far_points=False, th_far=0.0, cos_limit=0.5):
    pose7, cam4, scales = [np.ascontiguousarray(a, np.float32) for a in (pose7, cam4, scales)]
    points = np.ascontiguousarray(points, MAP_POINT_DTYPE)
    out = np.zeros(max(len(points), 1), QUERY_DTYPE)
    _check(lib().tc2li_project_local_map(pose7.ctypes.data, cam4.ctypes.data, bf, scales.ctypes.data, len(scales), log_scale, cols, rows,
                                         len(points), points.ctypes.data, th, int(far_points), th_far, cos_limit, out.ctypes.data))
    return out[:len(points)]


# ---- local-map bookkeeping (Tracking::UpdateLocalKeyFrames / UpdateLocalPoints) ---------------------------------------------
class MapGraph(C.Structure):
    """tc2li_map_graph"""
    _fields_ = [("n_keyframes", C.c_int32), ("n_points", C.c_int32), ("kf_bad", C.c_void_p), ("covis_offsets", C.c_void_p), ("covis", C.c_void_p),
                ("child_offsets", C.c_void_p), ("children", C.c_void_p), ("parent", C.c_void_p), ("prev_kf", C.c_void_p),
                ("match_offsets", C.c_void_p), ("matches", C.c_void_p), ("point_bad", C.c_void_p), ("obs_offsets", C.c_void_p), ("obs_kf", C.c_void_p)]


def map_graph(graph):
    """dict of flat arrays (see LocalMap) -> (MapGraph, the arrays it points into: keep them alive as long as it is used)"""
    g = {k: np.ascontiguousarray(v, np.uint8 if k in ("kf_bad", "point_bad") else np.int32) for k, v in graph.items()}
    ptr = lambda k: g[k].ctypes.data if g[k].size else None
    mg = MapGraph(len(g["kf_bad"]), len(g["point_bad"]), ptr("kf_bad"), ptr("covis_off"), ptr("covis"), ptr("child_off"), ptr("children"),
                  ptr("parent"), ptr("prev_kf"), ptr("match_off"), ptr("matches"), ptr("point_bad"), ptr("obs_off"), ptr("obs_kf"))
    return mg, g


class LocalMap:
    """Device-resident mirror of the keyframe graph (``tc2li_local_map``) and ``Tracking::UpdateLocalMap`` on it.  graph: dict of flat
    arrays kf_bad, covis_off, covis, child_off, children, parent, prev_kf, match_off, matches, point_bad, obs_off, obs_kf."""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().tc2li_local_map_create(C.byref(self.h)))
        self.n_keyframes = self.n_points = 0

    def set_graph(self, graph, stream=0):
        mg, keep = map_graph(graph)
        _check(lib().tc2li_local_map_set_graph(self.h, C.addressof(mg), C.c_void_p(stream)))
        del keep
        self.n_keyframes, self.n_points = mg.n_keyframes, mg.n_points

    def update(self, frame_points, temporal_last_kf=-1, stream=0, keyframe_capacity=None, point_capacity=None):
        """-> (local keyframes, reference keyframe, local points, frame points cleared)"""
        fp = np.ascontiguousarray(frame_points, np.int32)
        kc = self.n_keyframes if keyframe_capacity is None else keyframe_capacity
        pc = self.n_points if point_capacity is None else point_capacity
        kfs, pts = np.zeros(max(kc, 1), np.int32), np.zeros(max(pc, 1), np.int32)
        cleared = np.zeros(max(len(fp), 1), np.uint8)
        n_k, n_p, ref = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        _check(lib().tc2li_local_map_update(self.h, fp.ctypes.data if len(fp) else None, len(fp), int(temporal_last_kf), kfs.ctypes.data, kc,
                                            C.addressof(n_k), C.addressof(ref), pts.ctypes.data, pc, C.addressof(n_p),
                                            cleared.ctypes.data if len(fp) else None, C.c_void_p(stream)))
        return kfs[:n_k.value].copy(), ref.value, pts[:n_p.value].copy(), cleared[:len(fp)].astype(bool)

    def close(self):
        if self.h:
            lib().tc2li_local_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalMapUpdateProblem(C.Structure):
    """tc2li_local_map_update_problem"""
    _fields_ = [("map", C.c_void_p), ("graph", C.c_void_p), ("frame_points", C.c_void_p), ("n_frame_points", C.c_int32), ("temporal_last_kf", C.c_int32),
                ("counts", C.c_void_p), ("local_keyframes", C.c_void_p), ("local_points", C.c_void_p), ("frame_point_cleared", C.c_void_p),
                ("keyframe_capacity", C.c_int32), ("point_capacity", C.c_int32)]


_LOCAL_MAP_COUNTS = ("n_keyframes", "n_voted", "reference_kf", "n_points", "n_cleared")


def local_map_limits():
    """tc2li_local_map_limits -> {lds_keyframes, point_workgroups, threads}: the sizes at which the device path of local_map_update_batch
    changes (the vote counters and marks leave LDS above lds_keyframes keyframes; a problem's point phase is cut into point_workgroups slices)."""
    out = (C.c_int32 * 3)()
    f = lib().tc2li_local_map_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 3))
    return dict(zip(("lds_keyframes", "point_workgroups", "threads"), [int(v) for v in out]))


def pack_local_map_problems(problems, fill=0):
    """The tc2li_local_map_update_problem array of a batch with its output arrays (prefilled with `fill`) -> (array, outputs per problem, what
    must stay alive).  A problem is a dict with frame_points, optionally temporal_last_kf (-1), keyframe_capacity / point_capacity (by default
    the graph's sizes, which can never be too small) and ``map`` (a LocalMap with its graph set: the device entry) and / or ``graph`` (the dict
    of flat arrays LocalMap.set_graph takes: the host entry)."""
    P = len(problems)
    arr, outs, keep = (LocalMapUpdateProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        fp = np.ascontiguousarray(p["frame_points"], np.int32).reshape(-1)
        lm, mg, nk, npts = p.get("map"), None, 0, 0
        if lm is not None:
            arr[i].map, nk, npts = lm.h, lm.n_keyframes, lm.n_points
        if p.get("graph") is not None:
            mg, g = map_graph(p["graph"])
            keep.append((mg, g))
            arr[i].graph, nk, npts = C.addressof(mg), mg.n_keyframes, mg.n_points
        kc, pc = int(p.get("keyframe_capacity", nk)), int(p.get("point_capacity", npts))
        full = lambda n, t: np.full(max(n, 1), fill, np.int64).astype(t)
        o = dict(counts=full(8, np.int32), local_keyframes=full(kc, np.int32), local_points=full(pc, np.int32), frame_point_cleared=full(len(fp), np.uint8))
        arr[i].frame_points = fp.ctypes.data if len(fp) else None
        arr[i].n_frame_points, arr[i].temporal_last_kf = len(fp), int(p.get("temporal_last_kf", -1))
        arr[i].counts, arr[i].local_keyframes, arr[i].local_points = o["counts"].ctypes.data, o["local_keyframes"].ctypes.data, o["local_points"].ctypes.data
        arr[i].frame_point_cleared = o["frame_point_cleared"].ctypes.data if len(fp) else None
        arr[i].keyframe_capacity, arr[i].point_capacity = kc, pc
        keep.append(fp)
        outs.append(o)
    return arr, outs, keep


def run_local_map_update_batch(arr, n_problems, host=False, stream=0):
    """tc2li_local_map_update_batch / tc2li_host_local_map_update_batch on a packed array -> the call's return value; raises Tc2liError"""
    if host:
        f = lib().tc2li_host_local_map_update_batch
        f.argtypes = [C.c_void_p, C.c_int]
        return _check(f(C.addressof(arr), n_problems))
    f = lib().tc2li_local_map_update_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return _check(f(C.addressof(arr), n_problems, C.c_void_p(stream)))


def _local_map_results(problems, outs):
    res = []
    for p, o in zip(problems, outs):
        c = dict(zip(_LOCAL_MAP_COUNTS, [int(v) for v in o["counts"][:5]]))
        n = len(np.asarray(p["frame_points"]).reshape(-1))
        res.append(dict(c, keyframes=o["local_keyframes"][:c["n_keyframes"]], points=o["local_points"][:c["n_points"]],
                        cleared=o["frame_point_cleared"][:n].astype(bool)))
    return res


def local_map_update_batch(problems, stream=0, host=False):
    """One ``Tracking::UpdateLocalMap`` per problem in one device call (``tc2li_local_map_update_batch``).  problems: dicts with ``map`` (a
    LocalMap), frame_points and optionally temporal_last_kf, keyframe_capacity, point_capacity -> one dict per problem: keyframes, points,
    cleared (cut to their counts), reference_kf, n_voted, n_keyframes, n_points, n_cleared."""
    arr, outs, keep = pack_local_map_problems(problems)
    run_local_map_update_batch(arr, len(problems), host, stream)
    del keep
    return _local_map_results(problems, outs)


def host_local_map_update_batch(problems):
    """``tc2li_host_local_map_update_batch``: the same on the CPU over each problem's ``graph`` (dict of flat arrays); needs no device."""
    return local_map_update_batch(problems, host=True)


def local_map_set_graph_batch(maps, graphs, stream=0):
    """``tc2li_local_map_set_graph_batch``: LocalMap.set_graph for every (map, graph) pair with one wait; no mirror changes if a graph is
    refused."""
    n = len(maps)
    if len(graphs) != n:
        raise ValueError("as many graphs as maps are needed")
    packed = [map_graph(g) for g in graphs]
    mgs, hs = (MapGraph * max(n, 1))(), (C.c_void_p * max(n, 1))()
    for i, (mg, _) in enumerate(packed):
        mgs[i], hs[i] = mg, maps[i].h
    f = lib().tc2li_local_map_set_graph_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    _check(f(C.addressof(hs), C.addressof(mgs), n, C.c_void_p(stream)))
    for m, (mg, _) in zip(maps, packed):
        m.n_keyframes, m.n_points = mg.n_keyframes, mg.n_points
    del packed


# ---- ORB vocabulary (DBoW2): Frame::ComputeBoW / KeyFrame::ComputeBoW, ORBmatcher::SearchByBoW(KeyFrame*, Frame&) ----------------------
class BowOut(C.Structure):
    """tc2li_bow_out"""
    _fields_ = [(name, C.c_void_p) for name in ("word", "node", "n_words", "bow_word", "bow_value", "n_nodes", "fv_node", "fv_offset", "fv_index")]


class BowPair(C.Structure):
    """tc2li_bow_pair"""
    _fields_ = [("keyframe", KeyframeView), ("frame", KeyframeView), ("nn_ratio", C.c_float), ("check_orientation", C.c_int32)]


def _bow_arrays(total, n_frames):
    a = dict(word=np.full(total, -1, np.int32), node=np.full(total, -1, np.int32), n_words=np.zeros(n_frames, np.int32),
             bow_word=np.full(total, -1, np.int32), bow_value=np.zeros(total, np.float64), n_nodes=np.zeros(n_frames, np.int32),
             fv_node=np.full(total, -1, np.int32), fv_offset=np.full(total + n_frames, -1, np.int32), fv_index=np.full(total, -1, np.int32))
    s = BowOut(*[a[f].ctypes.data for f, _ in BowOut._fields_])
    return a, s


def _bow_frames(a, bases, counts):
    """Splits the batch arrays into per-frame dicts: word / node [n], bow_word / bow_value (mBowVec), fv_node / fv_offset / fv_index
    (mFeatVec, the slices a tc2li_keyframe_view points at)."""
    out = []
    for f, (b, n) in enumerate(zip(bases, counts)):
        nw, nn = int(a["n_words"][f]), int(a["n_nodes"][f])
        fo = a["fv_offset"][b + f:b + f + nn + 1]
        out.append(dict(word=a["word"][b:b + n], node=a["node"][b:b + n], bow_word=a["bow_word"][b:b + nw], bow_value=a["bow_value"][b:b + nw],
                        fv_node=a["fv_node"][b:b + nn], fv_offset=fo, fv_index=a["fv_index"][b:b + int(fo[-1])]))
    return out


class Vocabulary:
    """``ORBVocabulary`` (DBoW2 TemplatedVocabulary<FORB>): ``load_text`` / ``from_arrays`` build it on the host (no GPU needed),
    ``transform`` / ``transform_orb`` are ``ComputeBoW`` on the device."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load_text(cls, path):
        h = C.c_void_p()
        f = lib().tc2li_vocabulary_load_text
        f.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        _check(f(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, k, L, scoring, weighting, parent, is_leaf, descriptors, weights):
        """Nodes 1 .. n in file order (the root has no entry)."""
        p = np.ascontiguousarray(parent, np.int32); lf = np.ascontiguousarray(is_leaf, np.int32)
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32); w = np.ascontiguousarray(weights, np.float64)
        h = C.c_void_p()
        f = lib().tc2li_vocabulary_create
        f.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)]
        _check(f(k, L, scoring, weighting, len(p), p.ctypes.data, lf.ctypes.data, d.ctypes.data, w.ctypes.data, C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "_h", None):
            f = lib().tc2li_vocabulary_destroy
            f.argtypes = [C.c_void_p]
            f.restype = None
            f(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{k, L, scoring, weighting, nodes, words}"""
        out = (C.c_int32 * 6)()
        f = lib().tc2li_vocabulary_info
        f.argtypes = [C.c_void_p, C.c_void_p]
        _check(f(self._h, out))
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words"), [int(v) for v in out]))

    def nodes(self):
        """(parent, word_id, descriptors [n, 32], weight) per node, root first."""
        n = self.info()["nodes"]
        p, wid, d, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.zeros(n)
        f = lib().tc2li_vocabulary_nodes
        f.argtypes = [C.c_void_p] * 5
        _check(f(self._h, p.ctypes.data, wid.ctypes.data, d.ctypes.data, w.ctypes.data))
        return p, wid, d, w

    def transform(self, descriptors_per_frame, levelsup=4, stream=0):
        """``TemplatedVocabulary::transform`` of every frame's host descriptors -> list of per-frame dicts (see ``_bow_frames``)."""
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptors_per_frame]
        offs = np.concatenate([[0], np.cumsum([len(d) for d in ds])]).astype(np.int32)
        alld = np.ascontiguousarray(np.concatenate(ds) if ds else np.zeros((0, 32), np.uint8))
        a, s = _bow_arrays(max(int(offs[-1]), 1), len(ds))
        f = lib().tc2li_vocabulary_transform_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(self._h, len(ds), alld.ctypes.data, offs.ctypes.data, int(levelsup), C.byref(s), C.c_void_p(stream)))
        return _bow_frames(a, offs[:-1], np.diff(offs))

    def transform_orb(self, ext, n_keypoints, capacity=None, levelsup=4, stream=0, raw=False):
        """``ComputeBoW`` of frames 0 .. len(n_keypoints) - 1 of the extractor's last ``extract_batch_dev`` call (image 2f, with
        n_keypoints[f] keypoints: the counts that call returned for the even images), on the device-resident descriptors -> list of
        per-frame dicts, or with raw=True the batch arrays (slots at f * capacity)."""
        n_frames = len(n_keypoints)
        capacity = ext.capacity if capacity is None else capacity
        a, s = _bow_arrays(max(n_frames * capacity, 1), n_frames)
        f = lib().tc2li_orb_compute_bow_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(ext._h, self._h, n_frames, int(levelsup), capacity, C.byref(s), C.c_void_p(stream)))
        if raw:
            return a
        return _bow_frames(a, [i * capacity for i in range(n_frames)], [int(n) for n in n_keypoints])


def search_by_bow_batch(pairs, capacity=None, stream=0):
    """``ORBmatcher::SearchByBoW(KeyFrame*, Frame&)`` for a list of pairs; each pair is a dict with ``keyframe`` and ``frame`` (dicts as
    ``pack_keyframe_views`` takes: keys, descriptors, has_point (keyframe), fv_node / fv_offset / fv_index), ``nn_ratio`` and
    ``check_orientation`` -> (kf_keypoint_of_keypoint [n_pairs, capacity], n_matches [n_pairs])."""
    views, keep = [], []
    for p in pairs:
        for side in ("keyframe", "frame"):
            it = dict(p[side])
            n = len(it["keys"])
            it.setdefault("u_right", np.full(n, -1, np.float32)); it.setdefault("depth", np.full(n, -1, np.float32))
            it.setdefault("has_point", np.zeros(n, np.uint8)); it.setdefault("pose7", [0, 0, 0, 1, 0, 0, 0])
            views.append(it)
    arr, keep = pack_keyframe_views(views)
    if capacity is None:
        capacity = max([len(p["frame"]["keys"]) for p in pairs] + [1])
    bp = (BowPair * max(len(pairs), 1))()
    for i, p in enumerate(pairs):
        bp[i].keyframe, bp[i].frame = arr[2 * i], arr[2 * i + 1]
        bp[i].nn_ratio, bp[i].check_orientation = float(p.get("nn_ratio", 0.7)), int(bool(p.get("check_orientation", True)))
    match = np.full((max(len(pairs), 1), capacity), -1, np.int32)
    nm = np.zeros(max(len(pairs), 1), np.int32)
    f = lib().tc2li_search_by_bow_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(C.addressof(bp), len(pairs), capacity, match.ctypes.data, nm.ctypes.data, C.c_void_p(stream)))
    del keep
    return match[:len(pairs)], nm[:len(pairs)]


class ReferenceKeyframe(C.Structure):
    """tc2li_reference_keyframe"""
    _fields_ = [("kf", KeyframeView), ("Xw", C.c_void_p), ("observed", C.c_void_p), ("last_pose7", C.c_float * 7), ("pad_", C.c_float)]


def track_reference_keyframe_batch(ext, voc, keypoints, u_right, refs, cam5, stream=0, with_bow=False):
    """``Tracking::TrackReferenceKeyFrame`` data path for the frames of the preceding ``extract_batch_dev`` / ``stereo_match_batch`` calls.
    refs: one dict per frame with the reference keyframe (keys, descriptors, has_point, fv_node / fv_offset / fv_index as
    ``pack_keyframe_views`` takes them), Xw [n, 3], observed [n] and last_pose7 -> (poses7 [F, 7], kf_keypoint_of_keypoint [F, capacity],
    n_matches, n_inliers, n_matches_map[, bow arrays])."""
    keypoints = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
    u_right = np.ascontiguousarray(u_right, np.float32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    F, cap = len(refs), keypoints.shape[1]
    views = []
    for r in refs:
        it = dict(r)
        n = len(it["keys"])
        it.setdefault("u_right", np.full(n, -1, np.float32)); it.setdefault("depth", np.full(n, -1, np.float32))
        it.setdefault("pose7", [0, 0, 0, 1, 0, 0, 0])
        views.append(it)
    arr, keep = pack_keyframe_views(views)
    rk = (ReferenceKeyframe * max(F, 1))()
    for i, r in enumerate(refs):
        xw = np.ascontiguousarray(r["Xw"], np.float32).reshape(-1, 3)
        ob = np.ascontiguousarray(r["observed"], np.uint8)
        keep.append((xw, ob))
        rk[i].kf = arr[i]
        rk[i].Xw, rk[i].observed = xw.ctypes.data, ob.ctypes.data
        rk[i].last_pose7 = (C.c_float * 7)(*[float(x) for x in r["last_pose7"]])
    poses, mp = np.zeros((max(F, 1), 7)), np.full((max(F, 1), cap), -1, np.int32)
    nm, inl, nmap = np.zeros(max(F, 1), np.int32), np.zeros(max(F, 1), np.int32), np.zeros(max(F, 1), np.int32)
    bow_arrays, bow_s = _bow_arrays(max(F * cap, 1), max(F, 1)) if with_bow else (None, None)
    f = lib().tc2li_track_reference_keyframe_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    _check(f(ext._h, voc._h, F, keypoints.ctypes.data, u_right.ctypes.data, cap, C.addressof(rk), cam5.ctypes.data, poses.ctypes.data,
             mp.ctypes.data, nm.ctypes.data, inl.ctypes.data, nmap.ctypes.data, C.byref(bow_s) if with_bow else None, C.c_void_p(stream)))
    del keep
    out = (poses[:F], mp[:F], nm[:F], inl[:F], nmap[:F])
    return out + (bow_arrays,) if with_bow else out


# ---- relocalisation: TemplatedVocabulary::score, KeyFrameDatabase, DetectRelocalizationCandidates --------------------------------------
class BowVector(C.Structure):
    """tc2li_bow_vector"""
    _fields_ = [("word", C.c_void_p), ("value", C.c_void_p), ("n", C.c_int32), ("pad_", C.c_int32)]


class RelocQuery(C.Structure):
    """tc2li_reloc_query"""
    _fields_ = [("db", C.c_void_p), ("map_id", C.c_int32), ("n_words", C.c_int32), ("bow_word", C.c_void_p), ("bow_value", C.c_void_p)]


class RelocScored(C.Structure):
    """tc2li_reloc_scored"""
    _fields_ = [("capacity", C.c_int32), ("pad_", C.c_int32)] + [(name, C.c_void_p) for name in ("n_scored", "kf_id", "words", "si", "acc_score",
                                                                                                  "best_kf_id")]


def _bow_pair_arrays(word, value):
    w = np.ascontiguousarray(word, np.int32).reshape(-1)
    v = np.ascontiguousarray(value, np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("a BowVector has as many values as words")
    return w, v


def _vocabulary_score(self, pairs, stream=0):
    """``TemplatedVocabulary::score(v1, v2)`` for a list of pairs ((word1, value1), (word2, value2)) -> float64 [n_pairs]."""
    n = len(pairs)
    a, b, keep = (BowVector * max(n, 1))(), (BowVector * max(n, 1))(), []
    for i, (p1, p2) in enumerate(pairs):
        for arr, p in ((a, p1), (b, p2)):
            w, v = _bow_pair_arrays(*p)
            keep.append((w, v))
            arr[i].word, arr[i].value, arr[i].n = w.ctypes.data, v.ctypes.data, len(w)
    out = np.zeros(max(n, 1), np.float64)
    f = lib().tc2li_vocabulary_score_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(self._h, n, C.addressof(a), C.addressof(b), out.ctypes.data, C.c_void_p(stream)))
    del keep
    return out[:n]


Vocabulary.score = _vocabulary_score


class KeyFrameDatabase:
    """``KeyFrameDatabase`` bound to one ``Vocabulary``: ``add`` / ``erase`` / ``clear`` / ``clear_map`` / ``set_covisibility`` / ``entries``
    are host logic (no GPU needed); ``detect_relocalization_candidates_batch`` queries it on the device."""

    def __init__(self, voc):
        self._voc = voc  # the vocabulary must outlive the database
        h = C.c_void_p()
        f = lib().tc2li_keyframe_db_create
        f.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _check(f(voc._h, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            f = lib().tc2li_keyframe_db_destroy
            f.argtypes = [C.c_void_p]
            f.restype = None
            f(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        f = lib().tc2li_keyframe_db_size
        f.argtypes = [C.c_void_p]
        return _check(f(self._h))

    def add(self, kf_id, map_id, bow_word, bow_value):
        """``KeyFrameDatabase::add`` -> the entry's sequence number."""
        w, v = _bow_pair_arrays(bow_word, bow_value)
        f = lib().tc2li_keyframe_db_add
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
        return _check(f(self._h, int(kf_id), int(map_id), len(w), w.ctypes.data, v.ctypes.data))

    def erase(self, kf_id):
        f = lib().tc2li_keyframe_db_erase
        f.argtypes = [C.c_void_p, C.c_int32]
        return _check(f(self._h, int(kf_id)))

    def clear(self):
        f = lib().tc2li_keyframe_db_clear
        f.argtypes = [C.c_void_p]
        return _check(f(self._h))

    def clear_map(self, map_id):
        f = lib().tc2li_keyframe_db_clear_map
        f.argtypes = [C.c_void_p, C.c_int32]
        return _check(f(self._h, int(map_id)))

    def set_covisibility(self, kf_id, neighbour_ids):
        ids = np.ascontiguousarray(neighbour_ids, np.int32).reshape(-1)
        f = lib().tc2li_keyframe_db_set_covisibility
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
        return _check(f(self._h, int(kf_id), len(ids), ids.ctypes.data))

    def entries(self):
        """Live entries in sequence order -> dict(kf_id, map_id, sequence, score)."""
        n = len(self)
        out = dict(kf_id=np.zeros(n, np.int32), map_id=np.zeros(n, np.int32), sequence=np.zeros(n, np.int32), score=np.zeros(n, np.float32))
        f = lib().tc2li_keyframe_db_entries
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _check(f(self._h, n, out["kf_id"].ctypes.data, out["map_id"].ctypes.data, out["sequence"].ctypes.data, out["score"].ctypes.data))
        return out


def detect_relocalization_candidates_batch(queries, capacity=None, scored_capacity=None, stream=0):
    """``KeyFrameDatabase::DetectRelocalizationCandidates`` for a list of queries (db, map_id, bow_word, bow_value), each against its own
    database -> (list of candidate kf_id arrays, scored) where scored is None or, with ``scored_capacity``, a list of dicts
    (kf_id, words, si, acc_score, best_kf_id) in ``lScoreAndMatch`` order."""
    n = len(queries)
    if capacity is None:
        capacity = max([len(q[0]) for q in queries] + [1])
    qs, keep = (RelocQuery * max(n, 1))(), []
    for i, (db, map_id, word, value) in enumerate(queries):
        w, v = _bow_pair_arrays(word, value)
        keep.append((w, v))
        qs[i].db, qs[i].map_id, qs[i].n_words, qs[i].bow_word, qs[i].bow_value = db._h, int(map_id), len(w), w.ctypes.data, v.ctypes.data
    nc = np.zeros(max(n, 1), np.int32)
    cand = np.full((max(n, 1), max(capacity, 1)), -1, np.int32)
    sc, sa = None, None
    if scored_capacity is not None:
        m = (max(n, 1), max(scored_capacity, 1))
        sa = dict(n_scored=np.zeros(max(n, 1), np.int32), kf_id=np.full(m, -1, np.int32), words=np.zeros(m, np.int32), si=np.zeros(m, np.float32),
                  acc_score=np.zeros(m, np.float32), best_kf_id=np.full(m, -1, np.int32))
        sc = RelocScored(int(scored_capacity), 0, *[sa[name].ctypes.data for name, _ in RelocScored._fields_[2:]])
    f = lib().tc2li_detect_relocalization_candidates_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(C.addressof(qs), n, int(capacity), nc.ctypes.data, cand.ctypes.data, C.byref(sc) if sc is not None else None, C.c_void_p(stream)))
    del keep
    cands = [cand[i, :nc[i]].copy() for i in range(n)]
    if sa is None:
        return cands, None
    scored = []
    for i in range(n):
        k = int(sa["n_scored"][i])
        scored.append({name: sa[name][i, :k].copy() for name in ("kf_id", "words", "si", "acc_score", "best_kf_id")})
    return cands, scored


class ProjectionKeyframeItem(C.Structure):
    """tc2li_projection_keyframe_item"""
    _fields_ = [("n", C.c_int32), ("n_points", C.c_int32), ("keys", C.c_void_p), ("descriptors", C.c_void_p), ("held", C.c_void_p),
                ("pose7", C.c_float * 7), ("bounds", C.c_float * 4), ("pad_", C.c_float), ("has_point", C.c_void_p), ("found", C.c_void_p),
                ("Xw", C.c_void_p), ("point_descriptors", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p),
                ("max_distance_raw", C.c_void_p), ("angle", C.c_void_p)]


def search_by_projection_keyframe_batch(items, cam4, scale_factors, log_scale_factor, th, orb_dist, check_orientation=True, capacity=None, stream=0):
    """``ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)`` for a list of items; each item is a dict with the
    frame (keys, descriptors, held, pose7, bounds = mnMinX, mnMaxX, mnMinY, mnMaxY) and the candidate keyframe's points in keypoint order
    (has_point, found, Xw, point_descriptors, min_distance, max_distance, max_distance_raw, angle)
    -> (kf_keypoint_of_keypoint [n_items, capacity], n_matches [n_items])."""
    n = len(items)
    arr, keep = (ProjectionKeyframeItem * max(n, 1))(), []
    for i, it in enumerate(items):
        k = np.ascontiguousarray(it["keys"], KEYPOINT_DTYPE)
        d = np.ascontiguousarray(it["descriptors"], np.uint8).reshape(-1, 32)
        held = np.ascontiguousarray(it["held"], np.uint8)
        hp, fd = np.ascontiguousarray(it["has_point"], np.uint8), np.ascontiguousarray(it["found"], np.uint8)
        xw = np.ascontiguousarray(it["Xw"], np.float32).reshape(-1, 3)
        pd = np.ascontiguousarray(it["point_descriptors"], np.uint8).reshape(-1, 32)
        fl = [np.ascontiguousarray(it[name], np.float32) for name in ("min_distance", "max_distance", "max_distance_raw", "angle")]
        if not (len(d) == len(held) == len(k)) or not all(len(a) == len(hp) for a in [fd, xw, pd] + fl):
            raise ValueError("item %d: array lengths differ" % i)
        keep.append((k, d, held, hp, fd, xw, pd, fl))
        arr[i].n, arr[i].n_points = len(k), len(hp)
        arr[i].keys, arr[i].descriptors, arr[i].held = k.ctypes.data, d.ctypes.data, held.ctypes.data
        arr[i].pose7 = (C.c_float * 7)(*[float(v) for v in it["pose7"]])
        arr[i].bounds = (C.c_float * 4)(*[float(v) for v in it["bounds"]])
        arr[i].has_point, arr[i].found, arr[i].Xw, arr[i].point_descriptors = hp.ctypes.data, fd.ctypes.data, xw.ctypes.data, pd.ctypes.data
        arr[i].min_distance, arr[i].max_distance, arr[i].max_distance_raw, arr[i].angle = [a.ctypes.data for a in fl]
    if capacity is None:
        capacity = max([len(it["keys"]) for it in items] + [1])
    cam4 = np.ascontiguousarray(cam4, np.float32)
    sf = np.ascontiguousarray(scale_factors, np.float32)
    match = np.full((max(n, 1), max(capacity, 1)), -1, np.int32)
    nm = np.zeros(max(n, 1), np.int32)
    f = lib().tc2li_search_by_projection_keyframe_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(C.addressof(arr), n, cam4.ctypes.data, sf.ctypes.data, len(sf), float(log_scale_factor), float(th), int(orb_dist), int(bool(check_orientation)),
             int(capacity), match.ctypes.data, nm.ctypes.data, C.c_void_p(stream)))
    del keep
    return match[:n], nm[:n]


class RelocHypothesis(C.Structure):
    """tc2li_reloc_hypothesis"""
    _fields_ = [("frame_index", C.c_int32), ("n_points", C.c_int32), ("has_point", C.c_void_p), ("Xw", C.c_void_p), ("point_descriptors", C.c_void_p),
                ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("max_distance_raw", C.c_void_p), ("angle", C.c_void_p),
                ("match", C.c_void_p), ("inlier", C.c_void_p), ("pose7", C.c_float * 7), ("pad_", C.c_float)]


RELOC_OPT1, RELOC_REJECTED, RELOC_SEARCH1, RELOC_OPT2, RELOC_SEARCH2, RELOC_OPT3, RELOC_SUCCESS = 1, 2, 4, 8, 16, 32, 64


def relocalization_refine_batch(ext, hyps, u_right, cam5, stream=0):
    """The refinement ladder of ``Tracking::Relocalization`` after a PnP pose, for the frames of the preceding ``extract_batch_dev`` /
    ``stereo_match_batch`` calls.  hyps: dicts with frame_index, the candidate keyframe (has_point, Xw, point_descriptors, min_distance,
    max_distance, max_distance_raw, angle), pose7, match and inlier (per frame keypoint) -> dict(status, n_good, n_additional [H, 2],
    poses7 [H, 3, 7], kf_keypoint_of_keypoint [H, capacity], outlier [H, capacity])."""
    u_right = np.ascontiguousarray(u_right, np.float32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    n_frames, cap = u_right.shape
    H = len(hyps)
    arr, keep = (RelocHypothesis * max(H, 1))(), []
    for i, hy in enumerate(hyps):
        hp = np.ascontiguousarray(hy["has_point"], np.uint8)
        xw = np.ascontiguousarray(hy["Xw"], np.float32).reshape(-1, 3)
        pd = np.ascontiguousarray(hy["point_descriptors"], np.uint8).reshape(-1, 32)
        fl = [np.ascontiguousarray(hy[name], np.float32) for name in ("min_distance", "max_distance", "max_distance_raw", "angle")]
        m = np.full(cap, -1, np.int32); inl = np.zeros(cap, np.uint8)
        m[:len(hy["match"])] = hy["match"]; inl[:len(hy["inlier"])] = hy["inlier"]
        if not all(len(a) == len(hp) for a in [xw, pd] + fl):
            raise ValueError("hypothesis %d: array lengths differ" % i)
        keep.append((hp, xw, pd, fl, m, inl))
        arr[i].frame_index, arr[i].n_points = int(hy["frame_index"]), len(hp)
        arr[i].has_point, arr[i].Xw, arr[i].point_descriptors = hp.ctypes.data, xw.ctypes.data, pd.ctypes.data
        arr[i].min_distance, arr[i].max_distance, arr[i].max_distance_raw, arr[i].angle = [a.ctypes.data for a in fl]
        arr[i].match, arr[i].inlier = m.ctypes.data, inl.ctypes.data
        arr[i].pose7 = (C.c_float * 7)(*[float(v) for v in hy["pose7"]])
    n1 = max(H, 1)
    out = dict(status=np.zeros(n1, np.int32), n_good=np.zeros(n1, np.int32), n_additional=np.zeros((n1, 2), np.int32), poses7=np.zeros((n1, 3, 7)),
               kf_keypoint_of_keypoint=np.full((n1, cap), -1, np.int32), outlier=np.zeros((n1, cap), np.uint8))
    f = lib().tc2li_relocalization_refine_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    _check(f(ext._h, C.addressof(arr), H, n_frames, u_right.ctypes.data, cap, cam5.ctypes.data, out["status"].ctypes.data, out["n_good"].ctypes.data,
             out["n_additional"].ctypes.data, out["poses7"].ctypes.data, out["kf_keypoint_of_keypoint"].ctypes.data, out["outlier"].ctypes.data,
             C.c_void_p(stream)))
    del keep
    return {k: v[:H] for k, v in out.items()}


class MlpnpParams(C.Structure):
    """tc2li_mlpnp_params; the defaults are SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991) of Tracking.cc:3526"""
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float), ("pad_", C.c_int32)]


class MlpnpState(C.Structure):
    """tc2li_mlpnp_state"""
    _fields_ = [("iterations", C.c_int32), ("best_inliers", C.c_int32), ("best_Tcw", C.c_float * 12)]


class MlpnpProblem(C.Structure):
    """tc2li_mlpnp_problem"""
    _fields_ = [("keys", C.c_void_p), ("match", C.c_void_p), ("Xw", C.c_void_p), ("draws", C.c_void_p), ("state", C.c_void_p),
                ("best_inlier", C.c_void_p), ("n_keypoints", C.c_int32), ("n_points", C.c_int32), ("n_draws", C.c_int32),
                ("n_iterations", C.c_int32)]


def mlpnp_params(probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, th2=5.991):
    return MlpnpParams(float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2), 0)


def mlpnp_iterations(n_correspondences, params=None):
    """``MLPnPsolver::SetRansacParameters`` for N correspondences -> (min_inliers, max_iterations)."""
    params = params or mlpnp_params()
    a, b = C.c_int32(0), C.c_int32(0)
    f = lib().tc2li_mlpnp_iterations
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(int(n_correspondences), C.addressof(params), C.addressof(a), C.addressof(b)))
    return a.value, b.value


def mlpnp_ransac_batch(problems, level_sigma2, cam5, params=None, capacity=None, host=False, stream=0):
    """One ``MLPnPsolver::iterate`` call per problem.  problems: dicts with keys (KEYPOINT_DTYPE), match [n_keypoints] (index into Xw or
    -1), Xw [n_points, 3], draws (rand() values, 6 per iteration), n_iterations (default 5) and optionally the solver's state from an
    earlier call: iterations, best_inliers, best_Tcw [12], best_inlier [n_keypoints].  -> dict(found, no_more, n_inliers, pose7 [P, 7],
    Rt12 [P, 12], inlier [P, capacity], iterations, best_inliers, best_Tcw [P, 12], best_inlier [P, capacity]); the last four are the
    state to hand to the next call.  host=True runs the same arithmetic on the CPU."""
    params = params or mlpnp_params()
    level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
    cam5 = np.ascontiguousarray(cam5, np.float64)
    P = len(problems)
    if capacity is None:
        capacity = max([len(p["keys"]) for p in problems] + [1])
    arr, states, keep = (MlpnpProblem * max(P, 1))(), (MlpnpState * max(P, 1))(), []
    n1 = max(P, 1)
    best = np.zeros((n1, capacity), np.uint8)
    for i, p in enumerate(problems):
        keys = np.ascontiguousarray(p["keys"], KEYPOINT_DTYPE)
        match = np.ascontiguousarray(p["match"], np.int32)
        xw = np.ascontiguousarray(p["Xw"], np.float32).reshape(-1, 3)
        draws = np.ascontiguousarray(p["draws"], np.uint32)
        if len(match) != len(keys):
            raise ValueError("problem %d: match and keys differ in length" % i)
        keep.append((keys, match, xw, draws))
        states[i].iterations, states[i].best_inliers = int(p.get("iterations", 0)), int(p.get("best_inliers", 0))
        states[i].best_Tcw = (C.c_float * 12)(*[float(v) for v in p.get("best_Tcw", np.zeros(12))])
        if "best_inlier" in p and len(keys) <= capacity:
            best[i, :len(keys)] = np.asarray(p["best_inlier"], np.uint8)[:len(keys)]
        arr[i].keys, arr[i].match, arr[i].Xw, arr[i].draws = keys.ctypes.data, match.ctypes.data, xw.ctypes.data, draws.ctypes.data
        arr[i].state, arr[i].best_inlier = C.addressof(states[i]), best[i].ctypes.data
        arr[i].n_keypoints, arr[i].n_points, arr[i].n_draws = len(keys), len(xw), len(draws)
        arr[i].n_iterations = int(p.get("n_iterations", 5))
    out = dict(found=np.zeros(n1, np.int32), no_more=np.zeros(n1, np.int32), n_inliers=np.zeros(n1, np.int32), pose7=np.zeros((n1, 7), np.float32),
               Rt12=np.zeros((n1, 12)), inlier=np.zeros((n1, capacity), np.uint8))
    args = [C.addressof(arr), P, C.addressof(params), level_sigma2.ctypes.data, len(level_sigma2), cam5.ctypes.data, out["found"].ctypes.data,
            out["no_more"].ctypes.data, out["n_inliers"].ctypes.data, out["pose7"].ctypes.data, out["Rt12"].ctypes.data, out["inlier"].ctypes.data,
            int(capacity)]
    if host:
        f = lib().tc2li_host_mlpnp_ransac_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int]
        _check(f(*args))
    else:
        f = lib().tc2li_mlpnp_ransac_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        _check(f(*(args + [C.c_void_p(stream)])))
    del keep
    out = {k: v[:P] for k, v in out.items()}
    out["iterations"] = np.array([states[i].iterations for i in range(P)], np.int32)
    out["best_inliers"] = np.array([states[i].best_inliers for i in range(P)], np.int32)
    out["best_Tcw"] = np.array([list(states[i].best_Tcw) for i in range(P)], np.float32).reshape(P, 12)
    out["best_inlier"] = best[:P]
    return out


class CullingProblem(C.Structure):
    """tc2li_culling_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_flags", "kf_id", "kf_prev", "kf_next", "kf_time", "kf_imu_pos", "kf_th_depth", "slot_offsets",
                                          "slot_point", "slot_depth", "slot_octave", "local", "point_bad", "point_nobs", "obs_offsets", "obs_kf",
                                          "obs_octave", "obs_weight", "verdict", "n_mps", "n_redundant", "n_visited", "point_bad_after",
                                          "point_nobs_after")] \
        + [("current_id", C.c_int64), ("last_id", C.c_int64), ("n_keyframes", C.c_int32), ("n_local", C.c_int32), ("n_points", C.c_int32),
           ("keyframes_in_map", C.c_int32), ("inertial", C.c_uint8), ("imu_initialized", C.c_uint8), ("inertial_ba2", C.c_uint8),
           ("abort_ba", C.c_uint8), ("pad_", C.c_int32)]


CULL_SKIPPED, CULL_NOT_VISITED, CULL_REDUNDANT, CULL_SET_BAD, CULL_MERGED, CULL_DEFERRED = -1, -2, 1, 2, 4, 8
_CULLING_ARRAYS = (("kf_flags", np.uint8), ("kf_id", np.int64), ("kf_prev", np.int32), ("kf_next", np.int32), ("kf_time", np.float64),
                   ("kf_imu_pos", np.float32), ("kf_th_depth", np.float32), ("slot_offsets", np.int32), ("slot_point", np.int32),
                   ("slot_depth", np.float32), ("slot_octave", np.int8), ("local", np.int32), ("point_bad", np.uint8), ("point_nobs", np.int32),
                   ("obs_offsets", np.int32), ("obs_kf", np.int32), ("obs_octave", np.int8), ("obs_weight", np.uint8))
_CULLING_SCALARS = ("inertial", "imu_initialized", "inertial_ba2", "abort_ba", "keyframes_in_map", "current_id", "last_id")


def pack_culling_problems(problems):
    """The tc2li_culling_problem array of a batch with its output arrays -> (array, outputs per problem, what must stay alive)."""
    P = len(problems)
    arr, outs, keep = (CullingProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], t) for k, t in _CULLING_ARRAYS}
        nk, npts, nl = len(a["kf_flags"]), len(a["point_bad"]), len(a["local"])
        for k in ("kf_id", "kf_prev", "kf_next", "kf_time", "kf_th_depth"):
            if len(a[k]) != nk:
                raise ValueError("problem %d: %s has %d rows for %d keyframes" % (i, k, len(a[k]), nk))
        if a["kf_imu_pos"].size != 3 * nk or len(a["slot_offsets"]) != nk + 1 or len(a["point_nobs"]) != npts or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: kf_imu_pos, slot_offsets, point_nobs or obs_offsets do not fit the tables" % i)
        ns, no = int(a["slot_offsets"][-1]), int(a["obs_offsets"][-1])
        if min(len(a[k]) for k in ("slot_point", "slot_depth", "slot_octave")) < ns or min(len(a[k]) for k in ("obs_kf", "obs_octave", "obs_weight")) < no:
            raise ValueError("problem %d: slot or observation arrays are shorter than their offsets say" % i)
        o = dict(verdict=np.zeros(nl, np.int32), n_mps=np.zeros(nl, np.int32), n_redundant=np.zeros(nl, np.int32), n_visited=np.zeros(1, np.int32),
                 point_bad_after=np.zeros(npts, np.uint8), point_nobs_after=np.zeros(npts, np.int32))
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        for k in _CULLING_SCALARS:
            setattr(arr[i], k, int(p.get(k, 0)))
        arr[i].n_keyframes, arr[i].n_local, arr[i].n_points = nk, nl, npts
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def keyframe_culling_batch(problems, host=False, stream=0):
    """One ``LocalMapping::KeyFrameCulling`` call per problem.  problems: dicts with the arrays of tc2li_culling_problem (kf_flags, kf_id,
    kf_prev, kf_next, kf_time, kf_imu_pos [n, 3], kf_th_depth, slot_offsets, slot_point, slot_depth, slot_octave, local, point_bad, point_nobs,
    obs_offsets, obs_kf, obs_octave, obs_weight) and its scalars (inertial, imu_initialized, inertial_ba2, abort_ba, keyframes_in_map,
    current_id, last_id; default 0) -> one dict per problem: verdict, n_mps, n_redundant [n_local] (the counters are 0 where verdict < 0),
    n_visited, point_bad_after, point_nobs_after [n_points].  host=True walks the same graph on the CPU."""
    arr, outs, keep = pack_culling_problems(problems)
    if host:
        f = lib().tc2li_host_keyframe_culling_batch
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(C.addressof(arr), len(problems)))
    else:
        f = lib().tc2li_keyframe_culling_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(problems), C.c_void_p(stream)))
    del keep
    return [dict(o, n_visited=int(o["n_visited"][0])) for o in outs]


def map_point_culling_batch(points, th_obs=3, host=False, stream=0):
    """``LocalMapping::MapPointCulling`` for the entries of mlpRecentAddedMapPoints of any number of sequences.  points: dict of arrays bad,
    n_found, n_visible, first_kf_id, n_obs, current_kf_id (one entry per point) -> action [n] uint8: 0 stays, 1 dropped (bad), 2 SetBadFlag
    (found ratio), 3 SetBadFlag (observations), 4 dropped by age."""
    a = [np.ascontiguousarray(points[k], t) for k, t in (("bad", np.uint8), ("n_found", np.int32), ("n_visible", np.int32), ("first_kf_id", np.int64),
                                                         ("n_obs", np.int32), ("current_kf_id", np.int64))]
    n = len(a[0])
    if any(len(v) != n for v in a):
        raise ValueError("the arrays differ in length")
    action = np.zeros(n, np.uint8)
    args = [v.ctypes.data for v in a] + [n, int(th_obs), action.ctypes.data]
    if host:
        f = lib().tc2li_host_map_point_culling_batch
        f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
        _check(f(*args))
    else:
        f = lib().tc2li_map_point_culling_batch
        f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(*(args + [C.c_void_p(stream)])))
    return action


class ScaledRotationProblem(C.Structure):
    """tc2li_scaled_rotation_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_pose7", "kf_vel", "point_pos", "point_bad", "obs_offsets", "obs_kf", "point_ref_kf",
                                          "point_ref_level_scale", "kf_pose7_out", "kf_inv_pose7_out", "kf_imu_pos_out", "kf_vel_out",
                                          "point_pos_out", "point_normal", "point_min_distance", "point_max_distance")] \
        + [("T7", C.c_float * 7), ("s", C.c_float), ("tcb3", C.c_float * 3), ("last_level_scale", C.c_float), ("n_keyframes", C.c_int32),
           ("n_points", C.c_int32), ("scaled_vel", C.c_uint8), ("has_tcb", C.c_uint8), ("pad_", C.c_uint8 * 6)]


_SCALED_ROTATION_ARRAYS = (("kf_pose7", np.float32, 7), ("kf_vel", np.float32, 3), ("point_pos", np.float32, 3), ("point_bad", np.uint8, 0),
                           ("obs_offsets", np.int32, 0), ("obs_kf", np.int32, 0), ("point_ref_kf", np.int32, 0), ("point_ref_level_scale", np.float32, 0))
_SCALED_ROTATION_OUTPUTS = (("kf_pose7_out", np.float32, "k", 7), ("kf_inv_pose7_out", np.float32, "k", 7), ("kf_imu_pos_out", np.float32, "k", 3),
                            ("kf_vel_out", np.float32, "k", 3), ("point_pos_out", np.float32, "p", 3), ("point_normal", np.float32, "p", 3),
                            ("point_min_distance", np.float32, "p", 0), ("point_max_distance", np.float32, "p", 0))


def _rows(a, width):
    """A flat table as rows of `width` entries (0: a plain array)."""
    return a.reshape(-1, width) if width else a.reshape(-1)


def _fill_outputs(spec, sizes, fill):
    """The output arrays of a problem: spec entries (name, dtype, which size, width), every array filled with `fill` reinterpreted as its
    type, so that a test sees what a call left untouched."""
    out = {}
    for k, t, which, width in spec:
        a = np.empty((sizes[which], width) if width else (sizes[which],), t)
        a.view(np.uint8)[...] = fill
        out[k] = a
    return out


def pack_scaled_rotation_problems(problems, fill=0):
    """The tc2li_scaled_rotation_problem array of a batch with its output arrays (every byte prefilled with `fill`) -> (array, outputs per
    problem, what must stay alive)."""
    P = len(problems)
    arr, outs, keep = (ScaledRotationProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: _rows(np.ascontiguousarray(p[k], t), w) for k, t, w in _SCALED_ROTATION_ARRAYS}
        nk, npts = len(a["kf_pose7"]), len(a["point_pos"])
        if len(a["kf_vel"]) != nk or any(len(a[k]) != npts for k in ("point_bad", "point_ref_kf", "point_ref_level_scale")) or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: the tables do not fit n_keyframes = %d, n_points = %d" % (i, nk, npts))
        if len(a["obs_kf"]) < int(a["obs_offsets"][-1]):
            raise ValueError("problem %d: obs_kf is shorter than obs_offsets say" % i)
        o = _fill_outputs(_SCALED_ROTATION_OUTPUTS, dict(k=nk, p=npts), fill)
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        arr[i].T7 = (C.c_float * 7)(*[float(v) for v in np.asarray(p["T7"], np.float32)])
        arr[i].tcb3 = (C.c_float * 3)(*[float(v) for v in np.asarray(p.get("tcb3", (0, 0, 0)), np.float32)])
        arr[i].s, arr[i].last_level_scale = float(np.float32(p["s"])), float(np.float32(p["last_level_scale"]))
        arr[i].scaled_vel, arr[i].has_tcb = int(bool(p.get("scaled_vel", 0))), int(bool(p.get("has_tcb", 0)))
        arr[i].n_keyframes, arr[i].n_points = nk, npts
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def apply_scaled_rotation_batch(problems, host=False, stream=0, fill=0):
    """One ``Map::ApplyScaledRotation(T, s, bScaledVel)`` per problem.  problems: dicts with T7 (quaternion x, y, z, w, then translation), s,
    scaled_vel, has_tcb, tcb3, last_level_scale and the arrays of tc2li_scaled_rotation_problem (kf_pose7 [n, 7], kf_vel [n, 3], point_pos
    [m, 3], point_bad, obs_offsets [m + 1], obs_kf, point_ref_kf, point_ref_level_scale) -> one dict per problem: kf_pose7_out,
    kf_inv_pose7_out, kf_imu_pos_out, kf_vel_out, point_pos_out, point_normal, point_min_distance, point_max_distance.  What the reference
    leaves untouched (normal and distances of bad points and of points without observations, kf_imu_pos_out without has_tcb) keeps the
    `fill` bytes.  host=True runs the same arithmetic on the CPU."""
    arr, outs, keep = pack_scaled_rotation_problems(problems, fill)
    if host:
        f = lib().tc2li_host_apply_scaled_rotation_batch
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(C.addressof(arr), len(problems)))
    else:
        f = lib().tc2li_apply_scaled_rotation_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(problems), C.c_void_p(stream)))
    del keep
    return outs


class GbaCorrectionProblem(C.Structure):
    """tc2li_gba_correction_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_parent", "kf_origin", "kf_bad", "kf_in_gba", "kf_imu", "kf_vel_set", "kf_pose7", "kf_gba_pose7",
                                          "kf_bef_gba_pose7", "kf_vel", "kf_gba_vel", "kf_bias", "kf_gba_bias", "point_bad", "point_in_gba", "point_pos",
                                          "point_gba_pos", "point_ref_kf", "kf_visited", "kf_in_gba_out", "kf_pose7_out", "kf_bef_gba_pose7_out",
                                          "kf_vel_out", "kf_bias_out", "point_pos_out", "point_moved")] \
        + [("n_keyframes", C.c_int32), ("n_points", C.c_int32)]


_GBA_CORRECTION_ARRAYS = (("kf_parent", np.int32, 0, "k"), ("kf_origin", np.uint8, 0, "k"), ("kf_bad", np.uint8, 0, "k"), ("kf_in_gba", np.uint8, 0, "k"),
                          ("kf_imu", np.uint8, 0, "k"), ("kf_vel_set", np.uint8, 0, "k"), ("kf_pose7", np.float32, 7, "k"), ("kf_gba_pose7", np.float32, 7, "k"),
                          ("kf_bef_gba_pose7", np.float32, 7, "k"), ("kf_vel", np.float32, 3, "k"), ("kf_gba_vel", np.float32, 3, "k"),
                          ("kf_bias", np.float32, 6, "k"), ("kf_gba_bias", np.float32, 6, "k"), ("point_bad", np.uint8, 0, "p"),
                          ("point_in_gba", np.uint8, 0, "p"), ("point_pos", np.float32, 3, "p"), ("point_gba_pos", np.float32, 3, "p"),
                          ("point_ref_kf", np.int32, 0, "p"))
_GBA_CORRECTION_OUTPUTS = (("kf_visited", np.uint8, "k", 0), ("kf_in_gba_out", np.uint8, "k", 0), ("kf_pose7_out", np.float32, "k", 7),
                           ("kf_bef_gba_pose7_out", np.float32, "k", 7), ("kf_vel_out", np.float32, "k", 3), ("kf_bias_out", np.float32, "k", 6),
                           ("point_pos_out", np.float32, "p", 3), ("point_moved", np.uint8, "p", 0))


def pack_gba_correction_problems(problems, fill=0):
    """The tc2li_gba_correction_problem array of a batch with its output arrays (every byte prefilled with `fill`) -> (array, outputs per
    problem, what must stay alive)."""
    P = len(problems)
    arr, outs, keep = (GbaCorrectionProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: _rows(np.ascontiguousarray(p[k], t), w) for k, t, w, _ in _GBA_CORRECTION_ARRAYS}
        sizes = dict(k=len(a["kf_parent"]), p=len(a["point_bad"]))
        for k, _, _, which in _GBA_CORRECTION_ARRAYS:
            if len(a[k]) != sizes[which]:
                raise ValueError("problem %d: %s has %d rows, not %d" % (i, k, len(a[k]), sizes[which]))
        o = _fill_outputs(_GBA_CORRECTION_OUTPUTS, sizes, fill)
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        arr[i].n_keyframes, arr[i].n_points = sizes["k"], sizes["p"]
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def gba_map_correction_batch(problems, host=False, stream=0, fill=0):
    """The map update that follows a global BA (``LocalMapping::InitializeIMU`` after ``FullInertialBA``), one per problem.  problems: dicts
    with the arrays of tc2li_gba_correction_problem (kf_parent, kf_origin, kf_bad, kf_in_gba, kf_imu, kf_vel_set, kf_pose7, kf_gba_pose7,
    kf_bef_gba_pose7 [n, 7], kf_vel, kf_gba_vel [n, 3], kf_bias, kf_gba_bias [n, 6], point_bad, point_in_gba, point_pos, point_gba_pos [m, 3],
    point_ref_kf) -> one dict per problem: kf_visited, kf_in_gba_out, kf_pose7_out, kf_bef_gba_pose7_out, kf_vel_out, kf_bias_out,
    point_pos_out, point_moved (0 untouched, 1 the GBA position, 2 followed its reference keyframe).  host=True walks the tree on the CPU."""
    arr, outs, keep = pack_gba_correction_problems(problems, fill)
    if host:
        f = lib().tc2li_host_gba_map_correction_batch
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(C.addressof(arr), len(problems)))
    else:
        f = lib().tc2li_gba_map_correction_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(problems), C.c_void_p(stream)))
    del keep
    return outs


def map_update_limits():
    """tc2li_map_update_limits -> {max_keyframes, walk_threads, keyframe_tile, point_tile}."""
    out = (C.c_int32 * 4)()
    f = lib().tc2li_map_update_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 4))
    return dict(zip(("max_keyframes", "walk_threads", "keyframe_tile", "point_tile"), [int(v) for v in out]))


class InertialInitProblem(C.Structure):
    """tc2li_inertial_init_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("Rwb9", "twb3", "vel3", "pre", "Rwg9", "scale", "bg", "ba", "bg3", "ba3", "stats", "chi2", "iterations_run")] \
        + [(k, C.c_int32) for k in ("n_keyframes", "mono", "fixed_vel", "iterations", "refine")] \
        + [("prior_g", C.c_float), ("prior_a", C.c_float), ("pad_", C.c_int32)]


def pack_inertial_init_problems(problems, all_refine=False):
    """The tc2li_inertial_init_problem array of a batch -> (array, per problem the arrays the call writes, what must stay alive).  problems:
    dicts with Rwb [n, 3, 3], twb [n, 3], vel [n, 3], pres (``Preintegrated`` or None per keyframe, pres[0] ignored), Rwg, scale and, first
    form: bg, ba, mono, fixed_vel, prior_g (1e2), prior_a (1e6), iterations (200); refinement form (refine=True): bg3, ba3 [n, 3], iterations
    (10).  A key given as None reaches the library as a NULL pointer; n_keyframes overrides the count taken from Rwb.  all_refine: for the
    entry that takes every problem in the refinement form (the flag is passed on as the problem has it)."""
    P = len(problems)
    arr, outs, keep = (InertialInitProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        flag = bool(p.get("refine", False))
        refine = flag or all_refine
        n = int(p.get("n_keyframes", 0 if p.get("Rwb") is None else len(np.asarray(p["Rwb"]).reshape(-1, 9))))

        def table(key, width, must=True):
            v = p.get(key)
            if v is None:
                if must and key not in p:
                    raise ValueError("problem %d lacks %s" % (i, key))
                return None
            return np.ascontiguousarray(v, np.float64).reshape(-1, width).copy()
        a = dict(Rwb9=table("Rwb", 9), twb3=table("twb", 3), vel3=table("vel", 3), Rwg9=table("Rwg", 9), bg=table("bg", 3, not refine), ba=table("ba", 3, not refine),
                 bg3=table("bg3", 3, refine), ba3=table("ba3", 3, refine))
        a["scale"] = None if p.get("scale", 1.0) is None else np.array([p.get("scale", 1.0)], np.float64)
        pres = p.get("pres")
        ptrs = None
        if pres is not None:
            ptrs = (C.c_void_p * max(len(pres), 1))(*[None if (k == 0 or q is None) else C.addressof(q.p) for k, q in enumerate(pres)])
        o = dict(stats=InertialInitStats(), chi2=np.zeros(2), iterations_run=np.zeros(1, np.int32))
        for k, v in a.items():
            setattr(arr[i], k, None if v is None else v.ctypes.data)
        arr[i].pre = None if ptrs is None else C.addressof(ptrs)
        arr[i].stats, arr[i].chi2, arr[i].iterations_run = C.addressof(o["stats"]), o["chi2"].ctypes.data, o["iterations_run"].ctypes.data
        arr[i].n_keyframes, arr[i].mono, arr[i].fixed_vel = n, int(bool(p.get("mono", False))), int(bool(p.get("fixed_vel", False)))
        arr[i].iterations, arr[i].refine = int(p.get("iterations", 10 if refine else 200)), int(flag)
        arr[i].prior_g, arr[i].prior_a = float(p.get("prior_g", 1e2)), float(p.get("prior_a", 1e6))
        o.update(a)
        keep.append((a, ptrs, pres))
        outs.append(o)
    return arr, outs, keep


def _inertial_init_batch(name, problems, host, stream):
    arr, outs, keep = pack_inertial_init_problems(problems, name == "inertial_scale_refinement_batch")
    f = getattr(lib(), ("tc2li_host_" if host else "tc2li_") + name)
    if host:
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(C.addressof(arr), len(problems)))
    else:
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(problems), C.c_void_p(stream)))
    del keep
    res = []
    for p, o in zip(problems, outs):
        r = dict(Rwg=o["Rwg9"].reshape(3, 3), scale=float(o["scale"][0]), iterations=int(o["iterations_run"][0]))
        if p.get("refine", False) or name == "inertial_scale_refinement_batch":
            r.update(chi2=(float(o["chi2"][0]), float(o["chi2"][1])))
        else:
            r.update(vel=o["vel3"], bg=o["bg"].reshape(3), ba=o["ba"].reshape(3), stats=o["stats"])
        res.append(r)
    return res


def inertial_optimization_batch(problems, host=False, stream=0):
    """``Optimizer::InertialOptimization`` for many maps at once (tc2li_inertial_optimization_batch; host=True: the single-problem entries on the
    pool).  problems: see pack_inertial_init_problems; each is taken in the form its ``refine`` says -> one dict per problem: Rwg, scale,
    iterations and vel, bg, ba, stats (first form) or chi2 (refinement form)."""
    return _inertial_init_batch("inertial_optimization_batch", problems, host, stream)


def inertial_scale_refinement_batch(problems, host=False, stream=0):
    """The second overload (``LocalMapping::ScaleRefinement``) for many maps at once: every problem in the refinement form -> one dict per
    problem: Rwg, scale, iterations, chi2."""
    return _inertial_init_batch("inertial_scale_refinement_batch", problems, host, stream)


def inertial_init_limits():
    """tc2li_inertial_init_limits -> {max_keyframes, max_refine_keyframes, max_iterations}."""
    out = (C.c_int32 * 3)()
    f = lib().tc2li_inertial_init_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 3))
    return dict(zip(("max_keyframes", "max_refine_keyframes", "max_iterations"), [int(v) for v in out]))


def inertial_init_arrow_pivot(D, L, Sinv_prev, lam):
    """tc2li_inertial_init_arrow_pivot -> S^-1 [3, 3] of S = D + lam I - L Sinv_prev L' (Sinv_prev None: the first block), or None when S is
    singular."""
    D = np.ascontiguousarray(D, np.float64).reshape(9)
    L = None if L is None else np.ascontiguousarray(L, np.float64).reshape(9)
    Sp = None if Sinv_prev is None else np.ascontiguousarray(Sinv_prev, np.float64).reshape(9)
    out = np.full(9, np.nan)
    f = lib().tc2li_inertial_init_arrow_pivot
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    rc = _check(f(D.ctypes.data, None if L is None else L.ctypes.data, None if Sp is None else Sp.ctypes.data, float(lam), out.ctypes.data))
    return out.reshape(3, 3) if rc == 1 else None


class StereoPointsFrame(C.Structure):
    """tc2li_stereo_points_frame"""
    _fields_ = [(k, C.c_void_p) for k in ("depth", "keys", "held", "outlier", "created_keypoint", "x3D", "counts")] \
        + [("Rwc", C.c_float * 9), ("Ow", C.c_float * 3), ("th_depth", C.c_float), ("n", C.c_int32), ("max_point", C.c_int32), ("mode", C.c_int32)]


class KeyframeDecision(C.Structure):
    """tc2li_keyframe_decision"""
    _fields_ = [("ref_nobs", C.c_void_p), ("frame_id", C.c_uint64), ("last_reloc_frame_id", C.c_uint64), ("last_keyframe_id", C.c_uint64),
                ("time_frame", C.c_double), ("time_last_kf", C.c_double)] \
        + [(k, C.c_int32) for k in ("n_ref", "max_frames", "min_frames", "n_kfs", "matches_inliers", "n_ref_matches", "keyframes_in_queue")] \
        + [(k, C.c_uint8) for k in ("inertial", "imu_initialized", "only_tracking", "mapper_stopped", "mapper_idle", "mapper_initializing",
                                    "create_blocked", "has_last_kf")] + [("pad_", C.c_int32)]


class KeyframeVerdict(C.Structure):
    """tc2li_keyframe_verdict"""
    _fields_ = [(k, C.c_int32) for k in ("need", "interrupt_ba", "conditions", "exit_rule", "n_tracked_close", "n_non_tracked_close",
                                         "n_ref_matches", "pad_")]


STEREO_POINTS_CLOSEST, STEREO_POINTS_ALL = 0, 1
NEWKF_C1A, NEWKF_C1B, NEWKF_C1C, NEWKF_C2, NEWKF_C3 = 1, 2, 4, 8, 16
(NEWKF_EXIT_IMU_NOT_INITIALIZED, NEWKF_EXIT_ONLY_TRACKING, NEWKF_EXIT_MAPPER_STOPPED, NEWKF_EXIT_AFTER_RELOC, NEWKF_EXIT_CONDITIONS,
 NEWKF_EXIT_MAPPER_ACCEPTS, NEWKF_EXIT_MAPPER_BUSY) = range(1, 8)
_DECISION_SCALARS = tuple(k for k, _ in KeyframeDecision._fields_ if k not in ("ref_nobs", "n_ref", "pad_"))


def pack_stereo_points_frames(frames):
    """The tc2li_stereo_points_frame array of a batch with its output arrays -> (array, outputs per frame, what must stay alive).  A frame
    is a dict: depth [n], keys [n] (KEYPOINT_DTYPE, or an [n, 2] array of x, y), held [n], optionally outlier [n], Rwc [3, 3] or [9], Ow [3],
    th_depth, and optionally max_point (100) and mode (STEREO_POINTS_CLOSEST)."""
    arr, outs, keep = (StereoPointsFrame * max(len(frames), 1))(), [], []
    for i, f in enumerate(frames):
        depth = np.ascontiguousarray(f["depth"], np.float32).reshape(-1)
        n = len(depth)
        keys = f["keys"]
        if getattr(keys, "dtype", None) != KEYPOINT_DTYPE:
            xy = np.asarray(keys, np.float32).reshape(n, 2)
            keys = np.zeros(n, KEYPOINT_DTYPE)
            keys["x"], keys["y"] = xy[:, 0], xy[:, 1]
        keys = np.ascontiguousarray(keys)
        held = np.ascontiguousarray(f["held"], np.uint8).reshape(-1)
        outlier = None if f.get("outlier") is None else np.ascontiguousarray(f["outlier"], np.uint8).reshape(-1)
        if len(keys) != n or len(held) != n or (outlier is not None and len(outlier) != n):
            raise ValueError("frame %d: keys, held or outlier do not have depth's %d rows" % (i, n))
        o = dict(created_keypoint=np.full(n, -1, np.int32), x3D=np.zeros((n, 3), np.float32), counts=np.zeros(3, np.int32))
        a = arr[i]
        a.depth, a.keys, a.held = depth.ctypes.data, keys.ctypes.data, held.ctypes.data
        a.outlier = None if outlier is None else outlier.ctypes.data
        a.created_keypoint, a.x3D, a.counts = o["created_keypoint"].ctypes.data, o["x3D"].ctypes.data, o["counts"].ctypes.data
        a.Rwc = (C.c_float * 9)(*np.asarray(f["Rwc"], np.float32).reshape(9))
        a.Ow = (C.c_float * 3)(*np.asarray(f["Ow"], np.float32).reshape(3))
        a.th_depth, a.n, a.max_point, a.mode = float(np.float32(f["th_depth"])), n, int(f.get("max_point", 100)), int(f.get("mode", STEREO_POINTS_CLOSEST))
        keep.append((depth, keys, held, outlier))
        outs.append(o)
    return arr, outs, keep


def _stereo_points_results(outs):
    res = []
    for o in outs:
        k = int(o["counts"][0])
        res.append(dict(created_keypoint=o["created_keypoint"][:k].copy(), x3D=o["x3D"][:k].copy(), n_created=k, n_visited=int(o["counts"][1]),
                        n_with_depth=int(o["counts"][2])))
    return res


def stereo_points_batch(frames, unproject4, host=False, stream=0):
    """The stereo map points of ``Tracking::CreateNewKeyFrame`` / ``UpdateLastFrame`` (mode STEREO_POINTS_CLOSEST) or
    ``StereoInitialization`` (STEREO_POINTS_ALL), one frame per dict (pack_stereo_points_frames); unproject4 = (cx, cy, invfx, invfy) ->
    one dict per frame: created_keypoint [n_created], x3D [n_created, 3] in creation order, n_created, n_visited, n_with_depth.
    host=True runs the reference's loops on the CPU."""
    arr, outs, keep = pack_stereo_points_frames(frames)
    u = np.ascontiguousarray(unproject4, np.float32).reshape(4)
    if host:
        f = lib().tc2li_host_stereo_points_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(frames), u.ctypes.data))
    else:
        f = lib().tc2li_stereo_points_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(C.addressof(arr), len(frames), u.ctypes.data, C.c_void_p(stream)))
    del keep
    return _stereo_points_results(outs)


def new_keyframe_batch(frames, decisions, unproject4, host=False, stream=0):
    """``Tracking::NeedNewKeyFrame`` per frame and, where it says yes and create_blocked is 0, the new keyframe's stereo points.  frames as
    for stereo_points_batch (outlier required); decisions: dicts with the scalars of tc2li_keyframe_decision (default 0) and optionally
    ref_nobs -> one dict per frame: the fields of stereo_points_batch plus need, interrupt_ba, conditions, exit_rule, n_tracked_close,
    n_non_tracked_close, n_ref_matches."""
    if len(frames) != len(decisions):
        raise ValueError("%d frames, %d decisions" % (len(frames), len(decisions)))
    arr, outs, keep = pack_stereo_points_frames(frames)
    dec, ver = (KeyframeDecision * max(len(frames), 1))(), (KeyframeVerdict * max(len(frames), 1))()
    for i, d in enumerate(decisions):
        for k in _DECISION_SCALARS:
            v = d.get(k, 0)
            setattr(dec[i], k, float(v) if k.startswith("time_") else int(v))
        if d.get("ref_nobs") is not None:
            r = np.ascontiguousarray(d["ref_nobs"], np.int32).reshape(-1)
            keep.append(r)
            dec[i].ref_nobs, dec[i].n_ref = r.ctypes.data, len(r)
    u = np.ascontiguousarray(unproject4, np.float32).reshape(4)
    if host:
        f = lib().tc2li_host_new_keyframe_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), C.addressof(dec), C.addressof(ver), len(frames), u.ctypes.data))
    else:
        f = lib().tc2li_new_keyframe_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(C.addressof(arr), C.addressof(dec), C.addressof(ver), len(frames), u.ctypes.data, C.c_void_p(stream)))
    del keep
    res = _stereo_points_results(outs)
    for r, v in zip(res, ver):
        r.update({k: int(getattr(v, k)) for k, _ in KeyframeVerdict._fields_ if k != "pad_"})
    return res


class ConnectionsProblem(C.Structure):
    """tc2li_connections_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_flags", "conn_offsets", "conn_kf", "conn_weight", "slot_point", "point_bad", "obs_offsets", "obs_kf",
                                          "counts", "counter_kf", "counter_weight", "ordered_kf", "ordered_weight", "touched_kf", "touched_changed",
                                          "changed_offsets", "changed_kf", "changed_weight")] \
        + [(k, C.c_int32) for k in ("n_keyframes", "n_slots", "n_points", "current", "counter_capacity", "ordered_capacity", "changed_capacity")] \
        + [("first_connection", C.c_uint8), ("is_init_kf", C.c_uint8), ("pad_", C.c_uint8 * 2)]


CONNECTIONS_UNCHANGED, CONNECTIONS_UPDATED, CONNECTIONS_TH = 0, 1, 15
_CONNECTIONS_ARRAYS = (("kf_flags", np.uint8), ("conn_offsets", np.int32), ("conn_kf", np.int32), ("conn_weight", np.int32), ("slot_point", np.int32),
                       ("point_bad", np.uint8), ("obs_offsets", np.int32), ("obs_kf", np.int32))
_CONNECTIONS_COUNTS = ("status", "n_counter", "n_ordered", "n_changed", "n_changed_entries", "parent")


def connections_limits():
    """tc2li_connections_limits -> {lds_keyframes, rank_lanes, vote_threads}: the sizes at which the device path of update_connections_batch
    changes (the vote counters leave LDS above lds_keyframes keyframes; a wavefront of rank_lanes orders a list)."""
    out = (C.c_int32 * 3)()
    f = lib().tc2li_connections_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 3))
    return dict(zip(("lds_keyframes", "rank_lanes", "vote_threads"), [int(v) for v in out]))


def pack_connections_problems(problems, fill=0):
    """The tc2li_connections_problem array of a batch with its output arrays (prefilled with `fill`) -> (array, outputs per problem, what must
    stay alive).  Capacities: counter_capacity / ordered_capacity / changed_capacity of the problem's dict, by default what can never be too
    small (n_keyframes, n_keyframes, every row one longer)."""
    P = len(problems)
    arr, outs, keep = (ConnectionsProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], t).reshape(-1) for k, t in _CONNECTIONS_ARRAYS}
        nk, ns, npts = len(a["kf_flags"]), len(a["slot_point"]), len(a["point_bad"])
        if len(a["conn_offsets"]) != nk + 1 or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: conn_offsets or obs_offsets do not fit the tables" % i)
        nc, no = int(a["conn_offsets"][-1]), int(a["obs_offsets"][-1])
        if min(len(a["conn_kf"]), len(a["conn_weight"])) < nc or len(a["obs_kf"]) < no:
            raise ValueError("problem %d: conn or observation arrays are shorter than their offsets say" % i)
        cc, oc, hc = (int(p.get(k, d)) for k, d in (("counter_capacity", nk), ("ordered_capacity", nk), ("changed_capacity", nc + nk)))
        full = lambda n, t: np.full(max(n, 0), fill, np.int64).astype(t)
        o = dict(counts=full(8, np.int32), counter_kf=full(cc, np.int32), counter_weight=full(cc, np.int32), ordered_kf=full(oc, np.int32),
                 ordered_weight=full(oc, np.int32), touched_kf=full(oc, np.int32), touched_changed=full(oc, np.uint8),
                 changed_offsets=full(oc + 1, np.int32), changed_kf=full(hc, np.int32), changed_weight=full(hc, np.int32))
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        arr[i].n_keyframes, arr[i].n_slots, arr[i].n_points, arr[i].current = nk, ns, npts, int(p["current"])
        arr[i].counter_capacity, arr[i].ordered_capacity, arr[i].changed_capacity = cc, oc, hc
        arr[i].first_connection, arr[i].is_init_kf = int(bool(p.get("first_connection", 0))), int(bool(p.get("is_init_kf", 0)))
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def update_connections_batch(problems, host=False, stream=0, raw=False, fill=0):
    """One ``KeyFrame::UpdateConnections`` call per problem.  problems: dicts with the arrays of tc2li_connections_problem (kf_flags,
    conn_offsets, conn_kf, conn_weight, slot_point, point_bad, obs_offsets, obs_kf), current and optionally first_connection, is_init_kf and
    the three capacities -> one dict per problem: status, parent, counter_kf, counter_weight, ordered_kf, ordered_weight, touched_kf,
    touched_changed, changed_offsets [n_changed + 1], changed_kf, changed_weight, cut to their counts.  raw=True: the arrays at their full
    capacity as the library left them (prefilled with `fill`) and counts.  host=True walks the same graph on the CPU."""
    arr, outs, keep = pack_connections_problems(problems, fill)
    if host:
        f = lib().tc2li_host_update_connections_batch
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(C.addressof(arr), len(problems)))
    else:
        f = lib().tc2li_update_connections_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), len(problems), C.c_void_p(stream)))
    del keep
    if raw:
        return outs
    res = []
    for o in outs:
        c = dict(zip(_CONNECTIONS_COUNTS, [int(v) for v in o["counts"][:6]]))
        r = dict(status=c["status"], parent=c["parent"])
        for k, n in (("counter_kf", "n_counter"), ("counter_weight", "n_counter"), ("ordered_kf", "n_ordered"), ("ordered_weight", "n_ordered"),
                     ("touched_kf", "n_ordered"), ("touched_changed", "n_ordered"), ("changed_kf", "n_changed_entries"),
                     ("changed_weight", "n_changed_entries")):
            r[k] = o[k][:c[n]]
        r["changed_offsets"] = o["changed_offsets"][:c["n_changed"] + 1] if c["status"] else np.zeros(1, np.int32)
        res.append(r)
    return res


# ---- LocalMapping::ProcessNewKeyFrame (tc2li_process_new_keyframe_batch) -------------------------------------------------------------------
_PROCESS_KEYFRAME_INPUTS = (("kf_slot", np.int32), ("centres", np.float32), ("positions", np.float32), ("point_nobs", np.int32), ("point_ref_kf", np.int32),
                            ("point_ref_level_scale", np.float32), ("obs_index", np.int32))
_PROCESS_KEYFRAME_OUTPUTS = ("counts", "associated_slot", "associated_point", "recent", "point_nobs_out", "obs_offsets_out", "obs_kf_out", "obs_index_out",
                             "desc_kf", "desc_index", "refreshed", "normals_out", "min_distance_out", "max_distance_out")
PROCESS_KEYFRAME_COUNTS = ("status", "associated", "recent", "observations")
PROCESS_KEYFRAME_ON_DEVICE, PROCESS_KEYFRAME_ON_HOST = 0, 1
_PROCESS_KEYFRAME_CAPACITIES = ("associated", "recent", "observations", "counter", "ordered", "changed")


class ProcessKeyframeProblem(C.Structure):
    """tc2li_process_keyframe_problem"""
    _fields_ = [("conn", ConnectionsProblem)] + [(k, C.c_void_p) for k, _ in _PROCESS_KEYFRAME_INPUTS] + [(k, C.c_void_p) for k in _PROCESS_KEYFRAME_OUTPUTS] \
        + [(k, C.c_int32) for k in ("associated_capacity", "recent_capacity", "obs_capacity")] + [("last_level_scale", C.c_float)]


def process_new_keyframe_limits():
    """tc2li_process_new_keyframe_limits -> {observations, keypoints, threads, refresh_waves}: a problem in which a point would pass
    ``observations`` is computed by the host twin inside ``process_new_keyframe_batch``."""
    out = np.zeros(8, np.int32)
    f = lib().tc2li_process_new_keyframe_limits
    f.argtypes = [C.c_void_p, C.c_int]
    n = _check(f(out.ctypes.data, len(out)))
    return dict(zip(("observations", "keypoints", "threads", "refresh_waves"), [int(v) for v in out[:n]]))


def pack_process_keyframe_problems(problems, capacities=None):
    """The tc2li_process_keyframe_problem array of a batch with its output arrays -> (array, outputs per problem, what must stay alive).
    problems: dicts with the input arrays of tc2li_connections_problem (kf_flags, conn_offsets, conn_kf, conn_weight, slot_point, point_bad,
    obs_offsets, obs_kf: the observation rows on entry), kf_slot, centres [n, 3], positions [n, 3], point_nobs, point_ref_kf,
    point_ref_level_scale, obs_index, and current, last_level_scale, optionally first_connection, is_init_kf.  capacities: per problem a dict
    with associated / recent / observations / counter / ordered / changed; default: what always suffices.  The outputs of the connection
    half are in the dict under conn_counts and tc2li_connections_problem's names."""
    P = len(problems)
    arr, outs, keep = (ProcessKeyframeProblem * max(P, 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], t).reshape(-1) for k, t in _CONNECTIONS_ARRAYS + _PROCESS_KEYFRAME_INPUTS}
        nk, ns, npts = len(a["kf_flags"]), len(a["slot_point"]), len(a["point_bad"])
        if len(a["conn_offsets"]) != nk + 1 or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: conn_offsets or obs_offsets do not fit the tables" % i)
        nc, no = int(a["conn_offsets"][-1]), int(a["obs_offsets"][-1])
        if min(len(a["conn_kf"]), len(a["conn_weight"])) < nc or min(len(a["obs_kf"]), len(a["obs_index"])) < no:
            raise ValueError("problem %d: conn or observation arrays are shorter than their offsets say" % i)
        if len(a["kf_slot"]) != nk or len(a["centres"]) != 3 * nk:
            raise ValueError("problem %d: kf_slot or centres do not have %d rows" % (i, nk))
        for k, w in (("positions", 3), ("point_nobs", 1), ("point_ref_kf", 1), ("point_ref_level_scale", 1)):
            if len(a[k]) != w * npts:
                raise ValueError("problem %d: %s does not have %d rows" % (i, k, npts))
        occupied = int((a["slot_point"] >= 0).sum())
        cap = dict(associated=occupied, recent=occupied, observations=no + occupied, counter=nk, ordered=nk, changed=nc + nk)
        cap.update((capacities[i] if capacities is not None else None) or {})
        o = dict(counts=np.zeros(len(PROCESS_KEYFRAME_COUNTS), np.int32), associated_slot=np.full(cap["associated"], -2, np.int32),
                 associated_point=np.full(cap["associated"], -2, np.int32), recent=np.full(cap["recent"], -2, np.int32), point_nobs_out=np.full(npts, -2, np.int32),
                 obs_offsets_out=np.full(npts + 1, -2, np.int32), obs_kf_out=np.full(cap["observations"], -2, np.int32),
                 obs_index_out=np.full(cap["observations"], -2, np.int32), desc_kf=np.full(npts, -2, np.int32), desc_index=np.full(npts, -2, np.int32),
                 refreshed=np.zeros(npts, np.uint8), normals_out=np.zeros((npts, 3), np.float32), min_distance_out=np.zeros(npts, np.float32),
                 max_distance_out=np.zeros(npts, np.float32))
        co = dict(conn_counts=np.full(8, -2, np.int32), counter_kf=np.full(cap["counter"], -2, np.int32), counter_weight=np.full(cap["counter"], -2, np.int32),
                  ordered_kf=np.full(cap["ordered"], -2, np.int32), ordered_weight=np.full(cap["ordered"], -2, np.int32), touched_kf=np.full(cap["ordered"], -2, np.int32),
                  touched_changed=np.full(cap["ordered"], 254, np.uint8), changed_offsets=np.full(cap["ordered"] + 1, -2, np.int32),
                  changed_kf=np.full(cap["changed"], -2, np.int32), changed_weight=np.full(cap["changed"], -2, np.int32))
        for k, _ in _CONNECTIONS_ARRAYS:
            setattr(arr[i].conn, k, a[k].ctypes.data)
        for k, v in co.items():
            setattr(arr[i].conn, "counts" if k == "conn_counts" else k, v.ctypes.data if v.size else None)
        arr[i].conn.n_keyframes, arr[i].conn.n_slots, arr[i].conn.n_points, arr[i].conn.current = nk, ns, npts, int(p["current"])
        arr[i].conn.counter_capacity, arr[i].conn.ordered_capacity, arr[i].conn.changed_capacity = cap["counter"], cap["ordered"], cap["changed"]
        arr[i].conn.first_connection, arr[i].conn.is_init_kf = int(bool(p.get("first_connection", 0))), int(bool(p.get("is_init_kf", 0)))
        for k, _ in _PROCESS_KEYFRAME_INPUTS:
            setattr(arr[i], k, a[k].ctypes.data if a[k].size else None)
        for k, v in o.items():
            setattr(arr[i], k, v.ctypes.data if v.size else None)
        arr[i].associated_capacity, arr[i].recent_capacity, arr[i].obs_capacity = cap["associated"], cap["recent"], cap["observations"]
        arr[i].last_level_scale = float(p["last_level_scale"])
        keep.append(a)
        outs.append(dict(o, **co))
    return arr, outs, keep


def run_process_new_keyframe_batch(arr, n_problems, store=None, views=None, stream=0):
    """tc2li_process_new_keyframe_batch on ``store`` or, with ``views`` (per slot None or a dict with descriptors and u_right),
    tc2li_host_process_new_keyframe_batch -> the call's return value (no exception: the caller reads the code)."""
    if store is not None:
        f = lib().tc2li_process_new_keyframe_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return f(store._handle(), C.addressof(arr), int(n_problems), C.c_void_p(stream))
    varr, keep = (KeyframeView * max(len(views), 1))(), []
    for i, v in enumerate(views):
        if v is None:
            varr[i].n = -1
            continue
        d, ur = np.ascontiguousarray(v["descriptors"], np.uint8).reshape(-1, 32), np.ascontiguousarray(v["u_right"], np.float32)
        if len(d) != len(ur):
            raise ValueError("view %d: one u_right per descriptor" % i)
        keep.append((d, ur))
        varr[i].n, varr[i].descriptors, varr[i].u_right = len(d), d.ctypes.data, ur.ctypes.data
    f = lib().tc2li_host_process_new_keyframe_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    rc = f(C.addressof(varr), len(views), C.addressof(arr), int(n_problems))
    del keep
    return rc


def _process_keyframe_results(outs):
    res = []
    for o in outs:
        c = dict(zip(PROCESS_KEYFRAME_COUNTS, [int(v) for v in o["counts"]]))
        k = dict(zip(_CONNECTIONS_COUNTS, [int(v) for v in o["conn_counts"][:6]]))
        r = dict(o, counts=c, status=c["status"], associated_slot=o["associated_slot"][:c["associated"]], associated_point=o["associated_point"][:c["associated"]],
                 recent=o["recent"][:c["recent"]], obs_kf_out=o["obs_kf_out"][:c["observations"]], obs_index_out=o["obs_index_out"][:c["observations"]])
        conn = dict(status=k["status"], parent=k["parent"])
        for name, n in (("counter_kf", "n_counter"), ("counter_weight", "n_counter"), ("ordered_kf", "n_ordered"), ("ordered_weight", "n_ordered"),
                        ("touched_kf", "n_ordered"), ("touched_changed", "n_ordered"), ("changed_kf", "n_changed_entries"), ("changed_weight", "n_changed_entries")):
            conn[name] = o[name][:k[n]]
            del r[name]
        conn["changed_offsets"] = o["changed_offsets"][:k["n_changed"] + 1] if k["status"] else np.zeros(1, np.int32)
        del r["changed_offsets"], r["conn_counts"]
        r["connections"] = conn
        res.append(r)
    return res


def process_new_keyframe_batch(problems, store=None, views=None, stream=0, capacities=None):
    """One ``LocalMapping::ProcessNewKeyFrame`` per problem (``tc2li_process_new_keyframe_batch``; with ``views`` in place of ``store`` the
    host twin) -> one dict per problem: counts (dict), status, associated_slot, associated_point, recent, point_nobs_out, obs_offsets_out,
    obs_kf_out, obs_index_out, desc_kf, desc_index, refreshed, normals_out, min_distance_out, max_distance_out, and connections: the dict
    ``update_connections_batch`` returns."""
    if (store is None) == (views is None):
        raise ValueError("either a store (the device entry) or views (the host entry)")
    arr, outs, keep = pack_process_keyframe_problems(problems, capacities)
    _check(run_process_new_keyframe_batch(arr, len(problems), store, views, stream))
    del keep
    return _process_keyframe_results(outs)


def update_best_covisibles_batch(rows, bad, host=False, stream=0):
    """``KeyFrame::UpdateBestCovisibles`` for a flat list of keyframes of any number of sequences.  rows: dict with the CSR offsets, kf, weight of
    their mConnectedKeyFrameWeights (a row ascends by kf); bad [n_keyframes]: isBad() of every keyframe the rows name -> dict offsets, kf,
    weight: the ordered lists without the bad keyframes.  host=True orders on the CPU."""
    off, kf, w = (np.ascontiguousarray(rows[k], np.int32).reshape(-1) for k in ("offsets", "kf", "weight"))
    b = np.ascontiguousarray(bad, np.uint8).reshape(-1)
    n = len(off) - 1
    if n < 0 or min(len(kf), len(w)) < int(off[-1]):
        raise ValueError("offsets are empty or kf / weight are shorter than they say")
    out_off, out_kf, out_w = np.zeros(n + 1, np.int32), np.zeros(int(off[-1]), np.int32), np.zeros(int(off[-1]), np.int32)
    args = [off.ctypes.data, kf.ctypes.data, w.ctypes.data, n, b.ctypes.data, len(b), out_off.ctypes.data, out_kf.ctypes.data, out_w.ctypes.data]
    if host:
        f = lib().tc2li_host_update_best_covisibles_batch
        f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _check(f(*args))
    else:
        f = lib().tc2li_update_best_covisibles_batch
        f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _check(f(*(args + [C.c_void_p(stream)])))
    m = int(out_off[-1])
    return dict(offsets=out_off, kf=out_kf[:m], weight=out_w[:m])


class BaWindowProblem(C.Structure):
    """tc2li_ba_window_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_slot", "kf_id", "kf_flags", "poses7", "slot_offsets", "slot_point", "cov_kf", "point_flags", "positions",
                                          "obs_offsets", "obs_kf", "obs_index", "counts", "pose_row", "poses7_out", "fixed", "point_row", "points3_out",
                                          "edges", "lidar_pose_index")] \
        + [("init_kf_id", C.c_int64)] \
        + [(k, C.c_int32) for k in ("n_keyframes", "n_points", "n_cov", "current", "pose_capacity", "point_capacity", "edge_capacity", "pad_")]


BA_WINDOW_OK, BA_WINDOW_ABORTED, BA_WINDOW_MAX_LIDAR = 0, 1, 6
_BA_WINDOW_ARRAYS = (("kf_slot", np.int32), ("kf_id", np.int64), ("kf_flags", np.uint8), ("poses7", np.float64), ("slot_offsets", np.int32),
                     ("slot_point", np.int32), ("cov_kf", np.int32), ("point_flags", np.uint8), ("positions", np.float64), ("obs_offsets", np.int32),
                     ("obs_kf", np.int32), ("obs_index", np.int32))
_BA_WINDOW_COUNTS = ("status", "num_fixed_kf", "num_opt_kf", "n_poses", "n_points", "n_edges", "n_lidar", "n_points_without_edge")


def ba_window_limits():
    """tc2li_ba_window_limits -> {lds_keyframes, lds_points, threads}: the sizes at which the device path of ba_window_batch changes (the
    keyframe marks leave LDS above lds_keyframes keyframes, the first-occurrence keys above lds_points points)."""
    out = (C.c_int32 * 3)()
    f = lib().tc2li_ba_window_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 3))
    return dict(zip(("lds_keyframes", "lds_points", "threads"), [int(v) for v in out]))


def pack_ba_window_problems(problems, fill=0):
    """The tc2li_ba_window_problem array of a batch with its output arrays (prefilled with `fill`) -> (array, outputs per problem, what must
    stay alive).  Capacities: pose_capacity / point_capacity / edge_capacity of the problem's dict, by default what can never be too small
    (the keyframes, the points, the observations)."""
    arr, outs, keep = (BaWindowProblem * max(len(problems), 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], t).reshape(-1) for k, t in _BA_WINDOW_ARRAYS}
        nk, npts = len(a["kf_slot"]), len(a["point_flags"])
        if len(a["kf_id"]) != nk or len(a["kf_flags"]) != nk or len(a["poses7"]) != 7 * nk or len(a["slot_offsets"]) != nk + 1:
            raise ValueError("problem %d: the keyframe arrays do not have one row per keyframe" % i)
        if len(a["positions"]) != 3 * npts or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: the point arrays do not have one row per point" % i)
        ns, no = int(a["slot_offsets"][-1]), int(a["obs_offsets"][-1])
        if len(a["slot_point"]) < ns or min(len(a["obs_kf"]), len(a["obs_index"])) < no:
            raise ValueError("problem %d: slot or observation arrays are shorter than their offsets say" % i)
        pc, tc, ec = (int(p.get(k, d)) for k, d in (("pose_capacity", nk), ("point_capacity", npts), ("edge_capacity", no)))
        full = lambda n, t: np.full(max(n, 0), fill, np.int64).astype(t)
        edges = np.zeros(max(ec, 0), BA_EDGE_DTYPE)
        edges.view(np.uint8)[:] = fill & 0xff
        o = dict(counts=full(8, np.int32), pose_row=full(pc, np.int32), poses7_out=full(7 * pc, np.float64), fixed=full(pc, np.uint8),
                 point_row=full(tc, np.int32), points3_out=full(3 * tc, np.float64), edges=edges, lidar_pose_index=full(BA_WINDOW_MAX_LIDAR, np.int32))
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        arr[i].init_kf_id = int(p["init_kf_id"])
        arr[i].n_keyframes, arr[i].n_points, arr[i].n_cov, arr[i].current = nk, npts, len(a["cov_kf"]), int(p["current"])
        arr[i].pose_capacity, arr[i].point_capacity, arr[i].edge_capacity = pc, tc, ec
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def _pack_ba_window_views(views):
    """views: per slot None (empty) or a dict with keys (KEYPOINT_DTYPE) and u_right -> (tc2li_keyframe_view array with n, keys, u_right, keep)."""
    arr, keep = (KeyframeView * max(len(views), 1))(), []
    for i, v in enumerate(views):
        if v is None:
            arr[i].n = -1
            continue
        k, ur = np.ascontiguousarray(v["keys"], KEYPOINT_DTYPE), np.ascontiguousarray(v["u_right"], np.float32)
        if len(k) != len(ur):
            raise ValueError("view %d: one u_right per keypoint" % i)
        keep.append((k, ur))
        arr[i].n, arr[i].keys, arr[i].u_right = len(k), k.ctypes.data, ur.ctypes.data
    return arr, keep


def ba_window_batch(problems, inv_level_sigma2, store=None, views=None, stream=0, raw=False, fill=0):
    """The gather of ``OptimizerWithLidar::LocalLVBundleAdjustment`` (the window of the local BA), one per problem.  problems: dicts with the
    arrays of tc2li_ba_window_problem (kf_slot, kf_id, kf_flags, poses7, slot_offsets, slot_point, cov_kf, point_flags, positions, obs_offsets,
    obs_kf, obs_index), current, init_kf_id and optionally the three capacities.  store: a :class:`KeyframeStore` -- the device entry; views:
    per slot None or a dict with keys and u_right -- the host entry.  -> one dict per problem: status, num_fixed_kf, num_opt_kf, n_lidar,
    n_points_without_edge, pose_row, poses7 [n, 7], fixed, point_row, points3 [n, 3], edges (BA_EDGE_DTYPE), lidar_pose_index [n_lidar], cut to
    their counts.  raw=True: the arrays at their full capacity as the library left them (prefilled with `fill`) and counts."""
    if (store is None) == (views is None):
        raise ValueError("either a store (the device entry) or views (the host entry)")
    arr, outs, keep = pack_ba_window_problems(problems, fill)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    if views is not None:
        varr, vkeep = _pack_ba_window_views(views)
        f = lib().tc2li_host_ba_window_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _check(f(C.addressof(varr), len(views), C.addressof(arr), len(problems), sg.ctypes.data, len(sg)))
        del vkeep
    else:
        f = lib().tc2li_ba_window_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(store._handle(), C.addressof(arr), len(problems), sg.ctypes.data, len(sg), C.c_void_p(stream)))
    del keep
    if raw:
        return outs
    res = []
    for o in outs:
        c = dict(zip(_BA_WINDOW_COUNTS, [int(v) for v in o["counts"]]))
        r = {k: c[k] for k in ("status", "num_fixed_kf", "num_opt_kf", "n_lidar", "n_points_without_edge")}
        r.update(pose_row=o["pose_row"][:c["n_poses"]], poses7=o["poses7_out"].reshape(-1, 7)[:c["n_poses"]], fixed=o["fixed"][:c["n_poses"]],
                 point_row=o["point_row"][:c["n_points"]], points3=o["points3_out"].reshape(-1, 3)[:c["n_points"]], edges=o["edges"][:c["n_edges"]],
                 lidar_pose_index=o["lidar_pose_index"][:c["n_lidar"]])
        res.append(r)
    return res


def ba_window_outliers(edges, edge_chi2, edge_depth_positive, point_bad_now, capacity=None):
    """tc2li_ba_window_outliers: vToErase of the local BA as (pose index, point index) pairs [n, 2] in the reference's order -- the monocular
    edges over 5.991 or behind the camera, then the stereo edges with 7.815; edges of points that are bad by now are skipped."""
    e = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    chi2, dpos = np.ascontiguousarray(edge_chi2, np.float64).reshape(-1), np.ascontiguousarray(edge_depth_positive, np.uint8).reshape(-1)
    bad = np.ascontiguousarray(point_bad_now, np.uint8).reshape(-1)
    if min(len(chi2), len(dpos)) < len(e):
        raise ValueError("one chi2 and one depth flag per edge")
    cap = len(e) if capacity is None else int(capacity)
    pose, point = np.full(max(cap, 0), -1, np.int32), np.full(max(cap, 0), -1, np.int32)
    f = lib().tc2li_ba_window_outliers
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    n = _check(f(e.ctypes.data, chi2.ctypes.data, dpos.ctypes.data, len(e), bad.ctypes.data, len(bad), pose.ctypes.data, point.ctypes.data, cap))
    return np.stack([pose[:n], point[:n]], 1)


BA_STRUCTURE_FIELDS = ("scalars", "pose_var", "pt_off", "pt_edges", "pv_off", "pv_edges", "fl_off", "fl_pose", "fl_lm", "fl_place", "fl_edge", "w_slot",
                       "slice_off", "dup_off", "dup_edge", "dup_slot", "blk_off", "blk_rows", "grp_k0", "grp_l0", "chunk_mask")
BA_STRUCTURE_SCALARS = ("n_free", "n_slots", "n_free_pose_edges", "n_dups", "n_blocks", "n_groups", "max_group_landmarks", "np", "np_pad",
                        "n_schur_slices", "n_slices", "k_per_slice", "schur_group", "sparse", "schur_rd", "schur_ro")


def unpack_ba_structure(table, out):
    """The flat form of tc2li_host_ba_structure (table [fields][2], one int32 buffer) -> a dict: every scalar of BA_STRUCTURE_SCALARS as an
    int, every other field of BA_STRUCTURE_FIELDS as an int32 array of its count."""
    t = np.asarray(table, np.int32).reshape(len(BA_STRUCTURE_FIELDS), 2)
    r = {k: np.array(out[t[i, 0]:t[i, 0] + t[i, 1]], np.int32) for i, k in enumerate(BA_STRUCTURE_FIELDS)}
    r.update(zip(BA_STRUCTURE_SCALARS, [int(v) for v in r.pop("scalars")]))
    return r


def host_ba_structure(fixed, n_points, edges, extra_used=None):
    """tc2li_host_ba_structure: the index structure the local BA builds from (fixed, edges) -- see unpack_ba_structure.  edges: BA_EDGE_DTYPE
    (point and pose are read); extra_used [n_poses]: poses that count as used without an edge.  Needs no device."""
    fx, e = np.ascontiguousarray(fixed, np.uint8).reshape(-1), np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    xu = None if extra_used is None else np.ascontiguousarray(extra_used, np.uint8).reshape(-1)
    if xu is not None and len(xu) != len(fx):
        raise ValueError("one extra_used flag per pose")
    table = np.zeros((len(BA_STRUCTURE_FIELDS), 2), np.int32)
    f = lib().tc2li_host_ba_structure
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    args = [fx.ctypes.data, len(fx), int(n_points), e.ctypes.data, len(e), None if xu is None else xu.ctypes.data, table.ctypes.data]
    n = _check(f(*(args + [None, 0])))
    out = np.full(max(n, 1), -7, np.int32)
    assert _check(f(*(args + [out.ctypes.data, n]))) == n
    return unpack_ba_structure(table, out)


BA_STRUCTURE_DECLINED = -1000


def ba_window_solve_limits():
    """tc2li_ba_window_solve_limits -> {max_free, max_poses, max_points, threads}: the range in which a window's structure is built on the
    device; a window beyond it is declined."""
    out = (C.c_int32 * 4)()
    f = lib().tc2li_ba_window_solve_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 4))
    return dict(zip(("max_free", "max_poses", "max_points", "threads"), [int(v) for v in out]))


def _cut_ba_window_outputs(o):
    """The output arrays of one tc2li_ba_window_problem cut to their counts, as ba_window_batch returns them (edges: None stays None)
    -> (the dict, the counts by name)."""
    c = dict(zip(_BA_WINDOW_COUNTS, [int(v) for v in o["counts"]]))
    r = {k: c[k] for k in ("status", "num_fixed_kf", "num_opt_kf", "n_lidar", "n_points_without_edge")}
    r.update(pose_row=o["pose_row"][:c["n_poses"]], poses7=o["poses7_out"].reshape(-1, 7)[:c["n_poses"]], fixed=o["fixed"][:c["n_poses"]],
             point_row=o["point_row"][:c["n_points"]], points3=o["points3_out"].reshape(-1, 3)[:c["n_points"]],
             edges=None if o["edges"] is None else o["edges"][:c["n_edges"]], lidar_pose_index=o["lidar_pose_index"][:c["n_lidar"]])
    return r, c


def ba_window_structure_batch(problems, inv_level_sigma2, store, with_lidar=None, stream=0, out_stride=None):
    """tc2li_ba_window_structure_batch: the gather of ba_window_batch on the device followed by the optimiser's index structure of every
    window, built on the device from the gather's device output and read back from the windows' input blocks.  -> (the gather's results as
    ba_window_batch returns them, per problem the structure as unpack_ba_structure returns it -- the fields a sparse window's block does not
    hold are empty -- or the result code: 0 ABORTED, -2 refused as the BA would refuse it, BA_STRUCTURE_DECLINED outside the device range)."""
    arr, outs, keep = pack_ba_window_problems(problems, 0)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    n = len(problems)
    wl = None if with_lidar is None else np.ascontiguousarray(with_lidar, np.uint8).reshape(-1)
    if wl is not None and len(wl) != n:
        raise ValueError("one with_lidar flag per problem")
    if out_stride is None:   # no structure is larger: every field is bounded by the tables of its problem
        out_stride = max([len(BA_STRUCTURE_SCALARS) + 600 + 2 * arr[i].pose_capacity + 6 * arr[i].point_capacity + 8 * arr[i].edge_capacity for i in range(n)] + [1])
    tables = np.zeros((max(n, 1), len(BA_STRUCTURE_FIELDS), 2), np.int32)
    out, results = np.full((max(n, 1), out_stride), -7, np.int32), np.zeros(max(n, 1), np.int32)
    f = lib().tc2li_ba_window_structure_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _check(f(store._handle(), C.addressof(arr), n, sg.ctypes.data, len(sg), None if wl is None else wl.ctypes.data, tables.ctypes.data,
             out.ctypes.data, out_stride, results.ctypes.data, C.c_void_p(stream)))
    del keep
    gathered = [_cut_ba_window_outputs(o)[0] for o in outs]
    return gathered, [unpack_ba_structure(tables[i], out[i]) if results[i] > 0 else int(results[i]) for i in range(n)]


class BaWindowSolveProblem(C.Structure):
    """tc2li_ba_window_solve_problem"""
    _fields_ = [("window", BaWindowProblem)] \
        + [(k, C.c_void_p) for k in ("stop_flag", "stats", "edge_chi2", "edge_depth_positive", "cloud_offsets", "cloud_xyz", "lidar_stats", "erase_pose",
                                     "erase_point", "n_erase")] \
        + [("lambda_init", C.c_double), ("weight", C.c_double), ("Tcl", C.c_float * 7)] \
        + [(k, C.c_int32) for k in ("iterations", "edge_out_capacity", "erase_capacity")]


def pack_ba_window_solve_problems(problems, fill=0):
    """The tc2li_ba_window_solve_problem array of a batch -> (array, outputs per problem, what must stay alive).  problems: the dicts of
    pack_ba_window_problems plus, all optional: iterations (10), lambda_init (0), stop_flag (a uint8 array of one element), want_edges
    (True; False passes edges = NULL), want_chi2 (True: edge_chi2 and edge_depth_positive are asked for), edge_out_capacity and
    erase_capacity (the observations), clouds (per keyframe row None or [n, 3] points) with Tcl7 and weight (1)."""
    warr, wouts, wkeep = pack_ba_window_problems(problems, fill)
    n = len(problems)
    arr, outs, keep = (BaWindowSolveProblem * max(n, 1))(), [], [wkeep]
    stats, lstats = (BaStats * max(n, 1))(), (LidarBaStats * max(n, 1))()
    keep += [stats, lstats]
    for i, p in enumerate(problems):
        q, o = arr[i], dict(wouts[i])
        C.memmove(C.addressof(q.window), C.addressof(warr[i]), C.sizeof(BaWindowProblem))
        n_obs = int(np.asarray(p["obs_offsets"]).reshape(-1)[-1])
        if not p.get("want_edges", True):
            q.window.edges = None
            o["edges"] = None
        ec, rc = int(p.get("edge_out_capacity", n_obs)), int(p.get("erase_capacity", n_obs))
        full = lambda m, t: np.full(max(m, 0), fill, np.int64).astype(t)
        o.update(erase_pose=full(rc, np.int32), erase_point=full(rc, np.int32), n_erase=full(1, np.int32), stats=stats[i], lidar_stats=lstats[i])
        q.erase_pose, q.erase_point, q.n_erase, q.erase_capacity = o["erase_pose"].ctypes.data, o["erase_point"].ctypes.data, o["n_erase"].ctypes.data, rc
        q.stats, q.lidar_stats = C.addressof(stats) + i * C.sizeof(BaStats), C.addressof(lstats) + i * C.sizeof(LidarBaStats)
        q.edge_out_capacity = ec
        if p.get("want_chi2", True):
            o.update(edge_chi2=np.full(max(ec, 0), float(fill)), edge_depth_positive=full(ec, np.uint8))
            q.edge_chi2, q.edge_depth_positive = o["edge_chi2"].ctypes.data, o["edge_depth_positive"].ctypes.data
        else:
            o.update(edge_chi2=None, edge_depth_positive=None)
        q.iterations, q.lambda_init = int(p.get("iterations", 10)), float(p.get("lambda_init", 0.0))
        if p.get("stop_flag") is not None:
            q.stop_flag = p["stop_flag"].ctypes.data
            keep.append(p["stop_flag"])
        if p.get("clouds") is not None:
            cl = [np.zeros((0, 3), np.float32) if c is None else np.asarray(c, np.float32).reshape(-1, 3) for c in p["clouds"]]
            if len(cl) != q.window.n_keyframes:
                raise ValueError("problem %d: one cloud (or None) per keyframe row" % i)
            off = np.concatenate([[0], np.cumsum([len(c) for c in cl])]).astype(np.int32)
            xyz = np.ascontiguousarray(np.concatenate(cl + [np.zeros((1, 3), np.float32)]), np.float32)
            q.cloud_offsets, q.cloud_xyz, q.weight = off.ctypes.data, xyz.ctypes.data, float(p.get("weight", 1.0))
            q.Tcl = (C.c_float * 7)(*[float(x) for x in p["Tcl7"]])
            keep.append((off, xyz))
        outs.append(o)
    return arr, outs, keep


def ba_window_solve_batch(problems, inv_level_sigma2, store, cam5, group=0, fill=0):
    """tc2li_ba_window_solve_batch: gather, local BA and outlier rule of the windows in one call, the windows staying on the device in
    between (problems: see pack_ba_window_solve_problems).  -> one dict per problem: result (iterations done, 0 ABORTED, -2 refused), the
    gather's status / counts / pose_row / fixed / point_row / lidar_pose_index / edges (None unless asked for), the OPTIMISED poses7 and
    points3, chi2 and depth_positive (None unless asked for), stats, lidar_stats, erase [n, 2] (pose, point) and n_erase."""
    arr, outs, keep = pack_ba_window_solve_problems(problems, fill)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    cam = np.ascontiguousarray(cam5, np.float64)
    n = len(problems)
    results = np.zeros(max(n, 1), np.int32)
    f = lib().tc2li_ba_window_solve_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    _check(f(store._handle(), C.addressof(arr), n, sg.ctypes.data, len(sg), cam.ctypes.data, int(group), results.ctypes.data))
    res = []
    for i, o in enumerate(outs):
        r, c = _cut_ba_window_outputs(o)
        ne, m = c["n_edges"], int(o["n_erase"][0])
        r.update(result=int(results[i]), chi2=None if o["edge_chi2"] is None else o["edge_chi2"][:ne],
                 depth_positive=None if o["edge_depth_positive"] is None else o["edge_depth_positive"][:ne], stats=o["stats"],
                 lidar_stats=o["lidar_stats"], n_erase=m, erase=np.stack([o["erase_pose"][:m], o["erase_point"][:m]], 1), keep=keep)
        res.append(r)
    return res


MAP_GRAPH_EDIT_DTYPE = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
MAP_GRAPH_OPS = ("ADD_KEYFRAME", "SET_KEYFRAME_FLAGS", "SET_POSE", "ADD_POINT", "SET_POINT_FLAGS", "SET_POSITION", "SET_SLOT", "ADD_OBSERVATION",
                 "ERASE_OBSERVATION", "CLEAR_OBSERVATIONS")
MAP_GRAPH_OP = {k: i for i, k in enumerate(MAP_GRAPH_OPS)}
_MAP_GRAPH_ARRAYS = (("kf_slot", np.int32, 0, 1), ("kf_id", np.int64, 0, 1), ("kf_flags", np.uint8, 0, 1), ("poses7", np.float64, 0, 7),
                     ("slot_offsets", np.int32, 0, 1), ("slot_point", np.int32, 1, 1), ("point_flags", np.uint8, 2, 1), ("positions", np.float64, 2, 3),
                     ("obs_offsets", np.int32, 2, 1), ("obs_kf", np.int32, 3, 1), ("obs_index", np.int32, 3, 1))   # name, type, capacity, width
_MAP_GRAPH_INFO = ("n_keyframes", "n_points", "n_slots", "n_observations", "applies", "apply_bytes", "gather_bytes")


class MapGraphTables(C.Structure):
    """tc2li_map_graph_tables"""
    _fields_ = [(k, C.c_void_p) for k, _, _, _ in _MAP_GRAPH_ARRAYS] + [("n_keyframes", C.c_int32), ("n_points", C.c_int32)]


class MapGraphDelta(C.Structure):
    """tc2li_map_graph_delta"""
    _fields_ = [("edits", C.c_void_p), ("values", C.c_void_p)] + [(k, C.c_int32) for k in ("sequence", "n_edits", "n_values", "pad_")]


def _pack_map_graph_tables(t, into):
    """The tables of one sequence (a dict with the arrays of tc2li_ba_window_problem; further keys are ignored) into a MapGraphTables."""
    a = {k: np.ascontiguousarray(t[k], ty).reshape(-1) for k, ty, _, _ in _MAP_GRAPH_ARRAYS}
    nk, npts = len(a["kf_slot"]), len(a["point_flags"])
    if len(a["kf_id"]) != nk or len(a["kf_flags"]) != nk or len(a["poses7"]) != 7 * nk or len(a["slot_offsets"]) != nk + 1:
        raise ValueError("the keyframe arrays do not have one row per keyframe")
    if len(a["positions"]) != 3 * npts or len(a["obs_offsets"]) != npts + 1:
        raise ValueError("the point arrays do not have one row per point")
    if len(a["slot_point"]) < int(a["slot_offsets"][-1]) or min(len(a["obs_kf"]), len(a["obs_index"])) < int(a["obs_offsets"][-1]):
        raise ValueError("slot or observation arrays are shorter than their offsets say")
    for k, v in a.items():
        setattr(into, k, v.ctypes.data)
    into.n_keyframes, into.n_points = nk, npts
    return a


def _room_for_map_graph_tables(capacities, fill=0):
    """-> (MapGraphTables over fresh arrays with room for `capacities` (keyframes, slots, points, observations), the arrays)"""
    t, a = MapGraphTables(), {}
    for k, ty, c, w in _MAP_GRAPH_ARRAYS:
        a[k] = np.full((int(capacities[c]) + (1 if k.endswith("offsets") else 0)) * w, fill, np.int64).astype(ty)
        setattr(t, k, a[k].ctypes.data)
    return t, a


def _cut_map_graph_tables(a, counts):
    nk, ns, npts, no = [int(c) for c in counts]
    return dict(kf_slot=a["kf_slot"][:nk], kf_id=a["kf_id"][:nk], kf_flags=a["kf_flags"][:nk], poses7=a["poses7"][:7 * nk].reshape(-1, 7),
                slot_offsets=a["slot_offsets"][:nk + 1], slot_point=a["slot_point"][:ns], point_flags=a["point_flags"][:npts],
                positions=a["positions"][:3 * npts].reshape(-1, 3), obs_offsets=a["obs_offsets"][:npts + 1], obs_kf=a["obs_kf"][:no],
                obs_index=a["obs_index"][:no])


def map_graph_limits():
    """tc2li_map_graph_limits -> {lds_row, edits_per_step, threads, apply_record_bytes, gather_record_bytes, max_walk}"""
    out = (C.c_int32 * 6)()
    f = lib().tc2li_map_graph_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 6))
    return dict(zip(("lds_row", "edits_per_step", "threads", "apply_record_bytes", "gather_record_bytes", "max_walk"), [int(v) for v in out]))


def _pack_map_graph_log(edits, values):
    e = np.ascontiguousarray(edits, MAP_GRAPH_EDIT_DTYPE).reshape(-1)
    v = np.ascontiguousarray(values if values is not None else [], np.float64).reshape(-1)
    return e, v


def host_map_graph_apply(tables, edits, values, capacities):
    """tc2li_host_map_graph_apply, the host twin: the log (edits: MAP_GRAPH_EDIT_DTYPE, values: float64) applied one edit after the other to
    the tables (a dict as for ResidentMapGraph.set_batch) -> the tables after it.  capacities: keyframes, slots, points, observations."""
    tin = MapGraphTables()
    keep = _pack_map_graph_tables(tables, tin)
    e, v = _pack_map_graph_log(edits, values)
    caps = np.ascontiguousarray(capacities, np.int32)
    tout, a = _room_for_map_graph_tables(caps)
    counts = np.zeros(4, np.int32)
    f = lib().tc2li_host_map_graph_apply
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(C.addressof(tin), e.ctypes.data, len(e), v.ctypes.data, len(v), C.addressof(tout), caps.ctypes.data, counts.ctypes.data))
    del keep
    return _cut_map_graph_tables(a, counts)


_MAP_GRAPH_CONNECTIONS_ARRAYS = ("conn_offsets", "conn_kf", "conn_weight", "ord_offsets", "ord_kf", "ord_weight")
_MAP_GRAPH_CONNECTIONS_INFO = ("weight_entries", "ordered_entries", "updates", "update_bytes")


class MapGraphConnections(C.Structure):
    """tc2li_map_graph_connections"""
    _fields_ = [(k, C.c_void_p) for k in _MAP_GRAPH_CONNECTIONS_ARRAYS] + [("n_keyframes", C.c_int32), ("pad_", C.c_int32)]


def _pack_map_graph_connections(t, into):
    a = {k: np.ascontiguousarray(t[k], np.int32).reshape(-1) for k in _MAP_GRAPH_CONNECTIONS_ARRAYS}
    nk = len(a["conn_offsets"]) - 1
    if nk < 0 or len(a["ord_offsets"]) != nk + 1:
        raise ValueError("conn_offsets and ord_offsets have one entry per keyframe row and one more")
    if min(len(a["conn_kf"]), len(a["conn_weight"])) < int(a["conn_offsets"][-1]) or min(len(a["ord_kf"]), len(a["ord_weight"])) < int(a["ord_offsets"][-1]):
        raise ValueError("connection arrays are shorter than their offsets say")
    for k, v in a.items():
        setattr(into, k, v.ctypes.data)
    into.n_keyframes = nk
    return a


def _room_for_map_graph_connections(n_keyframes, capacities, fill=0):
    t, a = MapGraphConnections(), {}
    for k in _MAP_GRAPH_CONNECTIONS_ARRAYS:
        n = int(n_keyframes) + 1 if k.endswith("offsets") else int(capacities[0 if k.startswith("conn") else 1])
        a[k] = np.full(n, fill, np.int32)
        setattr(t, k, a[k].ctypes.data)
    return t, a


def _cut_map_graph_connections(a, n_keyframes, sizes):
    nw, no = int(sizes[0]), int(sizes[1])
    return dict(conn_offsets=a["conn_offsets"][:n_keyframes + 1], conn_kf=a["conn_kf"][:nw], conn_weight=a["conn_weight"][:nw],
                ord_offsets=a["ord_offsets"][:n_keyframes + 1], ord_kf=a["ord_kf"][:no], ord_weight=a["ord_weight"][:no])


def map_graph_connections_limits():
    """tc2li_map_graph_connections_limits -> {record_bytes, status_bytes}: what an update or an erase of the resident connections moves per
    sequence, host to device and (beside the counts block) device to host."""
    out = (C.c_int32 * 2)()
    f = lib().tc2li_map_graph_connections_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 2))
    return dict(record_bytes=int(out[0]), status_bytes=int(out[1]))


def _host_map_graph_connections(tables, connections, capacities, call):
    tin, cin = MapGraphTables(), MapGraphConnections()
    keep = (_pack_map_graph_tables(tables, tin), _pack_map_graph_connections(connections, cin))
    nk = int(tin.n_keyframes)
    caps = np.ascontiguousarray(capacities if capacities is not None else
                                [len(keep[1]["conn_kf"]) + 2 * nk + 2, len(keep[1]["ord_kf"]) + len(keep[1]["conn_kf"]) + 2 * nk + 2], np.int32)
    cout, a = _room_for_map_graph_connections(nk, caps)
    sizes = np.zeros(2, np.int32)
    try:
        rc = call(C.addressof(tin), C.addressof(cin), C.addressof(cout), caps.ctypes.data, sizes.ctypes.data)
        _check(rc)
    except Tc2liError as e:
        e.sizes = sizes
        raise
    del keep
    return rc, _cut_map_graph_connections(a, nk, sizes)


def host_map_graph_update_connections(tables, connections, current, first_connection=0, init_kf_id=-1, capacities=None):
    """tc2li_host_map_graph_update_connections, the host twin of ResidentMapGraph.update_connections_batch for one sequence: tables as for
    set_batch, connections as for set_connections_batch (its rows may end before the tables' keyframe rows) -> (counts [8], the
    connections after the call).  capacities: weight and ordered entries of the result; by default what always suffices.  A refusal for
    want of room carries the sizes needed as the exception's ``sizes``."""
    counts = np.zeros(8, np.int32)
    f = lib().tc2li_host_map_graph_update_connections
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _, out = _host_map_graph_connections(tables, connections, capacities, lambda t, ci, co, caps, sizes: f(
        t, ci, int(current), int(bool(first_connection)), int(init_kf_id), co, caps, sizes, counts.ctypes.data))
    return counts, out


def host_map_graph_erase_connections(tables, connections, row, capacities=None):
    """tc2li_host_map_graph_erase_connections, the host twin of ResidentMapGraph.erase_connections_batch -> the connections after it."""
    f = lib().tc2li_host_map_graph_erase_connections
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    return _host_map_graph_connections(tables, connections, capacities, lambda t, ci, co, caps, sizes: f(t, ci, int(row), co, caps, sizes))[1]


class ResidentMapGraph:
    """``tc2li_map_graph_*``: the input half of the local-BA window problems of n_sequences sequences, resident on the device and edited by
    logs.  capacities: per sequence keyframe rows, slot entries, point rows, observation entries.  Bound to one :class:`KeyframeStore`."""

    def __init__(self, store, n_sequences, capacities):
        self._h = C.c_void_p()
        self.store, self.n_sequences = store, int(n_sequences)
        self.capacities = np.ascontiguousarray(capacities, np.int32).copy()
        if self.capacities.shape != (4,):
            raise ValueError("four capacities: keyframes, slots, points, observations")
        f = lib().tc2li_map_graph_create
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(store._handle(), self.n_sequences, self.capacities.ctypes.data, C.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise ValueError("the map graph is closed")
        return self._h

    def set_batch(self, sequences, tables, stream=0):
        """tc2li_map_graph_set_batch: the full state of the named sequences (tables: dicts with the arrays of tc2li_ba_window_problem)."""
        seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
        arr = (MapGraphTables * max(len(tables), 1))()
        keep = [_pack_map_graph_tables(t, arr[i]) for i, t in enumerate(tables)]
        f = lib().tc2li_map_graph_set_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._handle(), seq.ctypes.data, C.addressof(arr), len(tables), C.c_void_p(stream)))
        del keep

    def apply_batch(self, deltas, stream=0):
        """tc2li_map_graph_apply_batch.  deltas: (sequence, edits (MAP_GRAPH_EDIT_DTYPE), values (float64 or None)) per named sequence."""
        arr, keep = (MapGraphDelta * max(len(deltas), 1))(), []
        for i, (s, edits, values) in enumerate(deltas):
            e, v = _pack_map_graph_log(edits, values)
            keep.append((e, v))
            arr[i].edits, arr[i].values, arr[i].sequence, arr[i].n_edits, arr[i].n_values = e.ctypes.data, v.ctypes.data, int(s), len(e), len(v)
        f = lib().tc2li_map_graph_apply_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._handle(), C.addressof(arr), len(deltas), C.c_void_p(stream)))
        del keep

    def download(self, sequence, fill=0):
        """tc2li_map_graph_download -> the resident tables of the sequence as a dict of arrays"""
        i = self.info(sequence)
        caps = np.array([i["n_keyframes"], i["n_slots"], i["n_points"], i["n_observations"]], np.int32)
        t, a = _room_for_map_graph_tables(caps, fill)
        counts = np.zeros(4, np.int32)
        f = lib().tc2li_map_graph_download
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self._handle(), int(sequence), C.addressof(t), caps.ctypes.data, counts.ctypes.data))
        return _cut_map_graph_tables(a, counts)

    def info(self, sequence):
        """tc2li_map_graph_info -> {n_keyframes, n_points, n_slots, n_observations, applies, apply_bytes, gather_bytes}"""
        out = (C.c_int64 * len(_MAP_GRAPH_INFO))()
        f = lib().tc2li_map_graph_info
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _check(f(self._handle(), int(sequence), out, len(_MAP_GRAPH_INFO)))
        return dict(zip(_MAP_GRAPH_INFO, [int(v) for v in out]))

    # ---- the covisibility graph (tc2li_map_graph_connections_*) ----
    def connections_reserve(self, entries_per_sequence):
        """tc2li_map_graph_connections_reserve: once per graph, room for that many entries per sequence in the weight and the ordered CSR."""
        f = lib().tc2li_map_graph_connections_reserve
        f.argtypes = [C.c_void_p, C.c_int]
        _check(f(self._handle(), int(entries_per_sequence)))

    def set_connections_batch(self, sequences, tables, stream=0):
        """tc2li_map_graph_set_connections_batch.  tables: dicts with conn_offsets, conn_kf, conn_weight, ord_offsets, ord_kf, ord_weight."""
        seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
        arr = (MapGraphConnections * max(len(tables), 1))()
        keep = [_pack_map_graph_connections(t, arr[i]) for i, t in enumerate(tables)]
        f = lib().tc2li_map_graph_set_connections_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._handle(), seq.ctypes.data, C.addressof(arr), len(tables), C.c_void_p(stream)))
        del keep

    def download_connections(self, sequence, fill=0):
        """tc2li_map_graph_download_connections -> the resident connections of the sequence as a dict of arrays"""
        i, c = self.info(sequence), self.connections_info(sequence)
        caps = np.array([c["weight_entries"], c["ordered_entries"]], np.int32)
        t, a = _room_for_map_graph_connections(i["n_keyframes"], caps, fill)
        counts = np.zeros(2, np.int32)
        f = lib().tc2li_map_graph_download_connections
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self._handle(), int(sequence), C.addressof(t), caps.ctypes.data, counts.ctypes.data))
        return _cut_map_graph_connections(a, int(t.n_keyframes), counts)

    def connections_info(self, sequence):
        """tc2li_map_graph_connections_info -> {weight_entries, ordered_entries, updates, update_bytes}"""
        out = (C.c_int64 * len(_MAP_GRAPH_CONNECTIONS_INFO))()
        f = lib().tc2li_map_graph_connections_info
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _check(f(self._handle(), int(sequence), out, len(_MAP_GRAPH_CONNECTIONS_INFO)))
        return dict(zip(_MAP_GRAPH_CONNECTIONS_INFO, [int(v) for v in out]))

    def update_connections_batch(self, sequences, current_rows, first_connection, init_kf_id, stream=0, counts_into=None):
        """tc2li_map_graph_update_connections_batch: one KeyFrame::UpdateConnections per named sequence on the resident tables ->
        counts [n, 8] (status, n_counter, n_ordered, n_changed, n_changed_entries, parent, 0, 0).  counts_into: an int32 [n, 8] array that
        receives the blocks also when the call is refused for want of room (entries 6 and 7 are then the sizes needed)."""
        seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
        cur = np.ascontiguousarray(current_rows, np.int32).reshape(-1)
        first = np.ascontiguousarray(first_connection, np.uint8).reshape(-1)
        init = np.ascontiguousarray(init_kf_id, np.int64).reshape(-1)
        if not len(seq) == len(cur) == len(first) == len(init):
            raise ValueError("one current row, first_connection and init_kf_id per sequence")
        counts = np.zeros((max(len(seq), 1), 8), np.int32) if counts_into is None else counts_into
        if counts.dtype != np.int32 or counts.size < 8 * len(seq) or not counts.flags["C_CONTIGUOUS"]:
            raise ValueError("counts_into: a contiguous int32 array of [n, 8]")
        f = lib().tc2li_map_graph_update_connections_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(f(self._handle(), seq.ctypes.data, cur.ctypes.data, first.ctypes.data, init.ctypes.data, len(seq), counts.ctypes.data, C.c_void_p(stream)))
        return counts.reshape(-1, 8)[:len(seq)]

    def erase_connections_batch(self, sequences, rows, stream=0):
        """tc2li_map_graph_erase_connections_batch: what KeyFrame::SetBadFlag does to covisibility, for one keyframe row per named sequence."""
        seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
        row = np.ascontiguousarray(rows, np.int32).reshape(-1)
        if len(seq) != len(row):
            raise ValueError("one row per sequence")
        f = lib().tc2li_map_graph_erase_connections_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(self._handle(), seq.ctypes.data, row.ctypes.data, len(seq), C.c_void_p(stream)))

    def close(self):
        if self._h:
            f = lib().tc2li_map_graph_destroy
            f.argtypes = [C.c_void_p]
            f(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _without_tables(window):
    """A tc2li_ba_window_problem as the graph-reading entries take it: the table pointers NULL and the sizes 0 -- they are not read."""
    for k, _ in _BA_WINDOW_ARRAYS:
        if k != "cov_kf":
            setattr(window, k, None)
    window.n_keyframes = window.n_points = 0


def _without_cov(window):
    """... and as the entries that read the neighbour list from the graph's ordered connections take it: no cov_kf either"""
    window.cov_kf = None
    window.n_cov = 0


def ba_window_graph_cov_batch(problems, sequences, inv_level_sigma2, store, graph, stream=0, raw=False, fill=0, keep_cov=False):
    """tc2li_ba_window_graph_cov_batch: ba_window_graph_batch with the neighbour list of problem i read from the resident ordered row of its
    current keyframe; the problems' cov_kf does not reach the library (keep_cov=True passes it on, to see it refused)."""
    return ba_window_graph_batch(problems, sequences, inv_level_sigma2, store, graph, stream, raw, fill, _cov=1 if keep_cov else 2)


def ba_window_graph_batch(problems, sequences, inv_level_sigma2, store, graph, stream=0, raw=False, fill=0, _cov=0):
    """tc2li_ba_window_graph_batch: ba_window_batch with the tables of problem i taken from sequence sequences[i] of `graph` (a
    :class:`ResidentMapGraph`).  problems: the dicts of ba_window_batch; of them current, cov_kf, init_kf_id and the capacities reach the library (the
    tables only size the default capacities).  -> as ba_window_batch."""
    arr, outs, keep = pack_ba_window_problems(problems, fill)
    for i in range(len(problems)):
        _without_tables(arr[i])
        if _cov == 2:
            _without_cov(arr[i])
    seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
    if len(seq) != len(problems):
        raise ValueError("one sequence per problem")
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    f = lib().tc2li_ba_window_graph_cov_batch if _cov else lib().tc2li_ba_window_graph_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    _check(f(store._handle(), graph._handle(), seq.ctypes.data, C.addressof(arr), len(problems), sg.ctypes.data, len(sg), C.c_void_p(stream)))
    del keep
    if raw:
        return outs
    res = []
    for o in outs:
        r, c = _cut_ba_window_outputs(o)
        r.update({k: c[k] for k in ("status", "num_fixed_kf", "num_opt_kf", "n_lidar", "n_points_without_edge")})
        res.append(r)
    return res


def ba_window_solve_graph_batch(problems, sequences, inv_level_sigma2, store, graph, cam5, group=0, fill=0):
    """tc2li_ba_window_solve_graph_batch: ba_window_solve_batch with the tables of problem i taken from sequence sequences[i] of `graph`.
    -> as ba_window_solve_batch."""
    arr, outs, keep = pack_ba_window_solve_problems(problems, fill)
    for i in range(len(problems)):
        _without_tables(arr[i].window)
    seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
    if len(seq) != len(problems):
        raise ValueError("one sequence per problem")
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    cam = np.ascontiguousarray(cam5, np.float64)
    n = len(problems)
    results = np.zeros(max(n, 1), np.int32)
    f = lib().tc2li_ba_window_solve_graph_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    _check(f(store._handle(), graph._handle(), seq.ctypes.data, C.addressof(arr), n, sg.ctypes.data, len(sg), cam.ctypes.data, int(group), results.ctypes.data))
    res = []
    for i, o in enumerate(outs):
        r, c = _cut_ba_window_outputs(o)
        ne, m = c["n_edges"], int(o["n_erase"][0])
        r.update(result=int(results[i]), chi2=None if o["edge_chi2"] is None else o["edge_chi2"][:ne],
                 depth_positive=None if o["edge_depth_positive"] is None else o["edge_depth_positive"][:ne], stats=o["stats"],
                 lidar_stats=o["lidar_stats"], n_erase=m, erase=np.stack([o["erase_pose"][:m], o["erase_point"][:m]], 1), keep=keep)
        res.append(r)
    return res


BA_COMMIT_POSITIONS_F32 = 1


def ba_window_solve_graph_commit_cov_batch(problems, sequences, inv_level_sigma2, store, graph, cam5, group=0, fill=0, flags=0):
    """tc2li_ba_window_solve_graph_commit_cov_batch: ba_window_solve_graph_commit_batch with the neighbour list of window i read from the
    resident ordered row of its current keyframe; the problems' cov_kf does not reach the library."""
    return ba_window_solve_graph_commit_batch(problems, sequences, inv_level_sigma2, store, graph, cam5, group, fill, flags, _cov=True)


def ba_window_solve_graph_commit_batch(problems, sequences, inv_level_sigma2, store, graph, cam5, group=0, fill=0, flags=0, _cov=False):
    """tc2li_ba_window_solve_graph_commit_batch: ba_window_solve_graph_batch, and every solved window written into its sequence of `graph`
    -- the erase pairs, the free poses and the points, the closing step of LocalLVBundleAdjustment -- without the values leaving the device.
    flags: 0 or BA_COMMIT_POSITIONS_F32.  No sequence twice.  -> as ba_window_solve_batch."""
    arr, outs, keep = pack_ba_window_solve_problems(problems, fill)
    for i in range(len(problems)):
        _without_tables(arr[i].window)
        if _cov:
            _without_cov(arr[i].window)
    seq = np.ascontiguousarray(sequences, np.int32).reshape(-1)
    if len(seq) != len(problems):
        raise ValueError("one sequence per problem")
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    cam = np.ascontiguousarray(cam5, np.float64)
    n = len(problems)
    results = np.zeros(max(n, 1), np.int32)
    f = lib().tc2li_ba_window_solve_graph_commit_cov_batch if _cov else lib().tc2li_ba_window_solve_graph_commit_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    _check(f(store._handle(), graph._handle(), seq.ctypes.data, C.addressof(arr), n, sg.ctypes.data, len(sg), cam.ctypes.data, int(group), int(flags),
             results.ctypes.data))
    res = []
    for i, o in enumerate(outs):
        r, c = _cut_ba_window_outputs(o)
        ne, m = c["n_edges"], int(o["n_erase"][0])
        r.update(result=int(results[i]), chi2=None if o["edge_chi2"] is None else o["edge_chi2"][:ne],
                 depth_positive=None if o["edge_depth_positive"] is None else o["edge_depth_positive"][:ne], stats=o["stats"],
                 lidar_stats=o["lidar_stats"], n_erase=m, erase=np.stack([o["erase_pose"][:m], o["erase_point"][:m]], 1), keep=keep)
        res.append(r)
    return res


def host_ba_window_commit_log(tables, solved, flags=0, edit_capacity=None, value_capacity=None, into=None, sizes=None):
    """tc2li_host_ba_window_commit_log: the closing step of LocalLVBundleAdjustment as an edit log of the map graph.  tables: the sequence's
    tables before the solve; solved: a result of ba_window_solve_batch (result, status, pose_row, fixed, poses7, point_row, points3, erase)
    -- n_erase and erase_capacity, if given, stand for the pairs the rule found and the room the erase lists had.  into: (edits, values)
    arrays to write instead of fresh ones; sizes: an int32 [2] that receives the edits and values of the log, also when the call is
    refused for want of room.  -> (edits as MAP_GRAPH_EDIT_DTYPE, values)."""
    t = MapGraphTables()
    keep = _pack_map_graph_tables(tables, t)
    pose_row = np.ascontiguousarray(solved["pose_row"], np.int32).reshape(-1)
    fixed = np.ascontiguousarray(solved["fixed"], np.uint8).reshape(-1)
    poses7 = np.ascontiguousarray(solved["poses7"], np.float64).reshape(-1)
    point_row = np.ascontiguousarray(solved["point_row"], np.int32).reshape(-1)
    points3 = np.ascontiguousarray(solved["points3"], np.float64).reshape(-1)
    erase = np.asarray(solved["erase"], np.int32).reshape(-1, 2)
    erase_pose, erase_point = np.ascontiguousarray(erase[:, 0]), np.ascontiguousarray(erase[:, 1])
    n_erase = np.array([solved.get("n_erase", len(erase))], np.int32)
    counts = np.zeros(len(_BA_WINDOW_COUNTS), np.int32)
    counts[0], counts[3], counts[4] = int(solved["status"]), len(pose_row), len(point_row)
    q = BaWindowSolveProblem()
    w = q.window
    w.counts, w.pose_row, w.fixed, w.poses7_out, w.point_row, w.points3_out = (counts.ctypes.data, pose_row.ctypes.data, fixed.ctypes.data, poses7.ctypes.data,
                                                                              point_row.ctypes.data, points3.ctypes.data)
    q.erase_pose, q.erase_point, q.n_erase = erase_pose.ctypes.data, erase_point.ctypes.data, n_erase.ctypes.data
    q.erase_capacity = int(solved.get("erase_capacity", len(erase)))
    ne = 2 * len(erase) + len(pose_row) + len(point_row) if edit_capacity is None else int(edit_capacity)
    nv = 7 * len(pose_row) + 3 * len(point_row) if value_capacity is None else int(value_capacity)
    edits, values = (np.zeros(max(ne, 1), MAP_GRAPH_EDIT_DTYPE), np.zeros(max(nv, 1), np.float64)) if into is None else into
    if len(edits) < ne or len(values) < nv or edits.dtype != MAP_GRAPH_EDIT_DTYPE or values.dtype != np.float64:
        raise ValueError("into: arrays of MAP_GRAPH_EDIT_DTYPE and float64 with the stated room")
    sizes = np.zeros(2, np.int32) if sizes is None else sizes
    f = lib().tc2li_host_ba_window_commit_log
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    n = _check(f(C.addressof(t), C.addressof(q), int(solved["result"]), int(flags), edits.ctypes.data, ne, values.ctypes.data, nv, sizes.ctypes.data,
                 sizes.ctypes.data + 4))
    del keep
    return edits[:n], values[:int(sizes[1])]


class InertialWindowProblem(C.Structure):
    """tc2li_inertial_window_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("kf_slot", "kf_id", "kf_flags", "prev_kf", "states", "slot_offsets", "slot_point", "point_flags", "positions",
                                          "obs_offsets", "obs_kf", "obs_index", "counts", "kf_row", "keyframes_out", "fixed", "has_imu", "point_row",
                                          "points3_out", "edges", "links", "link_kf2_row", "lidar_pose_index")] \
        + [(k, C.c_int32) for k in ("n_keyframes", "n_points", "current", "keyframes_in_map", "large", "rec_init", "with_lidar", "kf_capacity",
                                    "point_capacity", "edge_capacity", "link_capacity", "pad_")]


INERTIAL_WINDOW_OK, INERTIAL_WINDOW_EMPTY, INERTIAL_WINDOW_MAX_LIDAR, INERTIAL_WINDOW_MAX_OPT = 0, 1, 6, 25
INERTIAL_LINK_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("robust", "<i4"), ("pad_", "<i4"), ("info_scale", "<f8"), ("preintegrated", "<u8")])
_INERTIAL_WINDOW_ARRAYS = (("kf_slot", np.int32), ("kf_id", np.int64), ("kf_flags", np.uint8), ("prev_kf", np.int32), ("states", np.float64),
                           ("slot_offsets", np.int32), ("slot_point", np.int32), ("point_flags", np.uint8), ("positions", np.float64),
                           ("obs_offsets", np.int32), ("obs_kf", np.int32), ("obs_index", np.int32))
_INERTIAL_WINDOW_COUNTS = ("status", "n_fixed_kf", "n_opt_kf", "n_vertices", "n_points", "n_edges", "n_links", "n_lidar", "n_points_without_edge",
                           "n_vertices_under_3_edges")


def inertial_window_limits():
    """tc2li_inertial_window_limits -> {lds_keyframes, lds_points, threads}: the sizes at which the device path of inertial_window_batch
    changes (the keyframe marks leave LDS above lds_keyframes keyframes, the first-occurrence keys above lds_points points)."""
    out = (C.c_int32 * 3)()
    f = lib().tc2li_inertial_window_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 3))
    return dict(zip(("lds_keyframes", "lds_points", "threads"), [int(v) for v in out]))


def pack_inertial_window_problems(problems, fill=0):
    """The tc2li_inertial_window_problem array of a batch with its output arrays (prefilled with `fill`) -> (array, outputs per problem, what
    must stay alive).  Capacities: kf_capacity / point_capacity / edge_capacity / link_capacity of the problem's dict, by default what can
    never be too small (the keyframes, the points, the observations, 25)."""
    arr, outs, keep = (InertialWindowProblem * max(len(problems), 1))(), [], []
    for i, p in enumerate(problems):
        a = {k: np.ascontiguousarray(p[k], t).reshape(-1) for k, t in _INERTIAL_WINDOW_ARRAYS}
        nk, npts = len(a["kf_slot"]), len(a["point_flags"])
        if len(a["kf_id"]) != nk or len(a["kf_flags"]) != nk or len(a["prev_kf"]) != nk or len(a["states"]) != 33 * nk or len(a["slot_offsets"]) != nk + 1:
            raise ValueError("problem %d: the keyframe arrays do not have one row per keyframe" % i)
        if len(a["positions"]) != 3 * npts or len(a["obs_offsets"]) != npts + 1:
            raise ValueError("problem %d: the point arrays do not have one row per point" % i)
        ns, no = int(a["slot_offsets"][-1]), int(a["obs_offsets"][-1])
        if len(a["slot_point"]) < ns or min(len(a["obs_kf"]), len(a["obs_index"])) < no:
            raise ValueError("problem %d: slot or observation arrays are shorter than their offsets say" % i)
        kc, tc, ec, lc = (int(p.get(k, d)) for k, d in (("kf_capacity", nk), ("point_capacity", npts), ("edge_capacity", no),
                                                        ("link_capacity", INERTIAL_WINDOW_MAX_OPT)))
        full = lambda n, t: np.full(max(n, 0), fill, np.int64).astype(t)
        edges, links = np.zeros(max(ec, 0), BA_EDGE_DTYPE), np.zeros(max(lc, 0), INERTIAL_LINK_DTYPE)
        edges.view(np.uint8)[:] = fill & 0xff
        links.view(np.uint8)[:] = fill & 0xff
        o = dict(counts=full(len(_INERTIAL_WINDOW_COUNTS), np.int32), kf_row=full(kc, np.int32), keyframes_out=full(33 * kc, np.float64),
                 fixed=full(kc, np.uint8), has_imu=full(kc, np.uint8), point_row=full(tc, np.int32), points3_out=full(3 * tc, np.float64), edges=edges,
                 links=links, link_kf2_row=full(lc, np.int32), lidar_pose_index=full(INERTIAL_WINDOW_MAX_LIDAR, np.int32))
        for k, v in list(a.items()) + list(o.items()):
            setattr(arr[i], k, v.ctypes.data)
        arr[i].n_keyframes, arr[i].n_points, arr[i].current, arr[i].keyframes_in_map = nk, npts, int(p["current"]), int(p["keyframes_in_map"])
        arr[i].large, arr[i].rec_init, arr[i].with_lidar = int(bool(p.get("large", 0))), int(bool(p.get("rec_init", 0))), int(bool(p.get("with_lidar", 0)))
        arr[i].kf_capacity, arr[i].point_capacity, arr[i].edge_capacity, arr[i].link_capacity = kc, tc, ec, lc
        keep.append(a)
        outs.append(o)
    return arr, outs, keep


def inertial_window_batch(problems, inv_level_sigma2, store=None, views=None, stream=0, raw=False, fill=0):
    """The gather of ``OptimizerWithLidar::LocalLVIBA`` / ``Optimizer::LocalInertialBA`` (the window of the inertial local BA), one per
    problem.  problems: dicts with the arrays of tc2li_inertial_window_problem (kf_slot, kf_id, kf_flags, prev_kf, states [n, 33],
    slot_offsets, slot_point, point_flags, positions, obs_offsets, obs_kf, obs_index), current, keyframes_in_map and optionally large,
    rec_init, with_lidar and the four capacities.  store: a :class:`KeyframeStore` -- the device entry; views: per slot None or a dict with
    keys and u_right -- the host entry.  -> one dict per problem: status, n_fixed_kf, n_opt_kf, n_lidar, n_points_without_edge,
    n_vertices_under_3_edges, kf_row, kf33 [n, 33], fixed, has_imu, point_row, points3 [n, 3], edges (BA_EDGE_DTYPE), link4 [n, 4] = kf1,
    kf2, robust, info_scale as local_inertial_bundle_adjustment takes them, link_kf2_row, lidar_pose_index [n_lidar], cut to their counts.
    raw=True: the arrays at their full capacity as the library left them (prefilled with `fill`) and counts."""
    if (store is None) == (views is None):
        raise ValueError("either a store (the device entry) or views (the host entry)")
    arr, outs, keep = pack_inertial_window_problems(problems, fill)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    if views is not None:
        varr, vkeep = _pack_ba_window_views(views)
        f = lib().tc2li_host_inertial_window_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _check(f(C.addressof(varr), len(views), C.addressof(arr), len(problems), sg.ctypes.data, len(sg)))
        del vkeep
    else:
        f = lib().tc2li_inertial_window_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _check(f(store._handle(), C.addressof(arr), len(problems), sg.ctypes.data, len(sg), C.c_void_p(stream)))
    del keep
    if raw:
        return outs
    res = []
    for o in outs:
        c = dict(zip(_INERTIAL_WINDOW_COUNTS, [int(v) for v in o["counts"]]))
        r = {k: c[k] for k in ("status", "n_fixed_kf", "n_opt_kf", "n_lidar", "n_points_without_edge", "n_vertices_under_3_edges")}
        nv, nl = c["n_vertices"], c["n_links"]
        lk = o["links"][:nl]
        r.update(kf_row=o["kf_row"][:nv], kf33=o["keyframes_out"].reshape(-1, 33)[:nv], fixed=o["fixed"][:nv], has_imu=o["has_imu"][:nv],
                 point_row=o["point_row"][:c["n_points"]], points3=o["points3_out"].reshape(-1, 3)[:c["n_points"]], edges=o["edges"][:c["n_edges"]],
                 link4=np.stack([lk["kf1"], lk["kf2"], lk["robust"], lk["info_scale"]], 1).astype(np.float64).reshape(-1, 4),
                 link_null=bool((lk["preintegrated"] == 0).all() and (lk["pad_"] == 0).all()), link_kf2_row=o["link_kf2_row"][:nl],
                 lidar_pose_index=o["lidar_pose_index"][:c["n_lidar"]])
        res.append(r)
    return res


def inertial_window_outliers(edges, edge_chi2, edge_depth_positive, point_bad_now, track_depth, initial_chi2, final_chi2, large=False,
                             capacity=None):
    """tc2li_inertial_window_outliers: -> (vToErase of the inertial local BA as (pose index, point index) pairs [n, 2] in the reference's
    order, rejected).  rejected: the test of ``FAIL LOCAL-INERTIAL BA`` on float(initial_chi2) / float(final_chi2) and large; then no pairs.
    Monocular edges go by 5.991f, or 1.5f * 5.991f for points with track_depth < 10, or a negative depth; stereo edges by 7.815f alone."""
    e = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    chi2, dpos = np.ascontiguousarray(edge_chi2, np.float64).reshape(-1), np.ascontiguousarray(edge_depth_positive, np.uint8).reshape(-1)
    bad, depth = np.ascontiguousarray(point_bad_now, np.uint8).reshape(-1), np.ascontiguousarray(track_depth, np.float32).reshape(-1)
    if min(len(chi2), len(dpos)) < len(e):
        raise ValueError("one chi2 and one depth flag per edge")
    if len(depth) != len(bad):
        raise ValueError("one track_depth per point")
    cap = len(e) if capacity is None else int(capacity)
    pose, point = np.full(max(cap, 0), -1, np.int32), np.full(max(cap, 0), -1, np.int32)
    rejected = C.c_int32(0)
    f = lib().tc2li_inertial_window_outliers
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_int]
    n = _check(f(e.ctypes.data, chi2.ctypes.data, dpos.ctypes.data, len(e), bad.ctypes.data, depth.ctypes.data, len(bad), float(initial_chi2),
                 float(final_chi2), int(bool(large)), C.addressof(rejected), pose.ctypes.data, point.ctypes.data, cap))
    return np.stack([pose[:n], point[:n]], 1), bool(rejected.value)


# ---- image ingest: clone / remap / resize and colour to gray (System::TrackStereoLidar, Tracking::GrabImageStereoLidar) ------------------
IMAGE_PREP_COPY, IMAGE_PREP_RECTIFY, IMAGE_PREP_RESIZE = 0, 1, 2


class ImagePrepParams(C.Structure):
    """tc2li_image_prep_params"""
    _fields_ = [(k, C.c_int32) for k in ("src_width", "src_height", "channels", "rgb", "mode", "dst_width", "dst_height")]


def image_prep_params(src_width, src_height, channels=1, rgb=True, mode=IMAGE_PREP_COPY, dst_width=None, dst_height=None):
    """dst_width / dst_height: the maps' size (RECTIFY) or newImSize (RESIZE); the source's size by default."""
    return ImagePrepParams(int(src_width), int(src_height), int(channels), int(bool(rgb)), int(mode),
                           int(src_width if dst_width is None else dst_width), int(src_height if dst_height is None else dst_height))


def _image_prep_maps(params, maps):
    """(xl, yl, xr, yr) -> (the float* [4] the ABI takes, what must stay alive)"""
    arr = (C.c_void_p * 4)()
    keep = []
    for i, m in enumerate(maps or ()):
        if m is None:
            continue
        m = np.ascontiguousarray(m, np.float32)
        if m.shape != (params.dst_height, params.dst_width):
            raise ValueError("map %d is %s, the destination is %d x %d" % (i, m.shape, params.dst_height, params.dst_width))
        keep.append(m)
        arr[i] = m.ctypes.data
    return arr, keep


class ImagePrep:
    """tc2li_image_prep: the image ingest on the device.  One handle per image format and mode."""

    def __init__(self, src_width, src_height, channels=1, rgb=True, mode=IMAGE_PREP_COPY, dst_width=None, dst_height=None, max_images=2):
        self.params = image_prep_params(src_width, src_height, channels, rgb, mode, dst_width, dst_height)
        self._h = C.c_void_p()
        f = lib().tc2li_image_prep_create
        f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        _check(f(C.addressof(self.params), int(max_images), C.byref(self._h)))
        self.max_images = int(max_images)

    def close(self):
        if getattr(self, "_h", None):
            f = lib().tc2li_image_prep_destroy
            f.argtypes, f.restype = [C.c_void_p], None
            f(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_maps(self, camera, map_x, map_y, stream=0):
        """The CV_32F maps (M1, M2) of camera 0 (left) or 1 (right): checked and converted to fixed point once."""
        mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        shape = (self.params.dst_height, self.params.dst_width)
        if mx.shape != shape or my.shape != shape:
            raise ValueError("maps are %s and %s, the destination is %s" % (mx.shape, my.shape, shape))
        f = lib().tc2li_image_prep_set_maps
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self._h, int(camera), mx.ctypes.data, my.ctypes.data, C.c_void_p(stream)))

    def batch_ptr(self, images_ptr, images_on_device, n_images, stride, image_pitch, gray_ptr, gray_stride, gray_pitch, stream=0):
        """tc2li_image_prep_batch on plain addresses; gray_ptr is device memory in the layout OrbExtractor.extract_batch_dev reads."""
        f = lib().tc2li_image_prep_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        return _check(f(self._h, C.c_void_p(images_ptr), int(bool(images_on_device)), int(n_images), int(stride), int(image_pitch),
                        C.c_void_p(gray_ptr), int(gray_stride), int(gray_pitch), C.c_void_p(stream)))


def host_image_prep_batch_ptr(params, maps, images_ptr, n_images, stride, image_pitch, gray_ptr, gray_stride, gray_pitch):
    """tc2li_host_image_prep_batch on plain host addresses; maps = (xl, yl, xr, yr) arrays or None."""
    arr, keep = _image_prep_maps(params, maps)
    f = lib().tc2li_host_image_prep_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t]
    rc = _check(f(C.addressof(params), C.addressof(arr) if maps is not None else None, C.c_void_p(images_ptr), int(n_images), int(stride),
                  int(image_pitch), C.c_void_p(gray_ptr), int(gray_stride), int(gray_pitch)))
    del keep
    return rc


def image_prep_batch(prep, images, maps=None, host=False, out=None, stream=0):
    """The images of a step through the ingest; image i belongs to camera i & 1.
    images: a uint8 array [n, h, w] or [n, h, w, channels] (host memory), or -- host=False only -- a torch uint8 tensor of that shape on
    the device.
    host=False: prep is an :class:`ImagePrep` (RECTIFY: after set_maps of both cameras); the gray images go to ``out``, a contiguous torch
    uint8 device tensor [n, dst_height, dst_width] (made when None), which is returned: hand ``out.data_ptr()`` to
    ``OrbExtractor.extract_batch_dev`` and keep the tensor alive as long as the extractor's pyramids are read.
    host=True: prep is an :class:`ImagePrep` or an ImagePrepParams, maps = (xl, yl, xr, yr) for RECTIFY -> numpy [n, dst_height, dst_width]."""
    p = prep.params if isinstance(prep, ImagePrep) else prep
    n = int(images.shape[0])
    want = (n, p.src_height, p.src_width) + ((p.channels,) if p.channels != 1 or len(images.shape) == 4 else ())
    if tuple(images.shape) != want:
        raise ValueError("images are %s, expected %s" % (tuple(images.shape), want))
    row, one = p.src_width * p.channels, p.src_width * p.channels * p.src_height
    if host:
        img = np.ascontiguousarray(images, np.uint8)
        gray = np.empty((n, p.dst_height, p.dst_width), np.uint8)
        host_image_prep_batch_ptr(p, maps, img.ctypes.data, n, row, one, gray.ctypes.data, p.dst_width, p.dst_width * p.dst_height)
        return gray
    import torch
    if out is None:
        out = torch.empty((n, p.dst_height, p.dst_width), dtype=torch.uint8, device="cuda")
    if tuple(out.shape) != (n, p.dst_height, p.dst_width) or out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device tensor [%d, %d, %d]" % (n, p.dst_height, p.dst_width))
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or not images.is_contiguous() or not images.is_cuda:
            raise ValueError("a torch image batch must be a contiguous uint8 device tensor")
        ptr, on_device = images.data_ptr(), True
    else:
        images = np.ascontiguousarray(images, np.uint8)
        ptr, on_device = images.ctypes.data, False
    prep.batch_ptr(ptr, on_device, n, row, one, out.data_ptr(), p.dst_width, p.dst_width * p.dst_height, stream=stream)
    return out


class InertialTermProblem(C.Structure):
    """tc2li_inertial_term_problem"""
    _fields_ = [(k, C.c_void_p) for k in ("keyframes", "fixed", "has_imu", "links")] + [("n_keyframes", C.c_int32), ("n_links", C.c_int32)] \
        + [(k, C.c_void_p) for k in ("chi2", "H_diag", "H_link", "b")]


def inertial_term_limits():
    """tc2li_inertial_term_limits -> {max_keyframes, max_links}: the largest window inertial_term_batch takes."""
    out = (C.c_int32 * 2)()
    f = lib().tc2li_inertial_term_limits
    f.argtypes = [C.c_void_p, C.c_int]
    _check(f(out, 2))
    return dict(zip(("max_keyframes", "max_links"), [int(v) for v in out]))


def pack_inertial_term_problems(problems, linearize=True, out=None):
    """The tc2li_inertial_term_problem array of a batch -> (array, the four output arrays per problem, what must stay alive); the arguments
    are those of :func:`inertial_term_batch`."""
    n = len(problems)
    arr, keep, res = (InertialTermProblem * max(n, 1))(), [], []
    for i, p in enumerate(problems):
        kf = np.ascontiguousarray(p["kf33"], np.float64).reshape(-1, 33)
        fixed, has_imu = np.ascontiguousarray(p["fixed"], np.uint8), np.ascontiguousarray(p["has_imu"], np.uint8)
        link4 = np.ascontiguousarray(p["link4"], np.float64).reshape(-1, 4)
        K, L = len(kf), len(link4)
        if len(fixed) != K or len(has_imu) != K or len(p["pre"]) != L:
            raise ValueError("problem %d: fixed / has_imu need one entry per keyframe, pre one per link" % i)
        links = (InertialLink * max(L, 1))()
        for l, row in enumerate(link4):
            pre = p["pre"][l]
            links[l] = InertialLink(int(row[0]), int(row[1]), int(row[2] != 0), 0, float(row[3]), C.addressof(pre.p) if pre is not None else None)
        if out is not None:
            o = [np.ascontiguousarray(a, np.float64) for a in out[i]]
            if any(o[j] is not out[i][j] for j in range(4)) or [a.size for a in o] != [1, K * 225, L * 225, K * 15]:
                raise ValueError("problem %d: out needs contiguous float64 arrays of 1, K * 225, L * 225 and K * 15 entries" % i)
        elif linearize:
            o = [np.zeros(1), np.zeros((K, 15, 15)), np.zeros((L, 15, 15)), np.zeros((K, 15))]
        else:
            o = [np.zeros(1), None, None, None]
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        arr[i] = InertialTermProblem(ptr(kf), ptr(fixed), ptr(has_imu), C.addressof(links) if L else None, K, L, o[0].ctypes.data, ptr(o[1]), ptr(o[2]), ptr(o[3]))
        keep.append((kf, fixed, has_imu, links, p["pre"]))
        res.append(o)
    return arr, res, keep


def inertial_term_batch(problems, linearize=True, host=False, out=None, stream=0):
    """``tc2li_inertial_term_batch`` (host=True: ``tc2li_host_inertial_term_batch``): the inertial term of many local-BA windows at given
    states.  problems: dicts in the form of ``synthetic.inertial_window`` -- kf33 [K, 33], fixed [K], has_imu [K], link4 [L, 4] = kf1, kf2,
    robust, info_scale -- with pre: one ``Preintegrated`` per link (None: a NULL pointer).
    -> per window (chi2, H_diag [K, 15, 15], H_link [L, 15, 15], b [K, 15]); with linearize=False the three arrays are None and NULL is
    passed for them.  out: per window the four arrays to write into (tests: prefilled with a sentinel), passed whatever linearize is."""
    n = len(problems)
    arr, res, keep = pack_inertial_term_problems(problems, linearize, out)
    if host:
        f = lib().tc2li_host_inertial_term_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _check(f(C.addressof(arr), n, int(bool(linearize))))
    else:
        f = lib().tc2li_inertial_term_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _check(f(C.addressof(arr), n, int(bool(linearize)), C.c_void_p(stream)))
    return [(float(o[0].reshape(-1)[0]), o[1], o[2], o[3]) for o in res]
