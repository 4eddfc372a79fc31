"""ctypes binding of libbf_accel.so (include/bf_accel.h) -- plumbing for tests and bench.py.

The product is the C-ABI library and the C++ host code on top of it
(better_flow_amd/host/); this module only lets Python drive the same entry points.
There is no CPU path here: if the library is missing, or no HIP device is present,
construction raises.
"""
import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BF_ACCEL_LIB") or os.path.join(_DIR, "libbf_accel.so")
# The test build (`make -C better_flow_amd/csrc debug`): the same objects plus the BF_DEBUG_* environment hooks the release
# library does not contain.  Only tests load it (tests/helpers.py), by passing lib=DEBUG_LIB_PATH.
DEBUG_LIB_PATH = os.path.join(_DIR, "debug", "libbf_accel.so")

BF_OK, BF_SKIPPED = 0, 1
BF_ERR_ARG, BF_ERR_HIP, BF_ERR_STATE, BF_ERR_NOCONV, BF_ERR_NODEVICE, BF_ERR_CAPACITY = (
    -1, -2, -3, -4, -5, -6)


class Model(C.Structure):
    """bf_model == ObjectModel (object_model.h:10-13)."""
    _fields_ = [
        ("cx", C.c_double), ("cy", C.c_double), ("dx", C.c_double), ("dy", C.c_double),
        ("rot", C.c_double), ("div", C.c_double), ("cnt", C.c_uint32), ("_pad", C.c_uint32),
        ("total_dx", C.c_double), ("total_dy", C.c_double),
        ("total_rot", C.c_double), ("total_div", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "_pad"}


class Window(C.Structure):
    _fields_ = [
        ("scale", C.c_int32),
        ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_max", C.c_int32), ("y_max", C.c_int32),
        ("metric_wsizex", C.c_int32), ("metric_wsizey", C.c_int32),
        ("scale_img_x", C.c_int32), ("scale_img_y", C.c_int32), ("_pad", C.c_int32),
        ("x_shift", C.c_double), ("y_shift", C.c_double),
    ]


class RunOpts(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32), ("min_events", C.c_int32), ("res_x", C.c_int32),
        ("res_y", C.c_int32), ("hard_iter_cap", C.c_int32), ("poll_interval", C.c_int32),
        ("trace_cap", C.c_int32), ("want_uv", C.c_int32),
    ]


class RunInfo(C.Structure):
    _fields_ = [
        ("rc", C.c_int32), ("iterations", C.c_int32),
        ("x_divider", C.c_float), ("y_divider", C.c_float),
        ("rot_divider", C.c_float), ("div_divider", C.c_float),
        ("launches", C.c_int32), ("polls", C.c_int32),
        ("rebins", C.c_int32), ("overflow_events", C.c_int32),
    ]


class TileOpts(C.Structure):
    _fields_ = [
        ("grid_rows", C.c_int32), ("grid_cols", C.c_int32), ("scale", C.c_int32),
        ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32),
        ("guard_res_x", C.c_int32), ("guard_res_y", C.c_int32),
        ("min_events", C.c_int32), ("max_iter", C.c_int32), ("hard_iter_cap", C.c_int32),
    ]


class TraceRec(C.Structure):
    _fields_ = [
        ("model", Model),
        ("x_divider", C.c_float), ("y_divider", C.c_float),
        ("rot_divider", C.c_float), ("div_divider", C.c_float),
        ("iteration", C.c_int32), ("_pad", C.c_int32),
    ]


class Profile(C.Structure):
    _fields_ = [
        ("warp_scatter_ms", C.c_double), ("warp_scatter_launches", C.c_uint64),
        ("stencil_ms", C.c_double), ("stencil_launches", C.c_uint64),
        ("update_ms", C.c_double), ("update_launches", C.c_uint64),
        ("other_ms", C.c_double), ("other_launches", C.c_uint64),
        ("warp_scatter_events", C.c_uint64),
    ]


class LocalWindow(C.Structure):
    _fields_ = [
        ("scale", C.c_int32), ("metric_wsizex", C.c_int32), ("metric_wsizey", C.c_int32),
        ("scale_img_x", C.c_int32), ("scale_img_y", C.c_int32),
        ("c_fr_x", C.c_int32), ("c_fr_y", C.c_int32), ("_pad", C.c_int32), ("c_t", C.c_int64),
    ]


class LocalState(C.Structure):
    _fields_ = [
        ("nx", C.c_double), ("ny", C.c_double), ("last_score", C.c_double),
        ("dnx", C.c_double), ("dny", C.c_double), ("dn_th", C.c_double), ("evaluations", C.c_int64),
    ]


class LocalTileOpts(C.Structure):
    _fields_ = [
        ("grid_rows", C.c_int32), ("grid_cols", C.c_int32), ("scale", C.c_int32), ("wsz", C.c_int32),
        ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32), ("guard_res_x", C.c_int32), ("guard_res_y", C.c_int32),
        ("max_evaluations", C.c_int64),
    ]


class GlobalWindow(C.Structure):
    _fields_ = [
        ("scale", C.c_int32), ("metric_wsize", C.c_int32),
        ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_max", C.c_int32), ("y_max", C.c_int32),
        ("scale_img_x", C.c_int32), ("scale_img_y", C.c_int32),
        ("scale_bordered_img_x", C.c_int32), ("scale_bordered_img_y", C.c_int32),
    ]


class GlobalSearchOpts(C.Structure):
    _fields_ = [
        ("x_low", C.c_double), ("x_hi", C.c_double), ("x_step", C.c_double),
        ("y_low", C.c_double), ("y_hi", C.c_double), ("y_step", C.c_double), ("nz", C.c_double),
    ]


class GlobalResult(C.Structure):
    _fields_ = [
        ("best_nx", C.c_double), ("best_ny", C.c_double), ("best_sum", C.c_int64),
        ("n_x", C.c_int64), ("n_y", C.c_int64),
    ]


class GlobalCells(C.Structure):
    _fields_ = [("n_cell_x", C.c_int32), ("n_cell_y", C.c_int32)]


class GlobalCellResult(C.Structure):
    _fields_ = [
        ("best_nx", C.c_double), ("best_ny", C.c_double), ("best_u", C.c_double), ("best_v", C.c_double),
        ("best_sum", C.c_int64), ("best_index", C.c_int64), ("events", C.c_int64),
    ]


class GlobalPyramidOpts(C.Structure):
    _fields_ = [("levels", C.c_int32), ("factor", C.c_int32), ("radius", C.c_int32)]


class GlobalPyramidInfo(C.Structure):
    _fields_ = [
        ("n_x", C.c_int64), ("n_y", C.c_int64), ("evaluated", C.c_int64), ("level_count", C.c_int64 * 8),
        ("levels_run", C.c_int32), ("reserved", C.c_int32),
    ]


class SegmentOpts(C.Structure):
    _fields_ = [("above_s", C.c_double), ("below_s", C.c_double), ("min_count", C.c_int32), ("connectivity", C.c_int32),
                ("min_pixels", C.c_int32), ("reserved", C.c_int32)]


class SegmentInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("n1", C.c_int64), ("q_sum", C.c_int64), ("q_mean", C.c_int64),
                ("foreground_pixels", C.c_int32), ("components_found", C.c_int32), ("components", C.c_int32),
                ("reserved", C.c_int32)]


class Component(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_pixel", C.c_int32), ("pixels", C.c_int32), ("events", C.c_int32),
                ("row_min", C.c_int32), ("row_max", C.c_int32), ("col_min", C.c_int32), ("col_max", C.c_int32),
                ("row_sum", C.c_int64), ("col_sum", C.c_int64), ("q_sum", C.c_int64)]


class GroupOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32),
                ("guard_res_x", C.c_int32), ("guard_res_y", C.c_int32), ("min_events", C.c_int32),
                ("max_iter", C.c_int32), ("hard_iter_cap", C.c_int32)]


class GroupInfo(C.Structure):
    _fields_ = [("events", C.c_int32), ("row_min", C.c_int32), ("row_max", C.c_int32), ("col_min", C.c_int32),
                ("col_max", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32)]


class AssignOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32), ("margin", C.c_int32),
                ("min_score", C.c_int32), ("use_prior", C.c_int32), ("install", C.c_int32), ("reserved", C.c_int32)]


class AssignInfo(C.Structure):
    _fields_ = [("models", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("assigned", C.c_int32),
                ("unassigned", C.c_int32), ("changed", C.c_int32), ("max_score", C.c_int32), ("reserved", C.c_int32)]


class ProjectOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32), ("margin", C.c_int32),
                ("gain", C.c_int32), ("reserved", C.c_int32 * 3)]


class GroupScore(C.Structure):
    _fields_ = [("events", C.c_int32), ("inside", C.c_int32), ("pixels_hit", C.c_int32), ("pixels_owned", C.c_int32),
                ("max", C.c_int32), ("reserved", C.c_int32), ("sum_sq", C.c_uint64)]


class ProjectInfo(C.Structure):
    _fields_ = [("models", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("unassigned", C.c_int32),
                ("outside", C.c_int32), ("pixels", C.c_int32), ("sum", C.c_uint64), ("sum_sq", C.c_uint64),
                ("reserved", C.c_int32 * 2)]


class MergeOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32), ("margin", C.c_int32),
                ("targets_per_pass", C.c_int32), ("reserved", C.c_int32 * 3)]


class MergeInfo(C.Structure):
    _fields_ = [("models", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("unassigned", C.c_int32),
                ("passes", C.c_int32), ("reserved0", C.c_int32), ("sum", C.c_uint64), ("sum_sq", C.c_uint64),
                ("reserved", C.c_int32 * 2)]


class TrackOpts(C.Structure):
    _fields_ = [("scale", C.c_int32), ("sensor_res_x", C.c_int32), ("sensor_res_y", C.c_int32), ("margin", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class TrackInfo(C.Structure):
    _fields_ = [("models", C.c_int32), ("kept_models", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("unassigned", C.c_int32), ("outside", C.c_int32), ("reserved", C.c_int32 * 2)]


# BF_PROJECT_PALETTE of include/bf_accel.h: the (B, G, R) of group k is PROJECT_PALETTE[k % 12]
PROJECT_PALETTE = ((255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (255, 255, 0),
                   (0, 128, 255), (255, 128, 0), (128, 0, 255), (0, 255, 128), (128, 128, 255))


class AccelProposeOpts(C.Structure):
    _fields_ = [("radius", C.c_int32), ("suppress", C.c_int32), ("max_models", C.c_int32), ("min_votes", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class Proposal(C.Structure):
    _fields_ = [("nx", C.c_double), ("ny", C.c_double), ("u", C.c_double), ("v", C.c_double), ("index", C.c_int64),
                ("votes", C.c_int32), ("peak", C.c_int32)]


class ProposeInfo(C.Structure):
    _fields_ = [("n_x", C.c_int64), ("n_y", C.c_int64), ("voted", C.c_int32), ("unscored", C.c_int32),
                ("off_lattice", C.c_int32), ("proposals", C.c_int32)]


# the numpy view of a bf_component table
COMPONENT_DTYPE = np.dtype([(n, np.int32) for n in ("id", "first_pixel", "pixels", "events", "row_min", "row_max", "col_min",
                                                    "col_max")] + [(n, np.int64) for n in ("row_sum", "col_sum", "q_sum")])

# every symbol include/bf_accel.h declares
EXPORTS = [
    "bf_device_count", "bf_create", "bf_destroy", "bf_last_error", "bf_version",
    "bf_run_opts_default", "bf_abi_struct_sizes", "bf_set_option", "bf_get_stat", "bf_upload_events", "bf_upload_events_device",
    "bf_set_cloud", "bf_project_4param", "bf_project_4param_reinit", "bf_get_time_img", "bf_sobel", "bf_fast_model",
    "bf_writeout_events", "bf_compute_uv", "bf_set_model", "bf_run", "bf_run_many", "bf_run_tiles", "bf_run_tiles_many", "bf_get_trace",
    "bf_profile_enable", "bf_profile_reset", "bf_profile_get", "bf_synchronize",
    "bf_copy_bandwidth", "bf_device_malloc", "bf_device_free", "bf_memcpy_h2d",
    "bf_host_alloc", "bf_host_free", "bf_upload_events_async", "bf_commit_upload",
    "bf_local_set_window", "bf_local_iteration_step", "bf_local_run", "bf_local_run_tiles",
    "bf_upload_ring_async", "bf_upload_ring16_async", "bf_upload_ring16t32_async", "bf_upload_events16_async", "bf_compute_uv_ring", "bf_wait_uploads", "bf_projection_img",
    "bf_color_time_img", "bf_eval_sincos", "bf_device_numa_node", "bf_bind_thread_to_numa_node", "bf_bind_thread_to_device_numa",
    "bf_global_search_opts_default", "bf_global_set_window", "bf_global_project_all", "bf_global_search", "bf_global_get_events",
    "bf_global_set_cells", "bf_global_search_cells", "bf_global_search_cells_pyramid", "bf_global_project_cells",
    "bf_global_project_field",
    "bf_emit_create", "bf_emit_destroy", "bf_emit_reset", "bf_emit_output", "bf_emit_slice", "bf_emit_wait", "bf_emit_release",
    "bf_frame_create", "bf_frame_destroy", "bf_frame_render", "bf_frame_wait", "bf_frame_release", "bf_render_frame",
    "bf_flow_field", "bf_color_flow_img", "bf_flow_frame_create", "bf_flow_frame_destroy", "bf_flow_frame_render",
    "bf_flow_frame_wait", "bf_flow_frame_release", "bf_render_flow_frame",
    "bf_global_hold_field", "bf_global_hold_best", "bf_global_get_flow", "bf_global_flow_field", "bf_global_color_flow_img",
    "bf_global_flow_frame_render", "bf_global_render_flow_frame", "bf_global_emit_slice",
    "bf_segment_opts_default", "bf_segment", "bf_segment_get", "bf_label_image",
    "bf_set_groups", "bf_set_groups_from_segments", "bf_run_groups", "bf_assign_groups",
    "bf_propose_models", "bf_project_groups", "bf_merge_scores", "bf_hold_groups", "bf_group_flow_medians",
    "bf_track_keep", "bf_track_overlap", "bf_track_drop",
]

BF_FRAME_PPM, BF_FRAME_AVI = 1, 2   # bf_frame_create layouts
BF_FLOW_FRAME_FLO = 4               # ... and bf_flow_frame_create's third
BF_FLOW_LAST_UPLOADED, BF_FLOW_FIRST_UPLOADED = 0, 1   # owner_rule of the per-pixel flow
BF_GLOBAL_HOLD_CELLS, BF_GLOBAL_HOLD_FIELD = 1, 2      # mode of bf_global_hold_field
# bf_get_stat "loop_form": the loop the last bf_run took
BF_LOOP_ATOMIC, BF_LOOP_BINNED, BF_LOOP_ONE_KERNEL, BF_LOOP_PERSISTENT, BF_LOOP_DELTA = 0, 1, 2, 3, 4

_lib = None


def device_numa_node(device=0):
    """Host NUMA node of HIP device `device` (-1: the platform does not say)."""
    node = C.c_int32(-1)
    load().bf_device_numa_node(device, C.byref(node))
    return node.value


def bind_thread_to_numa_node(node):
    """Bind the CALLING thread to the CPUs of host NUMA node `node` (that the process may use); returns the number of CPUs it
    is now bound to, 0 when nothing was done (unknown node, not a NUMA system, CPUs outside the container's cpuset)."""
    n = C.c_int32(0)
    rc = load().bf_bind_thread_to_numa_node(node, C.byref(n))
    if rc < 0:
        raise BfError(rc, "bf_bind_thread_to_numa_node(%d)" % node)
    return n.value


def bind_thread_to_device_numa(device=0):
    """bf_bind_thread_to_device_numa: the calling thread next to its GPU; returns the node (-1: unknown, nothing done)."""
    node = C.c_int32(-1)
    load().bf_bind_thread_to_device_numa(device, C.byref(node))
    return node.value


def run_many(accels, opts=None):
    """bf_run_many: the slices staged on `accels` (Accel objects, each after upload + set_cloud) solved together.
    Returns [(rc, Model, RunInfo)]."""
    n = len(accels)
    L = load()
    hs = (C.c_void_p * n)(*[a.h for a in accels])
    models = (Model * n)()
    infos = (RunInfo * n)()
    rc = L.bf_run_many(hs, n, C.byref(opts) if opts is not None else None, models, infos)
    if rc < 0:
        bad = next((a for a, i in zip(accels, infos) if i.rc < 0), accels[0])
        raise BfError(rc, L.bf_last_error(bad.h).decode())
    return [(infos[i].rc, models[i], infos[i]) for i in range(n)]


def run_tiles_many(accels, grid_rows, grid_cols, scale, sensor_res, guard_res, min_events, max_iter=-1, hard_iter_cap=20000):
    """bf_run_tiles_many: the tile grids of the slices uploaded on `accels` in one launch.  Returns [(models, infos)] per slice."""
    n = len(accels)
    L = accels[0].L
    o = TileOpts(grid_rows, grid_cols, scale, sensor_res[0], sensor_res[1], guard_res[0], guard_res[1], min_events, max_iter,
                 hard_iter_cap)
    nt = grid_rows * grid_cols
    hs = (C.c_void_p * n)(*[a.h for a in accels])
    models = (Model * (n * nt))()
    infos = (RunInfo * (n * nt))()
    rc = L.bf_run_tiles_many(hs, n, C.byref(o), models, infos)
    if rc < 0:
        raise BfError(rc, L.bf_last_error(accels[0].h).decode())
    return [(list(models[i * nt:(i + 1) * nt]), list(infos[i * nt:(i + 1) * nt])) for i in range(n)]


class BfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bf_accel error %d: %s" % (code, msg))
        self.code = code


_libs = {}


def load(path=None):
    """Load libbf_accel.so (or the build at `path`); raises (never falls back) when it has not been built."""
    global _lib
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError(
                "libbf_accel.so is missing (%s): build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C better_flow_amd/csrc`" % path)
        L = C.CDLL(path)
        L.bf_last_error.restype = C.c_char_p
        L.bf_version.restype = C.c_char_p
        L.bf_create.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                C.POINTER(C.c_void_p)]
        L.bf_destroy.argtypes = [C.c_void_p]
        L.bf_destroy.restype = None
        L.bf_last_error.argtypes = [C.c_void_p]
        L.bf_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.bf_get_stat.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
        L.bf_upload_events.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64]
        L.bf_upload_events_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64]
        L.bf_set_cloud.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Window)]
        L.bf_local_set_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                          C.POINTER(LocalWindow)]
        L.bf_local_iteration_step.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double), C.c_void_p]
        L.bf_local_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(LocalState)]
        L.bf_local_run_tiles.argtypes = [C.c_void_p, C.POINTER(LocalTileOpts), C.c_void_p, C.c_void_p]
        L.bf_global_search_opts_default.argtypes = [C.POINTER(GlobalSearchOpts)]
        L.bf_global_search_opts_default.restype = None
        L.bf_global_set_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(GlobalWindow)]
        L.bf_global_project_all.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int64)]
        L.bf_global_search.argtypes = [C.c_void_p, C.POINTER(GlobalSearchOpts), C.POINTER(GlobalResult), C.c_void_p, C.c_int64]
        L.bf_global_get_events.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.bf_global_set_cells.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(GlobalCells)]
        L.bf_global_search_cells.argtypes = [C.c_void_p, C.POINTER(GlobalSearchOpts), C.POINTER(GlobalResult), C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_int64]
        L.bf_global_search_cells_pyramid.argtypes = [C.c_void_p, C.POINTER(GlobalSearchOpts), C.POINTER(GlobalPyramidOpts),
                                                     C.c_void_p, C.POINTER(GlobalResult), C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_int64, C.c_void_p, C.c_int64, C.POINTER(GlobalPyramidInfo)]
        L.bf_global_project_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int64), C.c_void_p, C.c_int64]
        L.bf_global_project_field.argtypes = L.bf_global_project_cells.argtypes + [C.c_void_p] * 4
        L.bf_projection_img.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.bf_color_time_img.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.bf_upload_ring_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_int64, C.c_uint64]
        L.bf_upload_ring16_async.argtypes = L.bf_upload_ring_async.argtypes
        L.bf_upload_ring16t32_async.argtypes = L.bf_upload_ring_async.argtypes
        L.bf_upload_events16_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.bf_compute_uv_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        L.bf_wait_uploads.argtypes = [C.c_void_p]
        L.bf_project_4param_reinit.argtypes = [C.c_void_p] + [C.c_double] * 6
        L.bf_project_4param.argtypes = [C.c_void_p] + [C.c_double] * 6
        L.bf_get_time_img.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bf_segment_opts_default.argtypes = [C.POINTER(SegmentOpts)]
        L.bf_segment_opts_default.restype = None
        L.bf_segment.argtypes = [C.c_void_p, C.POINTER(SegmentOpts), C.POINTER(SegmentInfo)]
        L.bf_segment_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.bf_label_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.POINTER(C.c_int32)]
        L.bf_set_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.bf_set_groups_from_segments.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.bf_run_groups.argtypes = [C.c_void_p, C.POINTER(GroupOpts), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bf_assign_groups.argtypes = [C.c_void_p, C.POINTER(AssignOpts), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(AssignInfo)]
        L.bf_project_groups.argtypes = [C.c_void_p, C.POINTER(ProjectOpts), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(ProjectInfo)]
        L.bf_merge_scores.argtypes = [C.c_void_p, C.POINTER(MergeOpts), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(MergeInfo)]
        L.bf_track_keep.argtypes = [C.c_void_p, C.POINTER(TrackOpts), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(TrackInfo)]
        L.bf_track_overlap.argtypes = [C.c_void_p, C.POINTER(TrackOpts), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.POINTER(TrackInfo)]
        L.bf_track_drop.argtypes = [C.c_void_p]
        L.bf_propose_models.argtypes = [C.c_void_p, C.POINTER(GlobalSearchOpts), C.POINTER(AccelProposeOpts), C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ProposeInfo)]
        L.bf_sobel.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.bf_fast_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Model)]
        L.bf_writeout_events.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.bf_compute_uv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bf_set_model.argtypes = [C.c_void_p, C.POINTER(Model)]
        L.bf_run.argtypes = [C.c_void_p, C.POINTER(RunOpts), C.POINTER(Model), C.POINTER(RunInfo)]
        L.bf_run_tiles.argtypes = [C.c_void_p, C.POINTER(TileOpts), C.c_void_p, C.c_void_p]
        L.bf_run_tiles_many.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TileOpts), C.c_void_p, C.c_void_p]
        L.bf_run_many.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RunOpts), C.c_void_p, C.c_void_p]
        L.bf_get_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.bf_profile_enable.argtypes = [C.c_void_p, C.c_int32]
        L.bf_profile_reset.argtypes = [C.c_void_p]
        L.bf_profile_get.argtypes = [C.c_void_p, C.POINTER(Profile)]
        L.bf_synchronize.argtypes = [C.c_void_p]
        L.bf_copy_bandwidth.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
        L.bf_eval_sincos.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.bf_device_numa_node.argtypes = [C.c_int32, C.POINTER(C.c_int32)]
        L.bf_bind_thread_to_numa_node.argtypes = [C.c_int32, C.POINTER(C.c_int32)]
        L.bf_bind_thread_to_device_numa.argtypes = [C.c_int32, C.POINTER(C.c_int32)]
        L.bf_run_opts_default.argtypes = [C.POINTER(RunOpts)]
        L.bf_device_count.argtypes = [C.POINTER(C.c_int32)]
        L.bf_device_malloc.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.bf_device_free.argtypes = [C.c_void_p, C.c_void_p]
        L.bf_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.bf_host_alloc.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.bf_host_free.argtypes = [C.c_void_p, C.c_void_p]
        L.bf_upload_events_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.bf_commit_upload.argtypes = [C.c_void_p]
        # the device-side -o table (include/bf_accel.h: bf_emit_*)
        L.bf_emit_create.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]
        L.bf_emit_destroy.argtypes = [C.c_void_p]
        L.bf_emit_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.bf_emit_output.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint16)),
                                     C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.POINTER(C.c_double)),
                                     C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int64)]
        L.bf_emit_slice.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint64, C.c_int32,
                                    C.c_int32, C.POINTER(C.c_int64)]
        L.bf_emit_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
        L.bf_emit_release.argtypes = [C.c_void_p, C.c_uint64]
        # per-slice frames on the device (include/bf_accel.h: bf_frame_*, bf_render_frame)
        L.bf_frame_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bf_frame_destroy.argtypes = [C.c_void_p]
        L.bf_frame_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.bf_frame_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.POINTER(C.c_uint8)),
                                    C.POINTER(C.POINTER(C.c_uint8))]
        L.bf_frame_release.argtypes = [C.c_void_p, C.c_int64]
        L.bf_render_frame.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        # per-pixel flow (include/bf_accel.h: bf_flow_field, bf_color_flow_img, bf_flow_frame_*, bf_render_flow_frame)
        L.bf_flow_field.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bf_color_flow_img.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.bf_flow_frame_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bf_flow_frame_destroy.argtypes = [C.c_void_p]
        L.bf_flow_frame_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
        L.bf_flow_frame_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.POINTER(C.c_uint8)),
                                         C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_float))]
        L.bf_flow_frame_release.argtypes = [C.c_void_p, C.c_int64]
        L.bf_render_flow_frame.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        # the held flow of the exhaustive search (include/bf_accel.h: bf_global_hold_*, bf_global_get_flow and its outputs)
        L.bf_global_hold_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32]
        L.bf_global_hold_best.argtypes = [C.c_void_p]
        L.bf_global_get_flow.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        L.bf_hold_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.bf_group_flow_medians.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bf_global_flow_field.argtypes = L.bf_flow_field.argtypes
        L.bf_global_color_flow_img.argtypes = L.bf_color_flow_img.argtypes
        L.bf_global_flow_frame_render.argtypes = L.bf_flow_frame_render.argtypes
        L.bf_global_render_flow_frame.argtypes = L.bf_render_flow_frame.argtypes
        L.bf_global_emit_slice.argtypes = L.bf_emit_slice.argtypes
        _libs[path] = L
        if path == LIB_PATH:
            _lib = L
    return _libs[path]


def device_count():
    n = C.c_int32(0)
    load().bf_device_count(C.byref(n))
    return n.value


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _sweep(lo, hi, step):
    """The reference's `for (v = lo; v < hi; v += step)` (optimizer_global.cpp:134-135)."""
    out = []
    v = lo
    while step > 0 and v < hi and len(out) <= (1 << 26):
        out.append(v)
        v += step
    return out


class Accel:
    """One bf_ctx: the AccelLib-equivalent plus the fused OptimizerRolling::run."""

    def __init__(self, device=0, max_events=1 << 20, max_rows=1024, max_cols=1280, stream=None, lib=None):
        self.L = load(lib)
        h = C.c_void_p()
        rc = self.L.bf_create(device, max_events, max_rows, max_cols, stream, C.byref(h))
        if rc != BF_OK:
            raise BfError(rc, "bf_create failed (no HIP device?)" if rc == BF_ERR_NODEVICE
                          else "bf_create failed")
        self.h = h
        self.n = 0
        self.window = None
        self._gwin = None
        self._gcells = None

    def close(self):
        if getattr(self, "h", None):
            for p in getattr(self, "_pinned", []):
                self.L.bf_host_free(self.h, p)
            self._pinned = []
            self.L.bf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, ok=(BF_OK,)):
        if rc not in ok:
            raise BfError(rc, self.L.bf_last_error(self.h).decode())
        return rc

    def set_option(self, key, value):
        self._chk(self.L.bf_set_option(self.h, key.encode(), int(value)))

    def get_stat(self, key):
        v = C.c_int64(0)
        self._chk(self.L.bf_get_stat(self.h, key.encode(), C.byref(v)))
        return v.value

    def upload_events(self, fr_x, fr_y, t_ns, noise=None):
        fr_x = np.ascontiguousarray(fr_x, dtype=np.int32)
        fr_y = np.ascontiguousarray(fr_y, dtype=np.int32)
        t_ns = np.ascontiguousarray(t_ns, dtype=np.int32)
        if noise is not None:
            noise = np.ascontiguousarray(noise, dtype=np.uint8)
        self.n = len(fr_x)
        self._chk(self.L.bf_upload_events(self.h, _ptr(fr_x), _ptr(fr_y), _ptr(t_ns), _ptr(noise),
                                          self.n))

    def upload_events_device(self, d_fr_x, d_fr_y, d_t, n):
        self.n = int(n)
        self._chk(self.L.bf_upload_events_device(self.h, d_fr_x, d_fr_y, d_t, self.n))

    def set_cloud(self, scale=3, res_x=180, res_y=240):
        w = Window()
        self._chk(self.L.bf_set_cloud(self.h, scale, res_x, res_y, C.byref(w)))
        self.window = w
        return w

    def project_4param_reinit(self, dnx, dny, cx, cy, div, crl):
        self._chk(self.L.bf_project_4param_reinit(self.h, dnx, dny, cx, cy, div, crl))

    def project_4param(self, dnx, dny, cx, cy, div, crl):
        """The incremental warp (AccelLib::project_4param, accel_lib.h:275-281): dn added to the events' (nx, ny)."""
        self._chk(self.L.bf_project_4param(self.h, dnx, dny, cx, cy, div, crl))

    def get_time_img(self, want_time=True, want_count=True):
        R, Cc = self.window.scale_img_x, self.window.scale_img_y
        t = np.empty((R, Cc), dtype=np.float32) if want_time else None
        c = np.empty((R, Cc), dtype=np.uint32) if want_count else None
        self._chk(self.L.bf_get_time_img(self.h, _ptr(t), _ptr(c)))
        return t, c

    def sobel(self, img):
        img = np.ascontiguousarray(img, dtype=np.float32)
        gx = np.empty_like(img)
        gy = np.empty_like(img)
        self._chk(self.L.bf_sobel(self.h, _ptr(img), img.shape[0], img.shape[1], _ptr(gx), _ptr(gy)))
        return gx, gy

    # ---- moving-object segmentation (include/bf_accel.h) ----
    def segment(self, above_s=-1.0, below_s=-1.0, min_count=1, connectivity=8, min_pixels=1):
        """bf_segment: the time-image pass, then the components of the thresholded time image; returns SegmentInfo.  Labels,
        table and cl_id stay on the device (segment_get)."""
        o = SegmentOpts(above_s, below_s, min_count, connectivity, min_pixels, 0)
        info = SegmentInfo()
        self._chk(self.L.bf_segment(self.h, C.byref(o), C.byref(info)))
        self._seg_info = info
        return info

    def segment_get(self, want_labels=True, want_components=True, want_cl_id=True, comps_cap=None):
        """bf_segment_get: (labels (R, C) int32, components (COMPONENT_DTYPE rows), cl_id (n,) int32); None where not asked."""
        R, Cc = self.window.scale_img_x, self.window.scale_img_y
        K = getattr(self, "_seg_info", SegmentInfo()).components if comps_cap is None else comps_cap
        labels = np.empty((R, Cc), dtype=np.int32) if want_labels else None
        comps = np.zeros(K, dtype=COMPONENT_DTYPE) if want_components else None
        cl = np.empty(self.n, dtype=np.int32) if want_cl_id else None
        self._chk(self.L.bf_segment_get(self.h, _ptr(labels), _ptr(comps), K, _ptr(cl)))
        return labels, comps, cl

    def label_image(self, mask, connectivity=8, min_pixels=1, comps_cap=None):
        """bf_label_image: components of a host mask (non-zero = foreground); returns (labels, components, K).  comps_cap None:
        room for every possible component."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        R, Cc = mask.shape
        cap = (R * Cc + 1) // 2 if comps_cap is None else comps_cap
        labels = np.empty((R, Cc), dtype=np.int32)
        comps = np.zeros(cap, dtype=COMPONENT_DTYPE)
        k = C.c_int32(0)
        self._chk(self.L.bf_label_image(self.h, _ptr(mask), R, Cc, connectivity, min_pixels, _ptr(labels), _ptr(comps), cap,
                                        C.byref(k)))
        return labels, comps[:min(cap, k.value)], k.value

    def fast_model(self, img=None):
        m = Model()
        if img is None:
            self._chk(self.L.bf_fast_model(self.h, None, 0, 0, C.byref(m)))
        else:
            img = np.ascontiguousarray(img, dtype=np.float32)
            self._chk(self.L.bf_fast_model(self.h, _ptr(img), img.shape[0], img.shape[1], C.byref(m)))
        return m

    def writeout_events(self):
        out = [np.empty(self.n) for _ in range(4)]
        self._chk(self.L.bf_writeout_events(self.h, *[_ptr(a) for a in out]))
        return tuple(out)   # pr_x, pr_y, nx, ny

    def compute_uv(self):
        u, v = np.empty(self.n), np.empty(self.n)
        self._chk(self.L.bf_compute_uv(self.h, _ptr(u), _ptr(v)))
        return u, v

    def set_model(self, model):
        self._chk(self.L.bf_set_model(self.h, C.byref(model)))

    # ---- OptimizerLocal (optimizer_sampler.h:12-68): the contrast-score optimiser ----
    def local_set_window(self, scale, center=None, wsz=0):
        """center=None: window = bounding box of the cloud; else center = (fr_x, fr_y, t_ns) and wsz."""
        w = LocalWindow()
        cx, cy, ct = center if center is not None else (0, 0, 0)
        self._chk(self.L.bf_local_set_window(self.h, scale, wsz if center is not None else 0, cx, cy, ct,
                                             C.byref(w)))
        self._lwin = w
        return w

    def local_iteration_step(self, nx, ny, want_img=False):
        sc = C.c_double()
        img = np.empty((self._lwin.scale_img_x, self._lwin.scale_img_y), dtype=np.uint8) if want_img else None
        self._chk(self.L.bf_local_iteration_step(self.h, nx, ny, C.byref(sc), _ptr(img) if want_img else None))
        return (sc.value, img) if want_img else sc.value

    # ---- OptimizerGlobal (optimizer_global.h:11-57): the exhaustive (nx, ny) search ----
    def global_set_window(self, scale=None, metric_wsize=0):
        """The constructors (optimizer_global.h:27-41) + update_fields; resets every event's best state.
        No argument: OptimizerGlobal(events) -- scale 5, window 21; scale only: window 5 * scale."""
        if scale is None:
            scale, metric_wsize = 5, 21
        w = GlobalWindow()
        self._chk(self.L.bf_global_set_window(self.h, scale, metric_wsize, C.byref(w)))
        self._gwin = w
        self._gcells = None   # (the library clears the cells with the window)
        return w

    def global_project_all(self, nx, ny, nz=127.0, want_img=True, want_scores=True):
        """One project_all.  Returns (S, blurred bordered image or None, current_scores or None)."""
        w = self._gwin   # None before global_set_window: the library reports BF_ERR_ARG
        img = np.empty((w.scale_bordered_img_x, w.scale_bordered_img_y), dtype=np.uint8) if want_img and w else None
        sc = np.empty((w.scale_img_x, w.scale_img_y), dtype=np.float32) if want_scores and w else None
        S = C.c_int64()
        self._chk(self.L.bf_global_project_all(self.h, nx, ny, nz, _ptr(img), _ptr(sc), C.byref(S)))
        return S.value, img, sc

    @staticmethod
    def global_search_opts(**kw):
        """bf_global_search_opts with the reference's defaults, overridden by keyword."""
        o = GlobalSearchOpts()
        load().bf_global_search_opts_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def global_search(self, opts=None, want_surface=True, surface_cap=None):
        """compute_flow_bruteforce over opts (None: the defaults).  Returns (GlobalResult, surface [n_x, n_y] int64 or None)."""
        r = GlobalResult()
        o = opts if opts is not None else self.global_search_opts()
        surf = None
        if want_surface:
            nx = len(_sweep(o.x_low, o.x_hi, o.x_step))
            ny = len(_sweep(o.y_low, o.y_hi, o.y_step))
            surf = np.zeros(nx * ny if surface_cap is None else surface_cap, dtype=np.int64)
        self._chk(self.L.bf_global_search(self.h, C.byref(o), C.byref(r), _ptr(surf), 0 if surf is None else len(surf)))
        if surf is not None:
            surf = surf[:r.n_x * r.n_y].reshape(r.n_x, r.n_y)
        return r, surf

    def global_set_cells(self, res_x, res_y, cell_rows, cell_cols):
        """A grid of cell_rows x cell_cols-pixel cells over the res_x x res_y sensor, anchored at pixel (0, 0), for
        global_search_cells; valid until the next global_set_window or upload.  Returns GlobalCells (n_cell_x, n_cell_y)."""
        g = GlobalCells()
        self._gcells = None
        self._chk(self.L.bf_global_set_cells(self.h, res_x, res_y, cell_rows, cell_cols, C.byref(g)))
        self._gcells = g
        return g

    def global_search_cells(self, opts=None, want_surface=False, cells_cap=None, surface_cap=None):
        """global_search with the objective kept per cell.  Returns (GlobalResult of the slice, structured array
        [n_cell_x, n_cell_y] with best_nx, best_ny, best_u, best_v, best_sum, best_index, events, and the surface
        S(k, cell) as int64 [n_cell_x, n_cell_y, n_x, n_y] or None)."""
        r = GlobalResult()
        o = opts if opts is not None else self.global_search_opts()
        g = self._gcells   # None before global_set_cells: the library reports BF_ERR_ARG
        nc = g.n_cell_x * g.n_cell_y if g else 0
        cells = np.zeros(nc if cells_cap is None else cells_cap, dtype=np.dtype(GlobalCellResult))
        surf = None
        if want_surface:
            k = len(_sweep(o.x_low, o.x_hi, o.x_step)) * len(_sweep(o.y_low, o.y_hi, o.y_step))
            if surface_cap is None:
                surface_cap = nc * k if nc * k <= (1 << 27) else 1   # (over the cap: the library refuses before it writes)
            surf = np.zeros(surface_cap, dtype=np.int64)
        self._chk(self.L.bf_global_search_cells(self.h, C.byref(o), C.byref(r), _ptr(cells), len(cells), _ptr(surf),
                                                0 if surf is None else len(surf)))
        if surf is not None:
            surf = surf[:nc * r.n_x * r.n_y].reshape(g.n_cell_x, g.n_cell_y, r.n_x, r.n_y)
        return r, cells[:nc].reshape(g.n_cell_x, g.n_cell_y), surf

    def global_search_cells_pyramid(self, opts=None, levels=1, factor=2, radius=1, seeds=None, want_surface=False,
                                    cells_cap=None, evaluated_cap=None, surface_cap=None):
        """global_search_cells over a candidate set decided on the device (bf_global_search_cells_pyramid): a strided pass
        over the lattice of opts and `levels - 1` refinements around every cell's own best, or, with seeds (one lattice index
        or -1 per cell, any shape of n_cell_x * n_cell_y entries: usually the previous slice's best_index), `levels`
        refinements around them.  evaluated_cap None: room for the whole lattice.  Returns (GlobalResult of the slice, the
        structured cell array of global_search_cells, the evaluated lattice indices in evaluation order (int64),
        S(k, cell) as int64 [n_cell_x, n_cell_y, n_evaluated] or None, GlobalPyramidInfo)."""
        r, info = GlobalResult(), GlobalPyramidInfo()
        o = opts if opts is not None else self.global_search_opts()
        p = GlobalPyramidOpts(levels, factor, radius)
        g = self._gcells   # None before global_set_cells: the library reports BF_ERR_ARG
        nc = g.n_cell_x * g.n_cell_y if g else 0
        cells = np.zeros(nc if cells_cap is None else cells_cap, dtype=np.dtype(GlobalCellResult))
        k = len(_sweep(o.x_low, o.x_hi, o.x_step)) * len(_sweep(o.y_low, o.y_hi, o.y_step)) if o.x_step > 0 and o.y_step > 0 else 0
        ev = np.zeros(k if evaluated_cap is None else evaluated_cap, dtype=np.int64)
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
        if sd is not None and len(sd) != nc:
            raise ValueError("seeds: %d entries for %d cells" % (len(sd), nc))
        surf = None
        if want_surface:
            if surface_cap is None:
                surface_cap = min(nc * k, 1 << 27)
            surf = np.zeros(max(surface_cap, 1), dtype=np.int64)
        self._chk(self.L.bf_global_search_cells_pyramid(self.h, C.byref(o), C.byref(p), _ptr(sd), C.byref(r), _ptr(cells),
                                                        len(cells), _ptr(ev), len(ev), _ptr(surf),
                                                        0 if surf is None else surface_cap, C.byref(info)))
        ne = info.evaluated
        if surf is not None:
            surf = surf[:nc * ne].reshape(g.n_cell_x, g.n_cell_y, ne)
        return r, cells[:nc].reshape(g.n_cell_x, g.n_cell_y), ev[:ne].copy(), surf, info

    def _project_runs_args(self, cell_nx, cell_ny, want_img, want_scores, want_cell_sums):
        """What global_project_cells and global_project_field pass alike: the grids as flat float64 arrays (ValueError when
        their lengths differ) and the output buffers asked for, the per-cell sums as [n_cell_x, n_cell_y].  Returns
        (cx, cy, img, sc, sums)."""
        w, g = self._gwin, self._gcells   # None before global_set_window / global_set_cells: the library reports BF_ERR_ARG
        cx = np.ascontiguousarray(np.asarray(cell_nx, dtype=np.float64).reshape(-1))
        cy = np.ascontiguousarray(np.asarray(cell_ny, dtype=np.float64).reshape(-1))
        if len(cx) != len(cy):
            raise ValueError("cell_nx has %d entries, cell_ny %d" % (len(cx), len(cy)))
        img = np.empty((w.scale_bordered_img_x, w.scale_bordered_img_y), dtype=np.uint8) if want_img and w else None
        sc = np.empty((w.scale_img_x, w.scale_img_y), dtype=np.float32) if want_scores and w else None
        sums = np.zeros((g.n_cell_x, g.n_cell_y) if g else 0, dtype=np.int64) if want_cell_sums else None
        return cx, cy, img, sc, sums

    def global_project_cells(self, cell_nx, cell_ny, nz=127.0, want_img=True, want_scores=True, want_cell_sums=True):
        """The piecewise projection (bf_global_project_cells): the slice rendered and scored with every event under its own
        cell's (nx, ny).  cell_nx / cell_ny: n_cell_x * n_cell_y values in any shape, row-major [n_cell_x, n_cell_y] (for
        instance global_search_cells' cells["best_nx"], cells["best_ny"]); the entry of a cell without events is not read.
        The per-event state is not touched.  want_cell_sums False passes no per-cell buffer, like want_img and want_scores
        for theirs.  Returns (blurred bordered image or None, current_scores or None, S_pw,
        S_pw(cell) as int64 [n_cell_x, n_cell_y] or None)."""
        cx, cy, img, sc, sums = self._project_runs_args(cell_nx, cell_ny, want_img, want_scores, want_cell_sums)
        S = C.c_int64()
        self._chk(self.L.bf_global_project_cells(self.h, _ptr(cx), _ptr(cy), len(cx), nz, _ptr(img), _ptr(sc), C.byref(S),
                                                 _ptr(sums), 0 if sums is None else sums.size))
        return img, sc, S.value, sums

    def global_project_field(self, cell_nx, cell_ny, nz=127.0, want_img=True, want_scores=True, want_events=False,
                             want_cell_sums=True):
        """The interpolated field (bf_global_project_field): global_project_cells with the (nx, ny) of every event
        interpolated between the centres of the cells around its recorded address.  cell_nx / cell_ny as there, but EVERY
        entry is read and must be finite.  The per-event state is not touched.  Returns (blurred bordered image or None,
        current_scores or None, S_f, S_f(cell) as int64 [n_cell_x, n_cell_y] or None) and, with want_events, a fifth item:
        the dict of nx, ny (the interpolated values) and u, v (compute_uv of them), n doubles each in upload order."""
        cx, cy, img, sc, sums = self._project_runs_args(cell_nx, cell_ny, want_img, want_scores, want_cell_sums)
        keys = ("nx", "ny", "u", "v")
        ev = {k: np.zeros(self.n, dtype=np.float64) for k in keys} if want_events else None
        S = C.c_int64()
        self._chk(self.L.bf_global_project_field(self.h, _ptr(cx), _ptr(cy), len(cx), nz, _ptr(img), _ptr(sc), C.byref(S),
                                                 _ptr(sums), 0 if sums is None else sums.size,
                                                 *[_ptr(ev[k]) if ev else None for k in keys]))
        return (img, sc, S.value, sums, ev) if want_events else (img, sc, S.value, sums)

    def global_get_events(self):
        """Per-event state in upload order: dict of max_score, best_nx, best_ny, best_pr_x, best_pr_y, best_u, best_v."""
        keys = ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y", "best_u", "best_v")
        out = {k: np.zeros(self.n, dtype=np.float64) for k in keys}
        self._chk(self.L.bf_global_get_events(self.h, *[_ptr(out[k]) for k in keys]))
        return out

    def projection_img(self, scale, res_x, res_y, show_final=False):
        """EventFile::projection_img (event_file.h:460-515): the (motion-compensated) 8-bit event image."""
        img = np.empty((res_x * scale, res_y * scale), dtype=np.uint8)
        self._chk(self.L.bf_projection_img(self.h, scale, res_x, res_y, 1 if show_final else 0, _ptr(img)))
        return img

    def color_time_img(self, scale, res_x, res_y, show_final=False):
        """EventFile::color_time_img (event_file.h:649-747): B, G, R colour-coded time image of the slice."""
        sc = scale if scale else 11
        img = np.empty((res_x * sc + sc, res_y * sc + sc, 3), dtype=np.uint8)
        self._chk(self.L.bf_color_time_img(self.h, scale, res_x, res_y, 1 if show_final else 0, _ptr(img)))
        return img

    def render_frame(self, res_x, res_y, ppm=True, avi=True):
        """DVS_flow::render_frame's frame of the live slice, composed on the device (bf_render_frame): returns (ppm, avi),
        the PPM payload as a (6 res_x, 6 res_y, 3) RGB array, the AVI payload as a (6 res_x, stride) byte array of bottom-up
        BGR rows padded to a multiple of 4 bytes; None for a layout not asked for."""
        rows, cols = 6 * res_x, 6 * res_y
        p = np.empty((rows, cols, 3), dtype=np.uint8) if ppm else None
        a = np.empty((rows, (cols * 3 + 3) & ~3), dtype=np.uint8) if avi else None
        self._chk(self.L.bf_render_frame(self.h, res_x, res_y, _ptr(p), _ptr(a)))
        return p, a

    def flow_field(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED, _call=None):
        """The per-pixel flow field of the live slice (bf_flow_field): (owner, u, v), each (res_x, res_y) -- the upload index
        of the event that owns the pixel (-1: none) and its (best_u, best_v) as bf_compute_uv returns them (0: none)."""
        owner = np.empty((res_x, res_y), dtype=np.int32)
        u, v = np.empty((res_x, res_y)), np.empty((res_x, res_y))
        self._chk((_call or self.L.bf_flow_field)(self.h, res_x, res_y, owner_rule, _ptr(owner), _ptr(u), _ptr(v)))
        return owner, u, v

    def color_flow_img(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED, want_hs=False, _call=None):
        """EventFile::color_flow_img (event_file.h:318-350): the (res_x, res_y, 3) B, G, R colour-coded flow of the live
        slice; with want_hs also the (res_x, res_y, 2) H and S bytes before the conversion."""
        bgr = np.empty((res_x, res_y, 3), dtype=np.uint8)
        hs = np.empty((res_x, res_y, 2), dtype=np.uint8) if want_hs else None
        self._chk((_call or self.L.bf_color_flow_img)(self.h, res_x, res_y, owner_rule, _ptr(bgr), _ptr(hs)))
        return (bgr, hs) if want_hs else bgr

    def render_flow_frame(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED, ppm=True, avi=True, flo=True, _call=None):
        """The flow frame of the live slice, composed on the device (bf_render_flow_frame): compensated events | colour-coded
        flow | raw events.  Returns (ppm, avi, flo): the PPM payload as a (res_x, 3 res_y, 3) RGB array, the AVI payload as a
        (res_x, stride) byte array of bottom-up BGR rows, the .flo payload as (res_x, res_y, 2) float32 (horizontal = v,
        vertical = u; 1e9 without an event); None for a layout not asked for."""
        p = np.empty((res_x, 3 * res_y, 3), dtype=np.uint8) if ppm else None
        a = np.empty((res_x, (9 * res_y + 3) & ~3), dtype=np.uint8) if avi else None
        f = np.empty((res_x, res_y, 2), dtype=np.float32) if flo else None
        self._chk((_call or self.L.bf_render_flow_frame)(self.h, res_x, res_y, owner_rule, _ptr(p), _ptr(a), _ptr(f)))
        return p, a, f

    # ---- the held flow of the exhaustive search (include/bf_accel.h: "the held flow") ----
    def global_hold_field(self, cell_nx, cell_ny, nz=127.0, mode=BF_GLOBAL_HOLD_FIELD):
        """Keeps on the device the flow global_project_field (mode BF_GLOBAL_HOLD_FIELD) or global_project_cells
        (BF_GLOBAL_HOLD_CELLS) would project every event under; grids and refusals as there.  Nothing is rendered or scored."""
        cx, cy, _, _, _ = self._project_runs_args(cell_nx, cell_ny, False, False, False)
        self._chk(self.L.bf_global_hold_field(self.h, _ptr(cx), _ptr(cy), len(cx), nz, mode))

    def global_hold_best(self):
        """Keeps on the device a snapshot of the searches' per-event best flow (bf_global_hold_best)."""
        self._chk(self.L.bf_global_hold_best(self.h))

    def global_get_flow(self, keys=("nx", "ny", "u", "v", "pr_x", "pr_y")):
        """The held flow (bf_global_get_flow): dict of the arrays asked for, n doubles each in upload order."""
        every = ("nx", "ny", "u", "v", "pr_x", "pr_y")
        out = {k: np.zeros(self.n, dtype=np.float64) for k in keys}
        self._chk(self.L.bf_global_get_flow(self.h, *[_ptr(out.get(k)) for k in every]))
        return out

    def global_flow_field(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED):
        """flow_field of the held flow (bf_global_flow_field): every event, the held (u, v) of the owner as bits."""
        return self.flow_field(res_x, res_y, owner_rule, _call=self.L.bf_global_flow_field)

    def global_color_flow_img(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED, want_hs=False):
        """color_flow_img of the held flow (bf_global_color_flow_img)."""
        return self.color_flow_img(res_x, res_y, owner_rule, want_hs, _call=self.L.bf_global_color_flow_img)

    def global_render_flow_frame(self, res_x, res_y, owner_rule=BF_FLOW_LAST_UPLOADED, ppm=True, avi=True, flo=True):
        """render_flow_frame of the held flow (bf_global_render_flow_frame): held positions | colour-coded flow | raw events."""
        return self.render_flow_frame(res_x, res_y, owner_rule, ppm, avi, flo, _call=self.L.bf_global_render_flow_frame)

    def local_run(self, res_x=180, res_y=240, max_evaluations=100000):
        st = LocalState()
        rc = self.L.bf_local_run(self.h, res_x, res_y, max_evaluations, C.byref(st))
        if rc < 0:
            self._chk(rc)
        return rc, st

    def local_run_tiles(self, grid_rows, grid_cols, scale, wsz, sensor_res, guard_res, max_evaluations=100000):
        """A grid of OptimizerLocal windows, one per sensor tile on the tile's own events (bf_local_run_tiles);
        returns ([LocalState], [rc])."""
        o = LocalTileOpts(grid_rows, grid_cols, scale, wsz, sensor_res[0], sensor_res[1], guard_res[0], guard_res[1], max_evaluations)
        nt = grid_rows * grid_cols
        st = (LocalState * nt)()
        rcs = (C.c_int32 * nt)()
        self._chk(self.L.bf_local_run_tiles(self.h, C.byref(o), st, rcs))
        return list(st), list(rcs)

    def default_opts(self):
        o = RunOpts()
        self.L.bf_run_opts_default(C.byref(o))
        return o

    def run(self, opts=None):
        m, info = Model(), RunInfo()
        rc = self.L.bf_run(self.h, C.byref(opts) if opts is not None else None, C.byref(m),
                           C.byref(info))
        self._chk(rc, ok=(BF_OK, BF_SKIPPED))
        return rc, m, info

    def run_tiles(self, grid_rows, grid_cols, scale, sensor_res, guard_res, min_events, max_iter=-1,
                  hard_iter_cap=20000):
        """One independent optimizer per sensor tile (bf_run_tiles); returns (models, infos)."""
        o = TileOpts(grid_rows, grid_cols, scale, sensor_res[0], sensor_res[1], guard_res[0], guard_res[1],
                     min_events, max_iter, hard_iter_cap)
        nt = grid_rows * grid_cols
        models = (Model * nt)()
        infos = (RunInfo * nt)()
        self._chk(self.L.bf_run_tiles(self.h, C.byref(o), models, infos))
        return list(models), list(infos)

    def set_groups(self, group_id, groups):
        """bf_set_groups: a group id per event (-1 .. groups - 1, upload order) for bf_run_groups; holds until the next upload."""
        gid = np.ascontiguousarray(group_id, dtype=np.int32)
        self._chk(self.L.bf_set_groups(self.h, _ptr(gid), int(groups)))

    def set_groups_from_segments(self):
        """bf_set_groups_from_segments: the held segmentation's cl_id becomes the grouping, on the device; returns K."""
        k = C.c_int32(0)
        self._chk(self.L.bf_set_groups_from_segments(self.h, C.byref(k)))
        return k.value

    def run_groups(self, groups, scale, sensor_res, guard_res, min_events, warm=None, max_iter=-1, hard_iter_cap=20000):
        """bf_run_groups on the held grouping of `groups` groups: one optimizer per group, cold (warm None), every group from
        one Model, or from one Model per group (a sequence of `groups`).  Returns (models, infos, GroupInfo per group)."""
        o = GroupOpts(scale, sensor_res[0], sensor_res[1], guard_res[0], guard_res[1], min_events, max_iter, hard_iter_cap)
        if warm is None:
            wm, wn = None, 0
        elif isinstance(warm, Model):
            wm, wn = (Model * 1)(warm), 1
        else:
            wn = len(warm)
            wm = (Model * max(wn, 1))(*warm)
        K = max(int(groups), 0)
        models = (Model * max(K, 1))()
        infos = (RunInfo * max(K, 1))()
        ginfo = (GroupInfo * max(K, 1))()
        self._chk(self.L.bf_run_groups(self.h, C.byref(o), wm, wn, models, infos, ginfo))
        return list(models)[:K], list(infos)[:K], list(ginfo)[:K]

    def assign_groups(self, models, scale, sensor_res, margin=0, min_score=1, use_prior=False, install=True):
        """bf_assign_groups: every event to the one of the candidate `models` (a sequence of Model) under which it lands on the
        largest pile of other events; with use_prior the held grouping restricts who votes where; with install the result
        becomes the held grouping (len(models) groups) for run_groups.  Returns (gid int32[n], score int32[n],
        counts int32[K + 1] (last: unassigned), AssignInfo), per-event arrays in upload order."""
        K = len(models)
        o = AssignOpts(scale, sensor_res[0], sensor_res[1], margin, min_score, 1 if use_prior else 0, 1 if install else 0, 0)
        ms = (Model * max(K, 1))(*models)
        n = int(self.n)
        gid = np.zeros(n, dtype=np.int32)
        score = np.zeros(n, dtype=np.int32)
        counts = np.zeros(K + 1, dtype=np.int32)
        info = AssignInfo()
        self._chk(self.L.bf_assign_groups(self.h, C.byref(o), ms, K, _ptr(gid), _ptr(score), _ptr(counts), C.byref(info)))
        return gid, score, counts, info

    def project_groups(self, models, scale, sensor_res, margin=0, gain=8, want=("count", "label", "bgr")):
        """bf_project_groups: the slice with every event of the held grouping warped by its own group's model (`models`, one
        Model per group).  Returns (images, scores, ProjectInfo): images a dict with those of "count" (uint32 [R, C]), "label"
        (int32 [R, C], -1: no event) and "bgr" (uint8 [R, C, 3]) that `want` names, scores a list of GroupScore per group."""
        K = len(models)
        o = ProjectOpts(scale, sensor_res[0], sensor_res[1], margin, gain)
        ms = (Model * max(K, 1))(*models)
        R, C_ = max(scale * (sensor_res[0] + 2 * margin), 0), max(scale * (sensor_res[1] + 2 * margin), 0)   # the header's window
        if R * C_ > (1 << 27):   # (the entry refuses it: BF_ERR_ARG or BF_ERR_CAPACITY)
            R = C_ = 0
        shapes = {"count": ((R, C_), np.uint32), "label": ((R, C_), np.int32), "bgr": ((R, C_, 3), np.uint8)}
        unknown = [k for k in want if k not in shapes]
        if unknown:
            raise ValueError("project_groups: unknown outputs %s" % unknown)
        img = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in want}
        scores = (GroupScore * max(K, 1))()
        info = ProjectInfo()
        self._chk(self.L.bf_project_groups(self.h, C.byref(o), ms, K, _ptr(img.get("count")), _ptr(img.get("label")),
                                           _ptr(img.get("bgr")), scores, C.byref(info)))
        return img, list(scores)[:K], info

    def merge_scores(self, models, scale, sensor_res, margin=0, targets_per_pass=0):
        """bf_merge_scores: for every ordered pair (b, a) of the held grouping's groups, what the events of b add to the
        contrast sum N^2 under model a (`models`, one Model per group).  Returns (gain uint64 [K, K], inside int32 [K, K],
        events int32 [K], MergeInfo), the matrices indexed [b, a]: after "b adopts model a" the objective is
        info.sum_sq - gain[b, b] + gain[b, a]."""
        K = len(models)
        o = MergeOpts(scale, sensor_res[0], sensor_res[1], margin, targets_per_pass)
        ms = (Model * max(K, 1))(*models)
        gain = np.zeros((K, K), dtype=np.uint64)
        inside = np.zeros((K, K), dtype=np.int32)
        events = np.zeros(K, dtype=np.int32)
        info = MergeInfo()
        self._chk(self.L.bf_merge_scores(self.h, C.byref(o), ms, K, _ptr(gain), _ptr(inside), _ptr(events), C.byref(info)))
        return gain, inside, events, info

    def track_keep(self, models, scale, sensor_res, margin=0, want_plane=True):
        """bf_track_keep: the owner plane of the held grouping under `models` (project_groups' "label") is kept on the device
        across the next uploads, with its window and its number of groups, for track_overlap.  Returns (plane int32 [R, C] or
        None, TrackInfo)."""
        K = len(models)
        o = TrackOpts(scale, sensor_res[0], sensor_res[1], margin)
        ms = (Model * max(K, 1))(*models)
        plane = None
        if want_plane:
            R, C_ = max(scale * (sensor_res[0] + 2 * margin), 0), max(scale * (sensor_res[1] + 2 * margin), 0)   # the header's window
            if R * C_ > (1 << 27):   # (the entry refuses it: BF_ERR_ARG or BF_ERR_CAPACITY)
                R = C_ = 0
            plane = np.zeros((R, C_), dtype=np.int32)
        info = TrackInfo()
        self._chk(self.L.bf_track_keep(self.h, C.byref(o), ms, K, _ptr(plane), C.byref(info)))
        return plane, info

    def track_overlap(self, models, dt_ns, scale, sensor_res, margin=0):
        """bf_track_overlap: the events of every group of the held grouping, carried back by dt_ns (this slice's time origin
        minus the kept slice's) under the group's own model, counted by the owner of the kept plane's pixel they land on.
        Returns (overlap int32 [K, Kp + 1] (last column: a pixel nobody owns), inside int32 [K], TrackInfo)."""
        K = len(models)
        Kp = max(self.tracks_held, 0)
        o = TrackOpts(scale, sensor_res[0], sensor_res[1], margin)
        ms = (Model * max(K, 1))(*models)
        overlap = np.zeros((K, Kp + 1), dtype=np.int32)
        inside = np.zeros(K, dtype=np.int32)
        info = TrackInfo()
        self._chk(self.L.bf_track_overlap(self.h, C.byref(o), ms, K, int(dt_ns), _ptr(overlap), _ptr(inside), C.byref(info)))
        return overlap, inside, info

    def track_drop(self):
        """bf_track_drop: releases the kept plane."""
        self._chk(self.L.bf_track_drop(self.h))

    @property
    def tracks_held(self):
        """The groups Kp of the kept plane, -1 without one (bf_get_stat "tracks_held")."""
        return self.get_stat("tracks_held")

    def hold_groups(self, models):
        """bf_hold_groups: every event of the held grouping under its own group's model (`models`, one Model per group) becomes
        the held flow that global_get_flow, global_flow_field, global_color_flow_img, global_render_flow_frame and
        global_emit_slice read; an event of no group is held with zero flow.  Needs global_set_window on the slice."""
        K = len(models)
        ms = (Model * max(K, 1))(*models)
        self._chk(self.L.bf_hold_groups(self.h, ms, K))

    def group_flow_medians(self):
        """bf_group_flow_medians: per group of the held grouping the median per axis of the held flow's (u, v) over its events
        (the mean of the two middle values of an even count, 0 for an empty group).  Returns (u_med float64[K],
        v_med float64[K], counts int32[K + 1] (last: the events of no group))."""
        k = C.c_int64(0)
        self._chk(self.L.bf_get_stat(self.h, b"groups_held", C.byref(k)))
        K = max(int(k.value), 0)
        u = np.zeros(K, dtype=np.float64)
        v = np.zeros(K, dtype=np.float64)
        counts = np.zeros(K + 1, dtype=np.int32)
        self._chk(self.L.bf_group_flow_medians(self.h, _ptr(u), _ptr(v), _ptr(counts)))
        return u, v, counts

    def propose_models(self, opts=None, radius=1, suppress=2, max_models=8, min_votes=1, want_planes=False):
        """bf_propose_models: the modes of the per-event best flow global_search left over the lattice `opts` (a
        GlobalSearchOpts; None: the defaults) as candidate models for assign_groups.  Returns (models, proposals, ProposeInfo)
        -- lists of Model and Proposal in pick order -- and, with want_planes, the vote plane H and its box sums B as uint32
        [n_x, n_y]."""
        o = opts if opts is not None else self.global_search_opts()
        po = AccelProposeOpts(radius, suppress, max_models, min_votes)
        cap = max(int(max_models), 1)
        models = (Model * cap)()
        props = (Proposal * cap)()
        info = ProposeInfo()
        H = B = None
        if want_planes:
            bins = len(_sweep(o.x_low, o.x_hi, o.x_step)) * len(_sweep(o.y_low, o.y_hi, o.y_step))
            H = np.zeros(bins, dtype=np.uint32)
            B = np.zeros(bins, dtype=np.uint32)
        self._chk(self.L.bf_propose_models(self.h, C.byref(o), C.byref(po), models, props, cap, _ptr(H), _ptr(B),
                                           0 if H is None else len(H), C.byref(info)))
        out = (list(models)[:info.proposals], list(props)[:info.proposals], info)
        if want_planes:
            out += (H[:info.n_x * info.n_y].reshape(info.n_x, info.n_y), B[:info.n_x * info.n_y].reshape(info.n_x, info.n_y))
        return out

    def get_trace(self, cap):
        buf = (TraceRec * max(cap, 1))()
        n = C.c_int32(0)
        self._chk(self.L.bf_get_trace(self.h, buf, cap, C.byref(n)))
        return list(buf)[: n.value]

    def profile_enable(self, mode=1):
        self._chk(self.L.bf_profile_enable(self.h, mode))

    def profile_reset(self):
        self._chk(self.L.bf_profile_reset(self.h))

    def profile_get(self):
        p = Profile()
        self._chk(self.L.bf_profile_get(self.h, C.byref(p)))
        return p

    def synchronize(self):
        self._chk(self.L.bf_synchronize(self.h))

    def pinned_int32(self, n):
        """A pinned host int32 array of n elements (bf_host_alloc) viewed through numpy."""
        p = C.c_void_p()
        self._chk(self.L.bf_host_alloc(self.h, max(4 * n, 16), C.byref(p)))
        arr = np.ctypeslib.as_array((C.c_int32 * n).from_address(p.value))
        self._pinned = getattr(self, "_pinned", []) + [p]   # released in close()
        return arr

    def pinned_array(self, n, dtype):
        """A pinned host array of n elements of `dtype` (bf_host_alloc) viewed through numpy."""
        dt = np.dtype(dtype)
        p = C.c_void_p()
        self._chk(self.L.bf_host_alloc(self.h, max(dt.itemsize * n, 16), C.byref(p)))
        arr = np.frombuffer((C.c_uint8 * (dt.itemsize * n)).from_address(p.value), dtype=dt)
        self._pinned = getattr(self, "_pinned", []) + [p]   # released in close()
        return arr

    def upload_events_async(self, fr_x, fr_y, t_ns, n):
        """fr_x / fr_y / t_ns: pinned int32 arrays (pinned_int32), or uint16 addresses (pinned_array) with int32 times --
        8 instead of 12 bytes per event over the link (bf_upload_events16_async); returns immediately."""
        assert fr_x.dtype == fr_y.dtype and t_ns.dtype == np.int32
        fn = self.L.bf_upload_events16_async if fr_x.dtype == np.uint16 else self.L.bf_upload_events_async
        self._chk(fn(self.h, _ptr(fr_x), _ptr(fr_y), _ptr(t_ns), int(n)))
        self._pending_n = getattr(self, "_pending_n", []) + [int(n)]

    def upload_ring_async(self, ring_x, ring_y, ring_ts, first, n, t0, ring_noise=None, span_ns=None):
        """Slice = n events from ring index `first` (wrapping) of row / column / uint64 timestamp ring arrays (pinned for
        a true DMA; pageable arrays work too); times become ts - t0 on the device.  int32 addresses go through
        bf_upload_ring_async, uint16 addresses through bf_upload_ring16_async; ring_noise: optional uint8 Event::noise ring.

        A uint32 `ring_ts` holds the LOW 32 bits of the timestamps (bf_upload_ring16t32_async, 8 bytes per event): the device
        can only form (int32)(ts32 - (uint32)t0), which is the true difference while |ts - t0| < 2^31 ns (2.1 s) and a
        plausible-looking WRONG time beyond -- the 64-bit forms mark such an event and bf_set_cloud reports it, this form
        cannot.  So the caller, who has the full timestamps, must state the slice's span: `span_ns` = max |ts - t0| over the
        slice (required with uint32 timestamps); 2^31 or more is refused here."""
        assert ring_x.dtype == ring_y.dtype and ring_x.dtype in (np.int32, np.uint16) and ring_ts.dtype in (np.uint64, np.uint32)
        assert ring_noise is None or ring_noise.dtype == np.uint8
        if ring_ts.dtype == np.uint32:   # the low 32 bits of the timestamps: 8 bytes per event (bf_upload_ring16t32_async)
            assert ring_x.dtype == np.uint16
            if span_ns is None:
                raise ValueError("uint32 timestamps: pass span_ns = max |timestamp - t0| of the slice (from the full timestamps)")
            if not (0 <= int(span_ns) < (1 << 31)):
                raise BfError(BF_ERR_ARG, "a slice that reaches %d ns from its start does not fit 32-bit local times (limit 2^31 ns)" % int(span_ns))
            fn = self.L.bf_upload_ring16t32_async
        else:
            fn = self.L.bf_upload_ring_async if ring_x.dtype == np.int32 else self.L.bf_upload_ring16_async
        self._chk(fn(self.h, _ptr(ring_x), _ptr(ring_y), _ptr(ring_ts), None if ring_noise is None else _ptr(ring_noise),
                     int(len(ring_ts)), int(first), int(n), int(t0)))
        self._pending_n = getattr(self, "_pending_n", []) + [int(n)]

    def compute_uv_ring(self, uv_ring, first):
        """Per-event (u, v) of the current slice as interleaved pairs into uv_ring (float64, 2 * cap), event i at ring
        index (first + i) % cap (bf_compute_uv_ring)."""
        assert uv_ring.dtype == np.float64 and uv_ring.size % 2 == 0
        self._chk(self.L.bf_compute_uv_ring(self.h, _ptr(uv_ring), int(uv_ring.size // 2), int(first)))

    def wait_uploads(self):
        """Block until every asynchronous upload issued so far has been copied (bf_wait_uploads)."""
        self._chk(self.L.bf_wait_uploads(self.h))

    def commit_upload(self):
        self._chk(self.L.bf_commit_upload(self.h))
        self.n = self._pending_n.pop(0)

    def to_device(self, arr):
        """Copy a numpy array into a fresh device buffer; returns the device pointer."""
        arr = np.ascontiguousarray(arr)
        d = C.c_void_p()
        self._chk(self.L.bf_device_malloc(self.h, max(arr.nbytes, 16), C.byref(d)))
        if arr.nbytes:
            self._chk(self.L.bf_memcpy_h2d(self.h, d, _ptr(arr), arr.nbytes))
        return d

    def device_free(self, d):
        self._chk(self.L.bf_device_free(self.h, d))

    def eval_sincos(self, x, table=False):
        """The device loops' sin / cos (bf_eval_sincos) of the float64 array x -> (sin, cos)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        sn, cs = np.empty_like(x), np.empty_like(x)
        self._chk(self.L.bf_eval_sincos(self.h, x.ctypes.data, x.size, 1 if table else 0, sn.ctypes.data, cs.ctypes.data))
        return sn, cs

    def copy_bandwidth(self, nbytes=1 << 30, reps=5):
        g = C.c_double(0)
        self._chk(self.L.bf_copy_bandwidth(self.h, nbytes, reps, C.byref(g)))
        return g.value


class Emit:
    """One bf_emit: the -o table accumulated on the device (include/bf_accel.h, bf_emit_*), minimal.  slice() enqueues one
    slice of `accel`'s context -- with the rolling optimiser's flow, or with held=True the held flow of the exhaustive
    search (bf_global_emit_slice) -- waits for it, copies its rows out of the pinned ring and releases them."""

    def __init__(self, accel, ring_cap, rows, cols, out_rows):
        self.acc, self.L = accel, accel.L
        self.h = C.c_void_p()
        accel._chk(self.L.bf_emit_create(accel.h, ring_cap, rows, cols, out_rows, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.bf_emit_destroy(self.h)
            self.h = None

    def slice(self, n, first, start_time, lead=None, held=False):
        """lead: None or (t, row, col) of the ring's oldest element.  Returns (ticket, rows): ticket -1 and rows None when
        there was nothing to enqueue, else rows = dict of t (uint64), row, col (uint16), u, v (float64)."""
        call = self.L.bf_global_emit_slice if held else self.L.bf_emit_slice
        lt, lr, lc = lead if lead is not None else (0, 0, 0)
        ticket = C.c_int64(-2)
        self.acc._chk(call(self.acc.h, self.h, n, first, start_time, 0 if lead is None else 1, lt, lr, lc, C.byref(ticket)))
        if ticket.value < 0:
            return ticket.value, None
        first_row, rows = C.c_uint64(), C.c_int64()
        self.acc._chk(self.L.bf_emit_wait(self.acc.h, self.h, ticket.value, C.byref(first_row), C.byref(rows)))
        cols = [C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint16)(), C.POINTER(C.c_uint16)(), C.POINTER(C.c_double)(),
                C.POINTER(C.c_double)()]
        R = C.c_int64()
        self.acc._chk(self.L.bf_emit_output(self.h, *[C.byref(x) for x in cols], C.byref(R)))
        idx = (first_row.value + np.arange(rows.value, dtype=np.uint64)) % np.uint64(R.value)
        out = {k: np.ctypeslib.as_array(x, shape=(R.value,))[idx].copy() for k, x in zip(("t", "row", "col", "u", "v"), cols)}
        self.acc._chk(self.L.bf_emit_release(self.h, first_row.value + rows.value))
        return ticket.value, out
