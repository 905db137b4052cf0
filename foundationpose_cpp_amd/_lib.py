"""ctypes loader for libfoundationpose_amd.so (the C ABI of include/foundationpose_amd.h).

The library is the product: there is NO CPU fallback.  If it is missing or cannot be loaded this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FP_LIB_PATH") or os.path.join(_HERE, "libfoundationpose_amd.so")  # FP_LIB_PATH: experimental builds (tools/)
CSRC = os.path.join(_HERE, "csrc")

# every symbol include/foundationpose_amd.h declares
SYMBOLS = [
    "fp_create", "fp_create_on", "fp_device", "fp_register_sharded", "fp_destroy", "fp_last_error", "fp_set_inplane_steps", "fp_num_hypotheses",
    "fp_register", "fp_track", "fp_register_ex", "fp_track_ex", "fp_track_submit", "fp_track_wait", "fp_track_multi",
    "fp_upload_frame", "fp_get_xyz_map", "fp_get_hyp_poses", "fp_filter_depth",
    "fp_render_and_transform", "fp_debug_rasterize", "fp_refiner_infer", "fp_scorer_infer",
    "fp_refine_post_process", "fp_argmax", "fp_register_shard_begin", "fp_register_shard_finish", "fp_register_shard_begin_packed", "fp_register_shard_finish_packed", "fp_download",
    "fp_profile_enable", "fp_profile_reset", "fp_profile_report", "fp_stream", "fp_synchronize",
    "fp_mesh_load_obj", "fp_mesh_free", "fp_mesh_view", "fp_mesh_orient_bounds",
    "fp_image_read_png", "fp_frame_size", "fp_read_rgb_depth_mask", "fp_read_cam_k", "fp_image_write_png_rgb",
    "fp_draw_bbox3d", "fp_set_precision", "fp_get_precision", "fp_calibrate_fp8", "fp_calibrate", "fp_calibrate_begin", "fp_calibrate_add_frame", "fp_calibrate_finish", "fp_calibrate_abort", "fp_calibrate_frames", "fp_calibration_size", "fp_get_calibration_blob", "fp_set_calibration_blob", "fp_get_calibration", "fp_set_calibration", "fp_set_float_model", "fp_get_float_model", "fp_net_create", "fp_net_destroy", "fp_net_max_batch", "fp_net_blob", "fp_net_infer",
    "fp_set_pose_fit", "fp_get_pose_fit", "fp_last_track_fit", "fp_last_register_fit", "fp_pose_fit_eval",
    "fp_mesh_color_source", "fp_mesh_vertex_colors", "fp_set_vertex_colors", "fp_get_color_source",
    "fp_set_depth_filter", "fp_get_depth_filter",
    "fp_render_pose", "fp_render_scene", "fp_pose_errors", "fp_pose_vsd", "fp_refine_depth", "fp_pose_search", "fp_register_depth",
    "fp_pose_color", "fp_resolve_symmetry", "fp_mask_distance", "fp_pose_silhouette",
    "fp_refine_silhouette",
]


class FpPoseFit(C.Structure):
    """fp_pose_fit of include/foundationpose_amd.h"""
    _fields_ = [("n_model", C.c_int32), ("n_observed", C.c_int32), ("n_inlier", C.c_int32), ("n_front", C.c_int32),
                ("n_behind", C.c_int32), ("reserved", C.c_int32), ("sum_dz_q20", C.c_int64), ("mean_dz_m", C.c_float),
                ("tol_n", C.c_float)]


class FpFrameRender(C.Structure):
    """fp_frame_render of include/foundationpose_amd.h: every pointer optional, all in the call's memspace"""
    _fields_ = [("model_depth", C.c_void_p), ("model_mask", C.c_void_p), ("visible_mask", C.c_void_p), ("tri_id", C.c_void_p),
                ("overlay", C.c_void_p)]


class FpSceneRender(C.Structure):
    """fp_scene_render of include/foundationpose_amd.h: every pointer optional, all in the call's memspace"""
    _fields_ = [("model_depth", C.c_void_p), ("instance_id", C.c_void_p), ("visible_mask", C.c_void_p), ("tri_id", C.c_void_p),
                ("cover_bits", C.c_void_p), ("overlay", C.c_void_p)]


class FpSceneObject(C.Structure):
    """fp_scene_object of include/foundationpose_amd.h"""
    _fields_ = [("n_covered", C.c_int32), ("n_front", C.c_int32), ("n_hidden", C.c_int32), ("n_visible", C.c_int32),
                ("n_occluded", C.c_int32), ("reserved", C.c_int32 * 3)]


class FpPoseError(C.Structure):
    """fp_pose_error of include/foundationpose_amd.h"""
    _fields_ = [("add_m", C.c_float), ("adds_m", C.c_float), ("mssd_m", C.c_float), ("mspd_px", C.c_float), ("rot_deg", C.c_float),
                ("trans_m", C.c_float), ("best_sym", C.c_int32), ("best_sym_mspd", C.c_int32), ("add_sum_q20", C.c_int64),
                ("adds_sum_q20", C.c_int64), ("n_vertices", C.c_int32), ("reserved", C.c_int32)]


FP_VSD_MAX_TAUS = 16


class FpPoseVsd(C.Structure):
    """struct fp_pose_vsd of include/foundationpose_amd.h"""
    _fields_ = [("n_model_est", C.c_int32), ("n_model_gt", C.c_int32), ("n_visib_est", C.c_int32), ("n_visib_gt", C.c_int32),
                ("n_inter", C.c_int32), ("n_union", C.c_int32), ("n_fail", C.c_int32 * FP_VSD_MAX_TAUS), ("vsd", C.c_float * FP_VSD_MAX_TAUS),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class FpDepthRefine(C.Structure):
    """struct fp_depth_refine of include/foundationpose_amd.h"""
    _fields_ = [("n_model", C.c_int32), ("n_valid", C.c_int32), ("n_used", C.c_int32), ("n_front", C.c_int32), ("n_behind", C.c_int32),
                ("n_grazing", C.c_int32), ("iterations", C.c_int32), ("rank", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
                ("rms_m", C.c_float), ("cond", C.c_float), ("last_rot_rad", C.c_float), ("last_trans_m", C.c_float),
                ("sums_q32", C.c_int64 * 28)]


class FpPoseSearch(C.Structure):
    """struct fp_pose_search of include/foundationpose_amd.h"""
    _fields_ = [("n_facing", C.c_int32), ("n_inlier", C.c_int32), ("n_front", C.c_int32), ("n_behind", C.c_int32), ("n_outside", C.c_int32),
                ("n_missing", C.c_int32), ("score", C.c_int32), ("best_step", C.c_int32), ("n_points", C.c_int32), ("status", C.c_int32)]


class FpPoseColor(C.Structure):
    """struct fp_pose_color of include/foundationpose_amd.h"""
    _fields_ = [("n_model", C.c_int32), ("n_visible", C.c_int32), ("n_compared", C.c_int32), ("n_nocolor", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32), ("sum_m", C.c_int64 * 3), ("sum_o", C.c_int64 * 3), ("sum_mm", C.c_int64 * 3), ("sum_oo", C.c_int64 * 3),
                ("sum_mo", C.c_int64 * 3), ("zncc", C.c_float), ("reserved_f", C.c_float)]


class FpPoseSilhouette(C.Structure):
    """struct fp_pose_silhouette of include/foundationpose_amd.h"""
    _fields_ = [("n_model", C.c_int32), ("n_visible", C.c_int32), ("n_inter", C.c_int32), ("n_spill", C.c_int32), ("n_mask", C.c_int32),
                ("n_miss", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32), ("sum_spill_d2", C.c_int64), ("sum_miss_d2", C.c_int64),
                ("iou", C.c_float), ("rms_spill_px", C.c_float), ("rms_miss_px", C.c_float), ("reserved_f", C.c_float)]


class FpSilhouetteRefine(C.Structure):
    """struct fp_silhouette_refine of include/foundationpose_amd.h"""
    _fields_ = [("n_model", C.c_int32), ("n_contour", C.c_int32), ("n_used", C.c_int32), ("n_occluded", C.c_int32), ("n_far", C.c_int32),
                ("n_flat", C.c_int32), ("n_steep", C.c_int32), ("iterations", C.c_int32), ("rank", C.c_int32), ("status", C.c_int32),
                ("rms_px", C.c_float), ("scale_px", C.c_float), ("cond", C.c_float), ("last_rot_rad", C.c_float), ("last_trans_m", C.c_float),
                ("reserved_f", C.c_float), ("sums_q24", C.c_int64 * 28)]


class FpDepthRegister(C.Structure):
    """struct fp_depth_register of include/foundationpose_amd.h"""
    _fields_ = [("hypothesis", C.c_int32), ("n_hypotheses", C.c_int32), ("n_candidates", C.c_int32), ("rank_key", C.c_int32),
                ("search", FpPoseSearch), ("refine", FpDepthRefine)]


class FpMesh(C.Structure):
    _fields_ = [("name", C.c_char_p), ("num_vertices", C.c_int), ("num_faces", C.c_int),
                ("vertices", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p),
                ("faces", C.c_void_p), ("texture", C.c_void_p), ("tex_height", C.c_int),
                ("tex_width", C.c_int), ("diameter", C.c_float), ("center", C.c_float * 3)]


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-8000:])
    if res.returncode != 0:
        raise RuntimeError("building libfoundationpose_amd.so failed")
    return LIB_PATH


_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    _LIB = _declare(L)
    return L


def _declare(L: C.CDLL) -> C.CDLL:
    """check that L exports the C ABI and give every fp_* entry point its signature"""
    for s in SYMBOLS:
        getattr(L, s)  # raises AttributeError if the library does not export the symbol
    L.fp_create.restype = C.c_void_p
    L.fp_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.fp_create_on.restype = C.c_void_p
    L.fp_create_on.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.fp_destroy.argtypes = [C.c_void_p]
    L.fp_destroy.restype = None
    L.fp_last_error.restype = C.c_char_p
    L.fp_stream.restype = C.c_void_p
    L.fp_stream.argtypes = [C.c_void_p]
    L.fp_mesh_load_obj.restype = C.c_void_p
    L.fp_mesh_load_obj.argtypes = [C.c_char_p, C.c_char_p]
    L.fp_mesh_free.restype = None
    L.fp_mesh_free.argtypes = [C.c_void_p]
    L.fp_image_read_png.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.fp_frame_size.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    L.fp_read_rgb_depth_mask.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fp_read_cam_k.argtypes = [C.c_char_p, C.c_void_p]
    L.fp_image_write_png_rgb.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    L.fp_draw_bbox3d.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fp_net_create.restype = C.c_void_p
    L.fp_net_create.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.fp_net_destroy.restype = None
    L.fp_net_destroy.argtypes = [C.c_void_p]
    L.fp_net_blob.restype = C.c_void_p
    L.fp_net_blob.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.fp_net_infer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fp_net_max_batch.argtypes = [C.c_void_p]
    L.fp_mesh_view.restype = C.POINTER(FpMesh)
    L.fp_mesh_view.argtypes = [C.c_void_p]
    L.fp_mesh_vertex_colors.restype = C.c_void_p
    L.fp_mesh_vertex_colors.argtypes = [C.c_void_p]
    vp, ci, cf, cs = C.c_void_p, C.c_int, C.c_float, C.c_char_p
    sigs = {
        "fp_set_inplane_steps": [vp, ci], "fp_num_hypotheses": [vp],
        "fp_register": [vp, vp, vp, vp, ci, ci, cs, ci, vp],
        "fp_track": [vp, vp, vp, ci, ci, vp, cs, ci, vp],
        "fp_register_ex": [vp, vp, vp, vp, ci, ci, ci, cs, ci, vp],
        "fp_track_ex": [vp, vp, vp, ci, ci, ci, vp, cs, ci, vp],
        "fp_track_submit": [vp, vp, vp, ci, ci, ci, vp, cs, ci],
        "fp_track_wait": [vp, vp],
        "fp_track_multi": [vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, vp],
        "fp_upload_frame": [vp, vp, vp, ci, ci, ci], "fp_get_xyz_map": [vp, vp],
        "fp_get_hyp_poses": [vp, vp, ci, vp, vp], "fp_filter_depth": [vp, vp, vp],
        "fp_render_and_transform": [vp, cs, vp, ci, cf, vp, vp, ci],
        "fp_debug_rasterize": [vp, cs, vp, ci, cf, vp, vp],
        "fp_refiner_infer": [vp, vp, vp, ci, ci, vp, vp], "fp_scorer_infer": [vp, vp, vp, ci, ci, vp],
        "fp_refine_post_process": [vp, cs, vp, vp, vp, ci, vp], "fp_argmax": [vp, vp, ci, vp],
        "fp_register_shard_begin": [vp, vp, vp, vp, ci, ci, ci, cs, ci, ci, ci, vp, vp],
        "fp_register_shard_finish": [vp, vp, vp, ci, vp, vp, vp],
        "fp_register_shard_begin_packed": [vp, vp, vp, vp, ci, ci, ci, cs, ci, ci, ci, vp, ci],
        "fp_register_shard_finish_packed": [vp, vp, ci, vp, vp],
        "fp_download": [vp, vp, vp, C.c_size_t],
        "fp_register_sharded": [vp, vp, vp, vp, vp, ci, ci, ci, cs, ci, vp, vp], "fp_device": [vp],
        "fp_profile_enable": [vp, ci], "fp_profile_reset": [vp], "fp_profile_report": [vp, vp, ci],
        "fp_synchronize": [vp], "fp_mesh_orient_bounds": [vp, vp, vp],
        "fp_set_precision": [vp, ci], "fp_get_precision": [vp], "fp_calibrate_fp8": [vp, vp, vp, vp, ci, ci, ci, cs],
        "fp_calibrate": [vp, vp, vp, vp, ci, ci, ci, cs, ci], "fp_calibrate_begin": [vp, ci], "fp_calibrate_add_frame": [vp, vp, vp, vp, ci, ci, ci, cs],
        "fp_calibrate_finish": [vp], "fp_calibrate_abort": [vp], "fp_calibrate_frames": [vp], "fp_get_calibration_blob": [vp, ci, vp, C.c_size_t], "fp_set_calibration_blob": [vp, vp, C.c_size_t],
        "fp_get_calibration": [vp, vp], "fp_set_calibration": [vp, vp], "fp_set_float_model": [vp, ci], "fp_get_float_model": [vp],
        "fp_set_pose_fit": [vp, ci, cf], "fp_get_pose_fit": [vp, vp, vp], "fp_last_track_fit": [vp, vp, ci],
        "fp_last_register_fit": [vp, vp, vp, ci], "fp_pose_fit_eval": [vp, cs, vp, ci, cf, cf, vp],
        "fp_mesh_color_source": [vp], "fp_set_vertex_colors": [vp, cs, vp, ci], "fp_get_color_source": [vp, cs],
        "fp_set_depth_filter": [vp, ci], "fp_get_depth_filter": [vp],
        "fp_render_pose": [vp, cs, vp, cf, vp, ci],
        "fp_render_scene": [vp, ci, vp, vp, cf, vp, vp, ci],
        "fp_pose_errors": [vp, cs, vp, ci, vp, ci, vp, ci, ci, ci, vp],
        "fp_pose_vsd": [vp, cs, vp, ci, vp, ci, cf, vp, ci, ci, vp],
        "fp_refine_depth": [vp, cs, vp, ci, ci, cf, ci, vp, vp],
        "fp_pose_search": [vp, cs, vp, ci, ci, cf, cf, ci, vp],
        "fp_register_depth": [vp, vp, vp, vp, ci, ci, ci, cs, ci, cf, ci, vp, vp],
        "fp_pose_color": [vp, cs, vp, ci, cf, vp],
        "fp_resolve_symmetry": [vp, cs, vp, vp, ci, cf, vp, vp, vp],
        "fp_mask_distance": [vp, vp, ci, vp, vp],
        "fp_pose_silhouette": [vp, cs, vp, ci, vp, ci, cf, ci, ci, vp],
        "fp_refine_silhouette": [vp, cs, vp, ci, vp, ci, ci, ci, cf, ci, vp, vp],
    }
    for name, at in sigs.items():
        f = getattr(L, name)
        f.argtypes = at
        f.restype = C.c_int
    L.fp_calibration_size.argtypes = []
    L.fp_calibration_size.restype = C.c_size_t
    return L


TEST_LIB_PATH = os.environ.get("FP_TEST_LIB_PATH") or os.path.join(_HERE, "libfoundationpose_amd_test.so")  # override: A/B of two builds (tools/)
_TEST_LIB = None


def test_lib() -> C.CDLL:
    """The same sources built with -DFP_TEST_HOOKS: the product plus the fpt_* kernel-level hooks (unit tests of single
    kernels, A/B switches, ablations, stress and debug helpers).  Used by tests/ and tools/ only; nothing in the
    product path loads it."""
    global _TEST_LIB
    if _TEST_LIB is None:
        if not os.path.exists(TEST_LIB_PATH):
            raise RuntimeError(f"{TEST_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _TEST_LIB = _declare(C.CDLL(TEST_LIB_PATH))   # (a superset of the product: the same fp_* signatures)
    return _TEST_LIB


def use_test_lib() -> None:
    """tools/ only: make lib() load the test build (a superset of the product) so that fpt_* switches act on the very
    library instance that runs the pipeline.  Must be called before the first lib()."""
    global LIB_PATH
    assert _LIB is None, "use_test_lib() must come before the first lib()"
    LIB_PATH = TEST_LIB_PATH


def last_error() -> str:
    return (lib().fp_last_error() or b"").decode("utf-8", "replace")
