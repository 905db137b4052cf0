"""Host-side mirror of the reference's operator interface over the C ABI.

`FoundationPose` mirrors detection_6d::Base6DofDetectionModel (reference
detection_6d_foundationpose/include/detection_6d_foundationpose/foundationpose.hpp:16-77): Register / Track with the
same argument meaning and the same error behaviour (False + message instead of bool + glog line), plus the
stage-level operators the reference's orchestrator calls (RenderAndTransform, GetHypPoses, SyncInfer, ...), which
the parity tests drive.  Poses are numpy [4,4] (row-major as numpy prints them); conversion to the ABI's
column-major float[16] happens here.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .synthetic import Mesh, from_colmajor, to_colmajor

FP_HOST, FP_DEVICE = 0, 1
FP_PREC_F16, FP_PREC_BF16, FP_PREC_FP8, FP_PREC_INT8 = 0, 1, 2, 3   # include/foundationpose_amd.h
FP_COLOR_TEXTURE, FP_COLOR_VERTEX = 0, 1
CROP = 160


class FoundationPoseError(RuntimeError):
    pass


@dataclasses.dataclass(frozen=True)
class PoseFit:
    """fp_pose_fit (include/foundationpose_amd.h): pixel counts of one hypothesis' rendered crop against the depth observed under it"""
    n_model: int
    n_observed: int
    n_inlier: int
    n_front: int
    n_behind: int
    sum_dz_q20: int
    mean_dz_m: float
    tol_n: float

    @property
    def inlier_share(self) -> float:
        """inliers per model pixel (0 without a model pixel): low = occluded, gone, or the pose is off the surface"""
        return self.n_inlier / self.n_model if self.n_model else 0.0

    @property
    def front_share(self) -> float:
        return self.n_front / self.n_model if self.n_model else 0.0

    @property
    def behind_share(self) -> float:
        return self.n_behind / self.n_model if self.n_model else 0.0


def _fit(r) -> PoseFit:
    return PoseFit(r.n_model, r.n_observed, r.n_inlier, r.n_front, r.n_behind, r.sum_dz_q20, float(r.mean_dz_m), float(r.tol_n))


@dataclasses.dataclass(frozen=True)
class PoseError:
    """fp_pose_error (include/foundationpose_amd.h): one estimated pose E against ground truth G over the used vertices of the target"""
    add_m: float          # mean_v |E v - G v|
    adds_m: float         # mean_u min_v |G u - E v| (NaN when ADD-S was not asked for)
    mssd_m: float         # min_s max_v |E v - G S_s v|
    mspd_px: float        # min_s max_v |proj(E v) - proj(G S_s v)| (inf: a vertex nearer than 1 cm to the camera plane)
    rot_deg: float        # E against G S_best_sym
    trans_m: float
    best_sym: int         # arg-min of MSSD: 0 = identity, k = the caller's symmetry k - 1
    best_sym_mspd: int    # arg-min of MSPD, -1 when mspd_px is inf
    add_sum_q20: int
    adds_sum_q20: int
    n_vertices: int


def recall(errors, threshold: float) -> float:
    """share of `errors` that are <= threshold (a NaN or inf error never is); 0 for no errors"""
    e = np.asarray(errors, np.float64).ravel()
    return float(np.count_nonzero(e <= threshold)) / e.size if e.size else 0.0


def auc(errors, max_value: float = 0.1, step: float = 0.001) -> float:
    """area under the recall-versus-threshold curve over thresholds 0, step, ..., max_value (trapezoids), normalised to 1: what
    YCB-Video and FoundationPose report for ADD / ADD-S with max_value 0.1 m"""
    n = int(round(max_value / step))
    if n < 1:
        raise ValueError("auc: max_value must be at least one step")
    x = np.linspace(0.0, max_value, n + 1)
    y = np.array([recall(errors, t) for t in x])
    return float(((y[1:] + y[:-1]) / 2 * np.diff(x)).sum() / max_value)


BOP19_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))   # 0.05, 0.10, ..., 0.50: BOP19's misalignment tolerances and its thresholds of correctness
FP_VSD_NORMALIZED = 1
FP_VSD_EST_REFUSED_NEAR, FP_VSD_EST_REFUSED_RANGE, FP_VSD_GT_REFUSED_NEAR, FP_VSD_GT_REFUSED_RANGE = 1, 2, 4, 8


@dataclasses.dataclass(frozen=True)
class PoseVsd:
    """struct fp_pose_vsd (include/foundationpose_amd.h): the surface visible under an estimate against the surface visible under the ground
    truth, given the observed depth; pixel counts of the uploaded frame"""
    n_model_est: int
    n_model_gt: int
    n_visib_est: int
    n_visib_gt: int
    n_inter: int
    n_union: int
    n_fail: tuple         # per tau: intersection pixels whose distances differ by at least the threshold
    vsd: tuple            # per tau: (n_fail + n_union - n_inter) / n_union, 1.0 without a visible pixel
    status: int           # FP_VSD_*_REFUSED_* bits: the pose needs a clipper or leaves the raster's range (all counts 0, vsd 1.0)


def vsd_recall(records, thetas=BOP19_TAUS) -> float:
    """BOP's AR_VSD: the mean over all (record, tau, theta) of vsd[tau] < theta; 0 for no records"""
    v = np.asarray([r.vsd for r in records], np.float64)
    if v.size == 0:
        return 0.0
    return float(np.mean(v[:, :, None] < np.asarray(thetas, np.float64)[None, None, :]))


FP_ICP_TRANSLATION_ONLY = 1
FP_ICP_CONVERGED, FP_ICP_TOO_FEW, FP_ICP_REFUSED_NEAR, FP_ICP_REFUSED_RANGE = 1, 2, 4, 8


@dataclasses.dataclass(frozen=True)
class DepthRefine:
    """struct fp_depth_refine (include/foundationpose_amd.h): how a pose returned by refine_depth fits the uploaded frame's depth, and how
    its refinement went; pixel counts of the frame"""
    n_model: int
    n_valid: int          # model pixels with an observed depth: n_used + n_front + n_behind + n_grazing
    n_used: int
    n_front: int          # something observed more than the gate in front of the model (an occluder)
    n_behind: int
    n_grazing: int
    iterations: int       # updates applied
    rank: int             # directions the last solve moved along (0: none was made)
    status: int           # FP_ICP_CONVERGED | FP_ICP_TOO_FEW | FP_ICP_REFUSED_NEAR | FP_ICP_REFUSED_RANGE
    rms_m: float          # point-to-plane RMS over the used pixels at the returned pose
    cond: float           # lambda_min / lambda_max of the last solve
    last_rot_rad: float
    last_trans_m: float
    sums_q32: tuple       # 28 integers: upper triangle of sum J J^T, sum J e, sum e^2, each term scaled by 2^32


FP_SEARCH_REFUSED_NEAR = 1


@dataclasses.dataclass(frozen=True)
class PoseSearch:
    """struct fp_pose_search (include/foundationpose_amd.h): how the sampled vertices of a pose meet the uploaded frame's depth at the
    best of the pose's steps along the ray of its origin; point counts"""
    n_facing: int         # n_inlier + n_front + n_behind + n_outside + n_missing
    n_inlier: int
    n_front: int          # something observed more than the tolerance in front of the point (an occluder)
    n_behind: int         # the camera saw through where the pose claims a surface
    n_outside: int
    n_missing: int
    score: int            # n_inlier - n_behind - n_outside
    best_step: int        # -1: every step was refused
    n_points: int
    status: int           # FP_SEARCH_REFUSED_NEAR


@dataclasses.dataclass(frozen=True)
class DepthRegister:
    """struct fp_depth_register (include/foundationpose_amd.h): how register_depth found its pose"""
    hypothesis: int       # index into get_hyp_poses of the pose the answer started from
    n_hypotheses: int
    n_candidates: int
    rank_key: int         # n_used - n_behind of the winner
    search: PoseSearch
    refine: DepthRefine


FP_COLOR_MIN_PIXELS = 32
FP_COLOR_REFUSED_NEAR, FP_COLOR_REFUSED_RANGE, FP_COLOR_TOO_FEW, FP_COLOR_FLAT = 1, 2, 4, 8


@dataclasses.dataclass(frozen=True)
class PoseColor:
    """struct fp_pose_color (include/foundationpose_amd.h): how the model's unshaded colour under a pose agrees with the uploaded frame's
    RGB over the visible model pixels; pixel counts of the frame and exact integer sums per channel R, G, B"""
    n_model: int
    n_visible: int        # n_compared + n_nocolor
    n_compared: int
    n_nocolor: int        # visible pixels whose texture coordinate or colour is not a number
    status: int           # FP_COLOR_REFUSED_NEAR | FP_COLOR_REFUSED_RANGE | FP_COLOR_TOO_FEW | FP_COLOR_FLAT
    sum_m: tuple          # the model's values (0..255)
    sum_o: tuple          # the frame's bytes
    sum_mm: tuple
    sum_oo: tuple
    sum_mo: tuple
    zncc: float           # zero-mean normalised cross-correlation, means per channel, one gain; 0 when a status bit is set


def _pose_color(r):
    return PoseColor(r.n_model, r.n_visible, r.n_compared, r.n_nocolor, r.status, tuple(r.sum_m), tuple(r.sum_o), tuple(r.sum_mm), tuple(r.sum_oo),
                     tuple(r.sum_mo), float(r.zncc))


FP_SIL_AMODAL = 1
FP_SIL_D2_NONE = 0x7FFFFFFF
FP_SIL_REFUSED_NEAR, FP_SIL_REFUSED_RANGE, FP_SIL_EMPTY = 1, 2, 4


@dataclasses.dataclass(frozen=True)
class PoseSilhouette:
    """struct fp_pose_silhouette (include/foundationpose_amd.h): how the (visible) silhouette of the model under a pose agrees with a mask
    of the uploaded frame; pixel counts, and exact integer sums of squared pixel distances to the mask's outline"""
    n_model: int
    n_visible: int        # n_inter + n_spill
    n_inter: int          # visible and mask
    n_spill: int          # visible and not mask
    n_mask: int           # the mask pixels of the frame
    n_miss: int           # n_mask - n_inter
    status: int           # FP_SIL_REFUSED_NEAR | FP_SIL_REFUSED_RANGE | FP_SIL_EMPTY
    sum_spill_d2: int     # over the spill pixels: squared distance to the mask, clipped to trunc_px^2 when trunc_px > 0
    sum_miss_d2: int      # over the mask pixels outside the visible model: squared distance to the background, clipped likewise
    iou: float            # n_inter / (n_mask + n_spill)
    rms_spill_px: float
    rms_miss_px: float


def _pose_silhouette(r):
    return PoseSilhouette(r.n_model, r.n_visible, r.n_inter, r.n_spill, r.n_mask, r.n_miss, r.status, r.sum_spill_d2, r.sum_miss_d2, float(r.iou),
                          float(r.rms_spill_px), float(r.rms_miss_px))


FP_SILREF_TRANSLATION_ONLY, FP_SILREF_OCCLUSION = 1, 2
FP_SILREF_CONVERGED, FP_SILREF_TOO_FEW, FP_SILREF_REFUSED_NEAR, FP_SILREF_REFUSED_RANGE = 1, 2, 4, 8


@dataclasses.dataclass(frozen=True)
class SilhouetteRefine:
    """struct fp_silhouette_refine (include/foundationpose_amd.h): how the outline of a pose returned by refine_silhouette lies on the
    mask's outline, and how the iteration ended"""
    n_model: int
    n_contour: int        # n_used + n_occluded + n_far + n_flat + n_steep
    n_used: int
    n_occluded: int
    n_far: int
    n_flat: int
    n_steep: int
    iterations: int       # updates applied
    rank: int
    status: int           # FP_SILREF_CONVERGED | FP_SILREF_TOO_FEW | FP_SILREF_REFUSED_NEAR | FP_SILREF_REFUSED_RANGE
    rms_px: float         # the outline's distance to the mask's outline at the returned pose
    scale_px: float       # the object's radius in pixels there
    cond: float
    last_rot_rad: float
    last_trans_m: float
    sums_q24: tuple


def _silhouette_refine(r):
    return SilhouetteRefine(r.n_model, r.n_contour, r.n_used, r.n_occluded, r.n_far, r.n_flat, r.n_steep, r.iterations, r.rank, r.status, float(r.rms_px),
                            float(r.scale_px), float(r.cond), float(r.last_rot_rad), float(r.last_trans_m), tuple(r.sums_q24))


def _pose_search(r):
    return PoseSearch(r.n_facing, r.n_inlier, r.n_front, r.n_behind, r.n_outside, r.n_missing, r.score, r.best_step, r.n_points, r.status)


def _depth_refine(r):
    return DepthRefine(r.n_model, r.n_valid, r.n_used, r.n_front, r.n_behind, r.n_grazing, r.iterations, r.rank, r.status, float(r.rms_m),
                       float(r.cond), float(r.last_rot_rad), float(r.last_trans_m), tuple(r.sums_q32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_mesh(name: str, mesh_file_path: str) -> Mesh:
    """CreateAssimpMeshLoader(name, path) (mesh_loader.hpp:92-93): OBJ + MTL + PNG through the C ABI.
    Raises FoundationPoseError where the reference throws (empty path, unreadable file, neither UVs nor vertex colours).
    Extra attributes: .orient_bounds [4,4], .dimension [3] (GetOrientBounds / GetObjectDimension).
    .vertex_colors ([V,3] u8, None when the file has none) and .color_source: FP_COLOR_VERTEX for a file without UVs that carries
    per-vertex colours (its texcoords are zero and its texture the grey default), FP_COLOR_TEXTURE otherwise."""
    L = _lib.lib()
    h = L.fp_mesh_load_obj(name.encode(), mesh_file_path.encode())
    if not h:
        raise FoundationPoseError(_lib.last_error())
    try:
        v = L.fp_mesh_view(h).contents
        nv, nf = v.num_vertices, v.num_faces

        def arr(ptr, ctype, shape, dtype):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).astype(dtype).reshape(shape).copy()

        mesh = Mesh(name, arr(v.vertices, C.c_float, (nv, 3), np.float32), arr(v.normals, C.c_float, (nv, 3), np.float32),
                    arr(v.texcoords, C.c_float, (nv, 2), np.float32), arr(v.faces, C.c_uint32, (nf, 3), np.int32),
                    arr(v.texture, C.c_uint8, (v.tex_height, v.tex_width, 3), np.uint8), diameter=float(v.diameter),
                    center=np.array(list(v.center), np.float32))
        ob = np.zeros(16, np.float32)
        dim = np.zeros(3, np.float32)
        L.fp_mesh_orient_bounds(h, _p(ob), _p(dim))
        mesh.orient_bounds = from_colmajor(ob)
        mesh.dimension = dim
        mesh.color_source = L.fp_mesh_color_source(h)
        cp = L.fp_mesh_vertex_colors(h)
        if cp:
            mesh.vertex_colors = arr(cp, C.c_uint8, (nv, 3), np.uint8)
        return mesh
    finally:
        L.fp_mesh_free(h)


class FoundationPose:
    """CreateFoundationPoseModel (foundationpose.hpp:99-105) equivalent."""

    def __init__(self, meshes, K, refiner_weights: str | None = None, scorer_weights: str | None = None,
                 max_input_image_height: int = 1080, max_input_image_width: int = 1920, device: int = -1):
        """device: HIP device the model lives on (-1 = the calling thread's current device); every call switches to it and back."""
        self._L = _lib.lib()
        if isinstance(meshes, Mesh):
            meshes = [meshes]
        self.meshes = {m.name: m for m in meshes}
        self._keep = []
        arr = (_lib.FpMesh * len(meshes))()
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(m.vertices, np.float32)
            n = np.ascontiguousarray(m.normals, np.float32)
            uv = np.ascontiguousarray(m.texcoords[:, :2], np.float32)
            f = np.ascontiguousarray(m.faces, np.uint32)
            tex = np.ascontiguousarray(m.texture, np.uint8)
            self._keep += [v, n, uv, f, tex]
            arr[i].name = m.name.encode()
            arr[i].num_vertices, arr[i].num_faces = len(v), len(f)
            arr[i].vertices, arr[i].normals, arr[i].texcoords = _p(v), _p(n), _p(uv)
            arr[i].faces, arr[i].texture = _p(f), _p(tex)
            arr[i].tex_height, arr[i].tex_width = tex.shape[0], tex.shape[1]
            arr[i].diameter = float(m.diameter)
            arr[i].center = (C.c_float * 3)(*[float(x) for x in m.center])
        self.K = np.ascontiguousarray(K, np.float32)
        h = self._L.fp_create_on(device, C.cast(arr, C.c_void_p), len(meshes), _p(self.K),
                                 refiner_weights.encode() if refiner_weights else None,
                                 scorer_weights.encode() if scorer_weights else None,
                                 max_input_image_height, max_input_image_width)
        if not h:
            raise FoundationPoseError(_lib.last_error())
        self._h = C.c_void_p(h)
        self.last_error = ""
        try:
            for m in meshes:
                if m.color_source == FP_COLOR_VERTEX:   # (a file without UVs: load_mesh)
                    if m.vertex_colors is None:
                        raise FoundationPoseError(f"[FoundationPose] mesh '{m.name}' has the colour source FP_COLOR_VERTEX but no vertex_colors")
                    self.set_vertex_colors(m.name, m.vertex_colors)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None):
            self._L.fp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc) -> bool:
        self.last_error = "" if rc == 0 else _lib.last_error()
        return rc == 0

    def _must(self, rc):
        if not self._ok(rc):
            raise FoundationPoseError(self.last_error)

    # ---- Base6DofDetectionModel -----------------------------------------------------------------
    def Register(self, rgb, depth, mask, target_name: str, refine_itr: int = 1):
        """-> (ok, pose[4,4]).  foundationpose.hpp:36-41."""
        rgb, depth, mask = self._frame(rgb, depth, mask)
        if rgb is None:
            return False, None
        out = np.zeros(16, np.float32)
        ok = self._ok(self._L.fp_register(self._h, _p(rgb), _p(depth), _p(mask), depth.shape[0], depth.shape[1],
                                          target_name.encode(), refine_itr, _p(out)))
        return ok, (from_colmajor(out) if ok else None)

    def register_detailed(self, rgb, depth, mask, target_name: str, refine_itr: int = 1):
        """Register through the two ABI halves (`fp_register_shard_begin` over the whole grid + `fp_register_shard_finish`):
        the same kernels as `Register`, but also hands back what the reference keeps internal (foundationpose.cpp:206-228):
        -> (ok, pose[4,4], winner index, scores[N], refined poses[N,4,4], pooled score features[N,512])."""
        rgb, depth, mask = self._frame(rgb, depth, mask)
        if rgb is None:
            return False, None, -1, None, None, None
        n = self.num_hypotheses
        feat, poses = C.c_void_p(), C.c_void_p()
        if not self._ok(self._L.fp_register_shard_begin(self._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0],
                                                        depth.shape[1], target_name.encode(), refine_itr, 0, n,
                                                        C.byref(feat), C.byref(poses))):
            return False, None, -1, None, None, None
        out = np.zeros(16, np.float32)
        idx = C.c_int(-1)
        scores = np.zeros(n, np.float32)
        if not self._ok(self._L.fp_register_shard_finish(self._h, feat, poses, n, _p(out), C.byref(idx), _p(scores))):
            return False, None, -1, None, None, None
        refined = np.zeros((n, 16), np.float32)
        feats = np.zeros((n, 512), np.float32)
        # (fp_download: a copy ordered on the model's own stream -- loading a second HIP runtime through ctypes would not even
        # share stream handles with the library's, and the legacy stream is off limits while any thread captures a hipGraph)
        self._must(self._L.fp_download(self._h, _p(refined), poses, refined.nbytes))
        self._must(self._L.fp_download(self._h, _p(feats), feat, feats.nbytes))
        return True, from_colmajor(out), idx.value, scores, from_colmajor(refined), feats

    def Track(self, rgb, depth, hyp_pose, target_name: str, refine_itr: int = 1):
        """-> (ok, pose[4,4]).  foundationpose.hpp:59-64."""
        rgb, depth, _ = self._frame(rgb, depth, None)
        if rgb is None:
            return False, None
        hyp = to_colmajor(np.asarray(hyp_pose, np.float32))
        out = np.zeros(16, np.float32)
        ok = self._ok(self._L.fp_track(self._h, _p(rgb), _p(depth), depth.shape[0], depth.shape[1], _p(hyp),
                                       target_name.encode(), refine_itr, _p(out)))
        return ok, (from_colmajor(out) if ok else None)

    def track_submit(self, rgb, depth, hyp_pose, target_name: str, refine_itr: int = 1) -> bool:
        """Enqueue a Track (frame upload + refinement) on this model's stream and return; `track_wait` fetches the pose.
        One host thread can keep several models (objects) in flight this way.  The frame arrays are kept alive until the wait."""
        rgb, depth, _ = self._frame(rgb, depth, None)
        if rgb is None:
            return False
        hyp = to_colmajor(np.asarray(hyp_pose, np.float32))
        self._pending_frame = (rgb, depth)
        return self._ok(self._L.fp_track_submit(self._h, _p(rgb), _p(depth), FP_HOST, depth.shape[0], depth.shape[1], _p(hyp),
                                                target_name.encode(), refine_itr))

    def track_wait(self):
        """-> (ok, pose[4,4]) of the last `track_submit`."""
        out = np.zeros(16, np.float32)
        ok = self._ok(self._L.fp_track_wait(self._h, _p(out)))
        self._pending_frame = None
        return ok, (from_colmajor(out) if ok else None)

    def track_multi(self, rgb, depth, hyp_poses, target_names, refine_itr: int = 1):
        """Track of K objects of one frame as one batch -> (ok, poses[K,4,4])."""
        rgb, depth, _ = self._frame(rgb, depth, None)
        if rgb is None:
            return False, None
        hyp = to_colmajor(np.asarray(hyp_poses, np.float32))
        K = len(hyp)
        names = (C.c_char_p * K)(*[n.encode() for n in target_names])
        out = np.zeros((K, 16), np.float32)
        ok = self._ok(self._L.fp_track_multi(self._h, _p(rgb), _p(depth), FP_HOST, depth.shape[0], depth.shape[1], K, _p(hyp),
                                             C.cast(names, C.c_void_p), refine_itr, _p(out)))
        return ok, (from_colmajor(out) if ok else None)

    def _frame(self, rgb, depth, mask):
        # CheckInputArguments (foundationpose.cpp:155-179): sizes must agree
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
        if rgb.shape[:2] != depth.shape or (mask is not None and mask.shape != depth.shape):
            self.last_error = "[FoundationPose] Got rgb/depth/mask with different size!"
            return None, None, None
        self._hw = depth.shape   # (the size of the frame the call hands to the library: render_pose sizes its outputs by it)
        return rgb, depth, mask

    # ---- stage-level operators -------------------------------------------------------------------
    def set_inplane_steps(self, steps: int):
        self._must(self._L.fp_set_inplane_steps(self._h, steps))

    @property
    def num_hypotheses(self) -> int:
        return self._L.fp_num_hypotheses(self._h)

    def upload_frame(self, rgb, depth):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        self._frame_keep = (rgb, depth)
        self._must(self._L.fp_upload_frame(self._h, _p(rgb), _p(depth), FP_HOST, depth.shape[0], depth.shape[1]))
        self._must(self._L.fp_synchronize(self._h))
        self._hw = depth.shape

    def xyz_map(self):
        out = np.zeros(self._hw + (3,), np.float32)
        self._must(self._L.fp_get_xyz_map(self._h, _p(out)))
        return out

    def filter_depth(self):
        e = np.zeros(self._hw, np.float32)
        b = np.zeros(self._hw, np.float32)
        self._must(self._L.fp_filter_depth(self._h, _p(e), _p(b)))
        return e, b

    def get_hyp_poses(self, mask):
        """FoundationPoseSampler::GetHypPoses -> [N,4,4] or None (False in the reference) on failure."""
        mask = np.ascontiguousarray(mask, np.uint8)
        out = np.zeros((self.num_hypotheses, 16), np.float32)
        n = C.c_int(0)
        if not self._ok(self._L.fp_get_hyp_poses(self._h, _p(mask), FP_HOST, _p(out), C.byref(n))):
            return None
        return from_colmajor(out[:n.value])

    def render_and_transform(self, target_name, poses, crop_ratio):
        """FoundationPoseRenderer::RenderAndTransform -> (render_input, transf_input), each [N,160,160,6] f32."""
        p = to_colmajor(np.asarray(poses, np.float32))
        N = len(p)
        a = np.zeros((N, CROP, CROP, 6), np.float32)
        b = np.zeros((N, CROP, CROP, 6), np.float32)
        self._must(self._L.fp_render_and_transform(self._h, target_name.encode(), _p(p), N, crop_ratio, _p(a), _p(b),
                                                   FP_HOST))
        return a, b

    def debug_rasterize(self, target_name, poses, crop_ratio):
        p = to_colmajor(np.asarray(poses, np.float32))
        N = len(p)
        tri = np.zeros((N, CROP, CROP), np.int32)
        rast = np.zeros((N, CROP, CROP, 4), np.float32)
        self._must(self._L.fp_debug_rasterize(self._h, target_name.encode(), _p(p), N, crop_ratio, _p(tri), _p(rast)))
        return tri, rast

    def refiner_infer(self, render_input, transf_input):
        a = np.ascontiguousarray(render_input, np.float32)
        b = np.ascontiguousarray(transf_input, np.float32)
        N = len(a)
        t = np.zeros((N, 3), np.float32)
        r = np.zeros((N, 3), np.float32)
        self._must(self._L.fp_refiner_infer(self._h, _p(a), _p(b), FP_HOST, N, _p(t), _p(r)))
        return t, r

    def scorer_infer(self, render_input, transf_input):
        a = np.ascontiguousarray(render_input, np.float32)
        b = np.ascontiguousarray(transf_input, np.float32)
        N = len(a)
        s = np.zeros(N, np.float32)
        self._must(self._L.fp_scorer_infer(self._h, _p(a), _p(b), FP_HOST, N, _p(s)))
        return s

    def refine_post_process(self, target_name, poses, trans, rot):
        p = to_colmajor(np.asarray(poses, np.float32))
        t = np.ascontiguousarray(trans, np.float32)
        r = np.ascontiguousarray(rot, np.float32)
        out = np.zeros_like(p)
        self._must(self._L.fp_refine_post_process(self._h, target_name.encode(), _p(p), _p(t), _p(r), len(p), _p(out)))
        return from_colmajor(out)

    def argmax(self, scores) -> int:
        s = np.ascontiguousarray(scores, np.float32).ravel()
        idx = C.c_int(-1)
        self._must(self._L.fp_argmax(self._h, _p(s), len(s), C.byref(idx)))
        return idx.value

    # ---- pose fit (include/foundationpose_amd.h "pose fit") --------------------------------------
    def set_pose_fit(self, on: bool, tol_m: float = 0.005):
        """Track / Register also report how well the depth under the pose agrees with the model (default off); tol_m in metres."""
        self._must(self._L.fp_set_pose_fit(self._h, 1 if on else 0, tol_m))

    @property
    def pose_fit_config(self):
        """-> (on, tol_m)"""
        on, tol = C.c_int(0), C.c_float(0)
        self._must(self._L.fp_get_pose_fit(self._h, C.byref(on), C.byref(tol)))
        return bool(on.value), tol.value

    def last_track_fit(self, K: int = 1):
        """records of the last Track (one) / track_multi (K): each describes the pose the last refine iteration STARTED from"""
        out = (_lib.FpPoseFit * K)()
        self._must(self._L.fp_last_track_fit(self._h, out, K))
        return [_fit(r) for r in out]

    def last_register_fit(self, all_hypotheses: bool = False):
        """-> the winner's record, or (winner, [record per hypothesis]) of the last Register: the FINAL poses at crop ratio 1.1"""
        win = _lib.FpPoseFit()
        n = self.num_hypotheses if all_hypotheses else 0
        every = (_lib.FpPoseFit * max(n, 1))()
        self._must(self._L.fp_last_register_fit(self._h, C.byref(win), every if all_hypotheses else None, n))
        return (_fit(win), [_fit(r) for r in every]) if all_hypotheses else _fit(win)

    def pose_fit(self, target_name: str, poses, crop_ratio: float = 1.2, tol_m: float = 0.005):
        """records of any poses [N,4,4] on the uploaded frame (stage operator; the option need not be on)"""
        p = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        out = (_lib.FpPoseFit * len(p))()
        self._must(self._L.fp_pose_fit_eval(self._h, target_name.encode(), _p(p), len(p), crop_ratio, tol_m, out))
        return [_fit(r) for r in out]

    def _render_outputs(self, table: dict, record, fn: str, want):
        """what render_pose and render_scene begin with -> ({name: zeroed array of the uploaded frame's size}, the ctypes record of their
        addresses) for the names in `want`, all of which `table` ({name: (dtype, trailing shape)}) must know"""
        hw = getattr(self, "_hw", None)
        if hw is None:
            self.last_error = f"[FoundationPose] fp_{fn}: no frame uploaded"
            raise FoundationPoseError(self.last_error)
        unknown = [n for n in want if n not in table]
        if unknown:
            raise FoundationPoseError(f"[FoundationPose] {fn}: unknown outputs {unknown}")
        out = {n: np.zeros(tuple(hw) + table[n][1], table[n][0]) for n in want}
        return out, record(**{n: _p(a) for n, a in out.items()})

    # ---- a pose at frame resolution (include/foundationpose_amd.h "a pose at frame resolution") ----
    RENDER_OUTPUTS = {"model_depth": (np.float32, ()), "model_mask": (np.uint8, ()), "visible_mask": (np.uint8, ()),
                      "tri_id": (np.int32, ()), "overlay": (np.uint8, (3,))}

    def render_pose(self, target_name: str, pose, tol_m: float = 0.005,
                    want=("model_depth", "model_mask", "visible_mask", "tri_id", "overlay")) -> dict:
        """fp_render_pose: the target under `pose` ([4,4], what Register / Track return) rasterised at the size of the uploaded frame
        -> {name: array} for the names in `want`: model_depth [H,W] f32 (0 = background), model_mask / visible_mask [H,W] u8 (255 / 0),
        tri_id [H,W] i32 (triangle + 1), overlay [H,W,3] u8.  A model pixel is visible unless the RAW observed depth is valid and more
        than tol_m in front of it.  Raises FoundationPoseError for a pose that would need clipping (a vertex nearer than 1 cm)."""
        out, rec = self._render_outputs(self.RENDER_OUTPUTS, _lib.FpFrameRender, "render_pose", want)
        p = to_colmajor(np.asarray(pose, np.float32).reshape(4, 4))
        self._must(self._L.fp_render_pose(self._h, target_name.encode(), _p(p), tol_m, C.byref(rec), FP_HOST))
        return out

    # ---- all tracked objects at frame resolution (include/foundationpose_amd.h "all tracked objects of a frame") ----
    SCENE_OUTPUTS = {"model_depth": (np.float32, ()), "instance_id": (np.uint8, ()), "visible_mask": (np.uint8, ()),
                     "tri_id": (np.int32, ()), "cover_bits": (np.uint64, ()), "overlay": (np.uint8, (3,))}
    SCENE_RECORD = np.dtype([("n_covered", np.int32), ("n_front", np.int32), ("n_hidden", np.int32), ("n_visible", np.int32),
                             ("n_occluded", np.int32), ("reserved", np.int32, (3,))])

    def render_scene(self, target_names, poses, tol_m: float = 0.005,
                     want=("model_depth", "instance_id", "visible_mask", "tri_id", "cover_bits", "overlay"), records: bool = True):
        """fp_render_scene: the K targets `target_names` under `poses` ([K,4,4], what track_multi returns) rasterised into ONE picture of
        the uploaded frame's size -> ({name: array} for the names in `want`, records).  instance_id [H,W] u8 is the object index + 1 of
        the nearest model surface, tri_id the triangle + 1 within that object's mesh, cover_bits [H,W] u64 has bit o set where object
        o's own silhouette covers the pixel, the overlay draws object o in tint o % 8.  records (None when `records` is false): a
        structured array [K] of SCENE_RECORD -- n_covered, n_front, n_hidden (behind another object of the call), n_visible,
        n_occluded (behind something observed).  Raises FoundationPoseError when any object's pose would need clipping."""
        out, rec = self._render_outputs(self.SCENE_OUTPUTS, _lib.FpSceneRender, "render_scene", want)
        names = [n.encode() for n in target_names]
        p = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        if len(p) != len(names):
            raise FoundationPoseError(f"[FoundationPose] render_scene: {len(names)} names but {len(p)} poses")
        recs = np.zeros(max(len(names), 1), self.SCENE_RECORD) if records else None
        arr = (C.c_char_p * max(len(names), 1))(*names)
        self._must(self._L.fp_render_scene(self._h, len(names), arr, _p(p), tol_m, C.byref(rec), _p(recs) if records else None, FP_HOST))
        return out, (recs[:len(names)] if records else None)

    # ---- pose errors (include/foundationpose_amd.h "pose errors") ----------------------------------
    def pose_errors(self, target_name: str, est_poses, gt_poses, symmetries=None, vertex_step: int = 1, adds: bool = True):
        """fp_pose_errors: ADD, ADD-S, MSSD and MSPD of est_poses [N,4,4] against gt_poses ([N,4,4], or one [4,4] for all of them: every
        hypothesis of a Register against one truth) -> [PoseError] * N.  symmetries: [S,4,4] in the MESH frame (BOP's models_info.json,
        already discretised), None = none; the identity is always symmetry 0 of best_sym.  vertex_step: use every vertex_step-th vertex.
        adds=False skips the Vs^2 nearest-neighbour part (adds_m is NaN then).  Needs no frame."""
        e = to_colmajor(np.asarray(est_poses, np.float32).reshape(-1, 4, 4))
        g = to_colmajor(np.asarray(gt_poses, np.float32).reshape(-1, 4, 4))
        s = None if symmetries is None or len(symmetries) == 0 else to_colmajor(np.asarray(symmetries, np.float32).reshape(-1, 4, 4))
        out = (_lib.FpPoseError * max(len(e), 1))()
        self._must(self._L.fp_pose_errors(self._h, target_name.encode(), _p(e), len(e), _p(g), len(g), _p(s), 0 if s is None else len(s),
                                          int(vertex_step), 1 if adds else 0, out))
        return [PoseError(float(r.add_m), float(r.adds_m), float(r.mssd_m), float(r.mspd_px), float(r.rot_deg), float(r.trans_m), r.best_sym,
                          r.best_sym_mspd, r.add_sum_q20, r.adds_sum_q20, r.n_vertices) for r in out[:len(e)]]

    # ---- visible surface discrepancy (include/foundationpose_amd.h "visible surface discrepancy") ---
    def pose_vsd(self, target_name: str, est_poses, gt_poses, delta_m: float = 0.015, taus=BOP19_TAUS, normalized: bool = True):
        """fp_pose_vsd: BOP's VSD of est_poses [N,4,4] against gt_poses ([N,4,4], or one [4,4] for all of them) on the uploaded frame's
        raw depth -> [PoseVsd] * N.  delta_m: the visibility tolerance; taus: up to 16 misalignment tolerances, fractions of the target's
        diameter when `normalized` (BOP19) and metres otherwise.  A pose that would need a clipper does not fail the call: its record
        carries the status bit and vsd 1.0 (one ground truth for all that does fails it)."""
        e = to_colmajor(np.asarray(est_poses, np.float32).reshape(-1, 4, 4))
        g = to_colmajor(np.asarray(gt_poses, np.float32).reshape(-1, 4, 4))
        t = np.ascontiguousarray(np.asarray(taus, np.float32).ravel())
        out = (_lib.FpPoseVsd * max(len(e), 1))()
        self._must(self._L.fp_pose_vsd(self._h, target_name.encode(), _p(e), len(e), _p(g), len(g), delta_m, _p(t), len(t),
                                       FP_VSD_NORMALIZED if normalized else 0, out))
        n = min(len(t), _lib.FP_VSD_MAX_TAUS)
        return [PoseVsd(r.n_model_est, r.n_model_gt, r.n_visib_est, r.n_visib_gt, r.n_inter, r.n_union, tuple(r.n_fail[:n]),
                        tuple(float(x) for x in r.vsd[:n]), r.status) for r in out[:len(e)]]

    # ---- depth refinement (include/foundationpose_amd.h "depth refinement") --------------------------
    def refine_depth(self, target_name: str, poses, iterations: int = 10, max_dist_m: float = 0.02, translation_only: bool = False):
        """fp_refine_depth: projective point-to-plane ICP of poses [N,4,4] on the uploaded frame's raw depth -> (poses [N,4,4] f32,
        [DepthRefine] * N).  max_dist_m: the gate along the ray, at most the target's diameter; translation_only: leave the rotation alone
        (a symmetric object's rotation about its axis would follow the noise).  iterations = 0 only measures the fit.  A pose that would
        need a clipper does not fail the call: it comes back unchanged with its status bit."""
        e = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        out_p = np.zeros_like(e)
        out = (_lib.FpDepthRefine * max(len(e), 1))()
        self._must(self._L.fp_refine_depth(self._h, target_name.encode(), _p(e), len(e), iterations, max_dist_m,
                                           FP_ICP_TRANSLATION_ONLY if translation_only else 0, _p(out_p), out))
        return from_colmajor(out_p), [_depth_refine(r) for r in out[:len(e)]]

    # ---- depth search and the Register built on it (include/foundationpose_amd.h "depth search") ----
    def pose_search(self, target_name: str, poses, n_steps: int = 9, step_m: float = None, tol_m: float = 0.005, vertex_step: int = 1):
        """fp_pose_search: poses [N,4,4] against the uploaded frame's raw depth -> [PoseSearch] * N.  Every pose is tried at n_steps pushes
        of step_m (default: the target's diameter / 16) along the ray of its origin; the record is that of its best step.  vertex_step:
        every vertex_step-th vertex is used, at most FP_SEARCH_MAX_POINTS of them."""
        e = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        if step_m is None:
            step_m = float(np.float32(self.meshes[target_name].diameter) / np.float32(16)) if target_name in self.meshes else 0.0
        out = (_lib.FpPoseSearch * max(len(e), 1))()
        self._must(self._L.fp_pose_search(self._h, target_name.encode(), _p(e), len(e), n_steps, step_m, tol_m, vertex_step, out))
        return [_pose_search(r) for r in out[:len(e)]]

    def register_depth(self, rgb, depth, mask, target_name: str, top_k: int = 16, tol_m: float = 0.005, icp_iterations: int = 15):
        """fp_register_depth: Register without weights -> (ok, pose [4,4], DepthRegister).  The hypothesis grid (set_inplane_steps) is ranked
        by pose_search on the depth alone, the top_k candidates are refined by refine_depth, and the one that explains most of the depth
        wins.  The frame stays uploaded.  A symmetric object's answer is one of its equivalent poses."""
        rgb, depth, mask = self._frame(rgb, depth, mask)
        if rgb is None:
            return False, None, None
        self._frame_keep = (rgb, depth)
        out = np.zeros(16, np.float32)
        rec = _lib.FpDepthRegister()
        ok = self._ok(self._L.fp_register_depth(self._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1], target_name.encode(),
                                                top_k, tol_m, icp_iterations, _p(out), C.byref(rec)))
        if not ok:
            return False, None, None
        return True, from_colmajor(out), DepthRegister(rec.hypothesis, rec.n_hypotheses, rec.n_candidates, rec.rank_key, _pose_search(rec.search),
                                                       _depth_refine(rec.refine))

    # ---- colour agreement and symmetry resolution (include/foundationpose_amd.h "colour agreement") --
    def pose_color(self, target_name: str, poses, tol_m: float = 0.005):
        """fp_pose_color: the model's unshaded colour (texture, or vertex colours after set_vertex_colors) under poses [N,4,4] against the
        uploaded frame's RGB over the visible model pixels -> [PoseColor] * N.  tol_m: the occlusion tolerance of render_pose.  A pose
        that would need a clipper does not fail the call: its record carries the status bit and zncc 0."""
        e = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        out = (_lib.FpPoseColor * max(len(e), 1))()
        self._must(self._L.fp_pose_color(self._h, target_name.encode(), _p(e), len(e), tol_m, out))
        return [_pose_color(r) for r in out[:len(e)]]

    def resolve_symmetry(self, target_name: str, pose, symmetries, tol_m: float = 0.005):
        """fp_resolve_symmetry: of the equivalents pose * S_s of a symmetric object's pose [4,4] the one the picture shows -> (pose [4,4],
        best_sym, [PoseColor] * (S + 1)).  symmetries: [S,4,4] in the MESH frame as for pose_errors (None = none); the identity is always
        symmetry 0.  Raises when no equivalent has a usable record (an untextured model)."""
        e = to_colmajor(np.asarray(pose, np.float32).reshape(4, 4))
        s = None if symmetries is None or len(symmetries) == 0 else to_colmajor(np.asarray(symmetries, np.float32).reshape(-1, 4, 4))
        n = 0 if s is None else len(s)
        out_p = np.zeros(16, np.float32)
        best = C.c_int(-1)
        recs = (_lib.FpPoseColor * (n + 1))()
        self._must(self._L.fp_resolve_symmetry(self._h, target_name.encode(), _p(e), _p(s), n, tol_m, _p(out_p), C.byref(best), recs))
        return from_colmajor(out_p), best.value, [_pose_color(r) for r in recs]

    # ---- silhouette agreement (include/foundationpose_amd.h "silhouette agreement") ----------------
    def _frame_mask(self, fn: str, mask):
        """the u8 mask of a call, which must have the uploaded frame's size (the library cannot know the size of what it is handed)"""
        mask = np.ascontiguousarray(mask, np.uint8)
        hw = getattr(self, "_hw", None)
        if hw is None or mask.shape != tuple(hw):
            self.last_error = f"[FoundationPose] {fn}: " + ("no frame uploaded" if hw is None else f"a mask of shape {mask.shape}, the uploaded frame is {tuple(hw)}")
            raise FoundationPoseError(self.last_error)
        return mask

    def mask_distance(self, mask):
        """fp_mask_distance: the exact squared Euclidean distance transform of a mask [H,W] (a mask pixel: byte > 0) of the uploaded frame's
        size -> (d2_to_mask, d2_to_bg) [H,W] u32: per pixel the squared distance in pixels to the nearest mask pixel / to the nearest other
        pixel, FP_SIL_D2_NONE where there is none."""
        mask = self._frame_mask("fp_mask_distance", mask)
        a, b = np.zeros(mask.shape, np.uint32), np.zeros(mask.shape, np.uint32)
        self._must(self._L.fp_mask_distance(self._h, _p(mask), FP_HOST, _p(a), _p(b)))
        return a, b

    def pose_silhouette(self, target_name: str, mask, poses, tol_m: float = 0.005, trunc_px: int = 0, amodal: bool = False):
        """fp_pose_silhouette: the visible silhouette of the model under poses [N,4,4] against a mask [H,W] u8 of the uploaded frame ->
        [PoseSilhouette] * N.  tol_m: the occlusion tolerance of render_pose; trunc_px > 0 clips every squared distance to trunc_px^2;
        amodal: every model pixel counts as visible and the depth is not read.  A pose that would need a clipper does not fail the call:
        its record carries the status bit and nothing else."""
        mask = self._frame_mask("fp_pose_silhouette", mask)
        e = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        out = (_lib.FpPoseSilhouette * max(len(e), 1))()
        self._must(self._L.fp_pose_silhouette(self._h, target_name.encode(), _p(mask), FP_HOST, _p(e), len(e), tol_m, int(trunc_px),
                                              FP_SIL_AMODAL if amodal else 0, out))
        return [_pose_silhouette(r) for r in out[:len(e)]]

    def refine_silhouette(self, target_name: str, mask, poses, iterations: int = 15, gate_px: int = 0, tol_m: float = 0.005,
                          translation_only: bool = False, occlusion: bool = False):
        """fp_refine_silhouette: poses [N,4,4] moved until the model's outline lies on the outline of mask [H,W] u8 of the uploaded frame
        -> (poses [N,4,4] f32, [SilhouetteRefine] * N).  No depth is read unless occlusion is set (then the outline pixels render_pose
        would call occluded at tol_m are dropped).  gate_px > 0 drops outline pixels farther than that from the mask's outline;
        translation_only leaves the rotation alone (an outline that a rotation does not move cannot determine it).  iterations = 0 only
        measures.  A pose that would need a clipper does not fail the call: it comes back unchanged with its status bit."""
        mask = self._frame_mask("fp_refine_silhouette", mask)
        e = to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
        out_p = np.zeros_like(e)
        out = (_lib.FpSilhouetteRefine * max(len(e), 1))()
        flags = (FP_SILREF_TRANSLATION_ONLY if translation_only else 0) | (FP_SILREF_OCCLUSION if occlusion else 0)
        self._must(self._L.fp_refine_silhouette(self._h, target_name.encode(), _p(mask), FP_HOST, _p(e), len(e), int(iterations), int(gate_px), tol_m,
                                                flags, _p(out_p), out))
        return from_colmajor(out_p), [_silhouette_refine(r) for r in out[:len(e)]]

    # ---- depth filter (include/foundationpose_amd.h "depth filter") --------------------------------
    def set_depth_filter(self, on: bool):
        """Register, Track and the stage operators read bilateral(erode(depth)) instead of the depth itself, like FoundationPose as
        published (default off).  Depth below 0.1 m reads as missing then.  Drops the captured graphs like set_pose_fit."""
        self._must(self._L.fp_set_depth_filter(self._h, 1 if on else 0))

    def depth_filter(self) -> bool:
        on = self._L.fp_get_depth_filter(self._h)
        self._must(1 if on < 0 else 0)
        return bool(on)

    # ---- vertex colours (include/foundationpose_amd.h "vertex colours") ----------------------------
    def set_vertex_colors(self, target_name: str, colors):
        """colors [V,3] u8 RGB become the colour source of the target's renderings (interpolated per pixel instead of a texture
        sample); None returns the target to its texture.  Drops the captured graphs like set_pose_fit."""
        if colors is None:
            self._must(self._L.fp_set_vertex_colors(self._h, target_name.encode(), None, 0))
            return
        c = np.ascontiguousarray(colors, np.uint8)
        if c.ndim != 2 or c.shape[1] != 3:
            raise FoundationPoseError("[FoundationPose] set_vertex_colors: colors must be [V,3] u8")
        self._must(self._L.fp_set_vertex_colors(self._h, target_name.encode(), _p(c), len(c)))

    def color_source(self, target_name: str) -> int:
        """FP_COLOR_TEXTURE / FP_COLOR_VERTEX of a target"""
        rc = self._L.fp_get_color_source(self._h, target_name.encode())
        if rc < 0:
            self.last_error = _lib.last_error()
            raise FoundationPoseError(self.last_error)
        return rc

    # ---- float model of the rendering stage (1 = contracted like nvcc -fmad=true, default; 0 = separate roundings) ----
    def set_float_model(self, fmad: int):
        self._must(self._L.fp_set_float_model(self._h, int(fmad)))

    @property
    def device(self) -> int:
        return self._L.fp_device(self._h)

    @property
    def float_model(self) -> int:
        return self._L.fp_get_float_model(self._h)

    # ---- network precision (include/foundationpose_amd.h "network precision") ---------------------
    def set_precision(self, precision: int):
        """FP_PREC_F16 (the reference's TensorRT --fp16 engines, default) / FP_PREC_BF16 / FP_PREC_FP8, FP_PREC_INT8 (after calibrate)."""
        self._must(self._L.fp_set_precision(self._h, precision))

    @property
    def precision(self) -> int:
        return self._L.fp_get_precision(self._h)

    def calibrate(self, rgb, depth, mask, target_name: str, precision: int = FP_PREC_INT8):
        """Post-training quantisation of the 8-bit precision on one frame: f16 statistics -> per-channel scales -> bias correction."""
        rgb, depth, mask = self._frame(rgb, depth, mask)
        if rgb is None:
            raise FoundationPoseError(self.last_error)
        self._must(self._L.fp_calibrate(self._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1],
                                        target_name.encode(), precision))

    def calibrate_frames(self, frames, target_name: str, precision: int = FP_PREC_INT8):
        """Post-training quantisation over several frames (fp_calibrate_begin / _add_frame / _finish): `frames` = iterable of
        (rgb, depth, mask) or of objects with .rgb / .depth / .mask.  K >= 8 frames of the deployment's scene family make the
        common-mode part of the correction carry over to frames the calibration never saw."""
        self._must(self._L.fp_calibrate_begin(self._h, precision))
        try:
            for f in frames:
                rgb, depth, mask = (f.rgb, f.depth, f.mask) if hasattr(f, "rgb") else f
                rgb, depth, mask = self._frame(rgb, depth, mask)
                if rgb is None:
                    raise FoundationPoseError(self.last_error)
                self._must(self._L.fp_calibrate_add_frame(self._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1],
                                                          target_name.encode()))
        except Exception:
            self._L.fp_calibrate_abort(self._h)
            raise
        self._must(self._L.fp_calibrate_finish(self._h))

    def calibrate_fp8(self, rgb, depth, mask, target_name: str):
        self.calibrate(rgb, depth, mask, target_name, FP_PREC_FP8)

    def get_calibration_blob(self, precision: int) -> bytes:
        n = self._L.fp_calibration_size()
        buf = np.zeros(n, np.uint8)
        self._must(self._L.fp_get_calibration_blob(self._h, precision, _p(buf), n))
        return buf.tobytes()

    def set_calibration_blob(self, blob: bytes):
        buf = np.frombuffer(blob, np.uint8).copy()
        self._must(self._L.fp_set_calibration_blob(self._h, _p(buf), buf.size))

    def get_calibration(self):
        out = np.zeros(32, np.float32)
        self._must(self._L.fp_get_calibration(self._h, _p(out)))
        return out

    def set_calibration(self, amax):
        a = np.ascontiguousarray(amax, np.float32)
        assert a.size == 32
        self._must(self._L.fp_set_calibration(self._h, _p(a)))

    # ---- measurement -----------------------------------------------------------------------------
    def profile(self, on: bool):
        self._must(self._L.fp_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._must(self._L.fp_profile_reset(self._h))

    def profile_report(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        self._must(self._L.fp_profile_report(self._h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms, flops, nbytes = line.split()
            out[name] = dict(calls=int(calls), ms=float(ms), flops=float(flops), bytes=float(nbytes))
        return out

    def synchronize(self):
        self._must(self._L.fp_synchronize(self._h))

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return self._L.fp_stream(self._h)
