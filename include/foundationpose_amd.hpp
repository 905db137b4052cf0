// foundationpose_amd.hpp -- dependency-free C++17 RAII wrapper over the C ABI (foundationpose_amd.h).
// Mirrors detection_6d::Base6DofDetectionModel (reference detection_6d_foundationpose/include/
// detection_6d_foundationpose/foundationpose.hpp:16-77) with plain structs instead of cv::Mat / Eigen types, so it
// builds where OpenCV and Eigen do not exist (the MI355X image).  detection_6d_foundationpose_amd.hpp layers the
// reference's exact signatures on top when those headers are present.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "foundationpose_amd.h"

namespace fp_amd {

using Pose = std::array<float, 16>;  // column-major 4x4 (Eigen::Matrix4f::data())

struct ImageU8 { const uint8_t *data; int rows, cols, channels; };
struct ImageF32 { const float *data; int rows, cols; };

struct Mesh {  // what BaseMeshLoader's getters return (mesh_loader.hpp:25-61)
  std::string name;
  std::vector<float> vertices, normals, texcoords;  // [V,3], [V,3], [V,2]
  std::vector<uint32_t> faces;                      // [F,3]
  std::vector<uint8_t> texture;                     // [TH,TW,3] RGB
  int tex_height = 0, tex_width = 0;
  float diameter = 0;
  float center[3] = {0, 0, 0};
  // new; the reference has no counterpart: per-vertex colours [V,3] RGB (empty: the file had none) and the colour source
  // (FP_COLOR_TEXTURE / FP_COLOR_VERTEX: a file without UVs that carries colours; its texcoords are zero, its texture the grey default)
  std::vector<uint8_t> vertex_colors;
  int color_source = FP_COLOR_TEXTURE;
};

// CreateAssimpMeshLoader(name, path) equivalent (mesh_loader.hpp:92-93): OBJ + MTL + PNG; throws like the reference
inline Mesh LoadObjMesh(const std::string &name, const std::string &mesh_file_path, float *orient_bounds16 = nullptr,
                        float *dimension3 = nullptr) {
  fp_loaded_mesh *h = fp_mesh_load_obj(name.c_str(), mesh_file_path.c_str());
  if (!h) throw std::runtime_error(fp_last_error());
  const fp_mesh *v = fp_mesh_view(h);
  Mesh m;
  m.name = name;
  m.vertices.assign(v->vertices, v->vertices + (size_t)v->num_vertices * 3);
  m.normals.assign(v->normals, v->normals + (size_t)v->num_vertices * 3);
  m.texcoords.assign(v->texcoords, v->texcoords + (size_t)v->num_vertices * 2);
  m.faces.assign(v->faces, v->faces + (size_t)v->num_faces * 3);
  m.texture.assign(v->texture, v->texture + (size_t)v->tex_height * v->tex_width * 3);
  m.tex_height = v->tex_height; m.tex_width = v->tex_width; m.diameter = v->diameter;
  for (int k = 0; k < 3; k++) m.center[k] = v->center[k];
  m.color_source = fp_mesh_color_source(h);
  if (const uint8_t *c = fp_mesh_vertex_colors(h)) m.vertex_colors.assign(c, c + (size_t)v->num_vertices * 3);
  fp_mesh_orient_bounds(h, orient_bounds16, dimension3);
  fp_mesh_free(h);
  return m;
}

class FoundationPose {
public:
  // CreateFoundationPoseModel (foundationpose.hpp:99-105); throws std::runtime_error like the reference constructor
  FoundationPose(const std::vector<Mesh> &meshes, const float K[9], const std::string &refiner_weights,
                 const std::string &scorer_weights, int max_h = 1080, int max_w = 1920) {
    std::vector<fp_mesh> cm(meshes.size());
    for (size_t i = 0; i < meshes.size(); i++) {
      const Mesh &m = meshes[i];
      cm[i].name = m.name.c_str();
      cm[i].num_vertices = (int)(m.vertices.size() / 3);
      cm[i].num_faces = (int)(m.faces.size() / 3);
      cm[i].vertices = m.vertices.data(); cm[i].normals = m.normals.data(); cm[i].texcoords = m.texcoords.data();
      cm[i].faces = m.faces.data(); cm[i].texture = m.texture.data();
      cm[i].tex_height = m.tex_height; cm[i].tex_width = m.tex_width;
      cm[i].diameter = m.diameter;
      for (int k = 0; k < 3; k++) cm[i].center[k] = m.center[k];
    }
    h_ = fp_create(cm.data(), (int)cm.size(), K, refiner_weights.empty() ? nullptr : refiner_weights.c_str(),
                   scorer_weights.empty() ? nullptr : scorer_weights.c_str(), max_h, max_w);
    if (!h_) throw std::runtime_error(std::string("[FoundationPose] Failed to Construct FoundationPose, ex : ") + fp_last_error());
    for (const Mesh &m : meshes)   // meshes without UVs are rendered from their vertex colours, with no extra call from the user
      if (m.color_source == FP_COLOR_VERTEX && fp_set_vertex_colors(h_, m.name.c_str(), m.vertex_colors.data(), (int)(m.vertex_colors.size() / 3))) {
        const std::string why = fp_last_error();
        fp_destroy(h_);
        throw std::runtime_error("[FoundationPose] Failed to Construct FoundationPose, ex : " + why);
      }
  }
  ~FoundationPose() { fp_destroy(h_); }
  FoundationPose(const FoundationPose &) = delete;
  FoundationPose &operator=(const FoundationPose &) = delete;

  // Register (foundationpose.hpp:36-41): false on failure, message in last_error()
  bool Register(const ImageU8 &rgb, const ImageF32 &depth, const ImageU8 &mask, const std::string &target_name,
                Pose &out_pose_in_mesh, size_t refine_itr = 1) {
    if (rgb.rows != depth.rows || rgb.cols != depth.cols || mask.rows != depth.rows || mask.cols != depth.cols) {
      err_ = "[FoundationPose] Got rgb/depth/mask with different size!";
      return false;
    }
    return ok(fp_register(h_, rgb.data, depth.data, mask.data, depth.rows, depth.cols, target_name.c_str(),
                          (int)refine_itr, out_pose_in_mesh.data()));
  }
  // Track (foundationpose.hpp:59-64)
  bool Track(const ImageU8 &rgb, const ImageF32 &depth, const Pose &hyp_pose_in_mesh, const std::string &target_name,
             Pose &out_pose_in_mesh, size_t refine_itr = 1) {
    if (rgb.rows != depth.rows || rgb.cols != depth.cols) {
      err_ = "[FoundationPose] Got rgb/depth/mask with different size!";
      return false;
    }
    return ok(fp_track(h_, rgb.data, depth.data, depth.rows, depth.cols, hyp_pose_in_mesh.data(), target_name.c_str(),
                       (int)refine_itr, out_pose_in_mesh.data()));
  }
  // Track in two halves (pipelined serving: one thread, several objects in flight): the frame must stay valid until TrackWait
  bool TrackSubmit(const ImageU8 &rgb, const ImageF32 &depth, const Pose &hyp_pose_in_mesh, const std::string &target_name,
                   size_t refine_itr = 1) {
    if (rgb.rows != depth.rows || rgb.cols != depth.cols) {
      err_ = "[FoundationPose] Got rgb/depth/mask with different size!";
      return false;
    }
    return ok(fp_track_submit(h_, rgb.data, depth.data, FP_HOST, depth.rows, depth.cols, hyp_pose_in_mesh.data(), target_name.c_str(),
                              (int)refine_itr));
  }
  bool TrackWait(Pose &out_pose_in_mesh) { return ok(fp_track_wait(h_, out_pose_in_mesh.data())); }
  // K objects of one frame as one batch (geometry per object, one refine-net pass over all crops)
  bool TrackMulti(const ImageU8 &rgb, const ImageF32 &depth, const std::vector<Pose> &hyp_poses, const std::vector<std::string> &target_names,
                  std::vector<Pose> &out_poses, size_t refine_itr = 1) {
    if (rgb.rows != depth.rows || rgb.cols != depth.cols || hyp_poses.size() != target_names.size() || hyp_poses.empty()) {
      err_ = "[FoundationPose] TrackMulti: inconsistent arguments";
      return false;
    }
    std::vector<const char *> names;
    for (const auto &n : target_names) names.push_back(n.c_str());
    out_poses.resize(hyp_poses.size());
    return ok(fp_track_multi(h_, rgb.data, depth.data, FP_HOST, depth.rows, depth.cols, (int)hyp_poses.size(), hyp_poses[0].data(), names.data(),
                             (int)refine_itr, out_poses[0].data()));
  }

  // ---- options the reference does not have ----
  // element type of both networks: FP_PREC_F16 (default, the reference's TensorRT --fp16), FP_PREC_BF16, FP_PREC_FP8 / FP_PREC_INT8 (after Calibrate)
  bool SetPrecision(int precision) { return ok(fp_set_precision(h_, precision)); }
  int precision() const { return fp_get_precision(h_); }
  // one f16 Register of a representative frame that records the per-activation maxima the static FP8 quantisation needs
  bool CalibrateFp8(const ImageU8 &rgb, const ImageF32 &depth, const ImageU8 &mask, const std::string &target_name) {
    return ok(fp_calibrate_fp8(h_, rgb.data, depth.data, mask.data, FP_HOST, depth.rows, depth.cols, target_name.c_str()));
  }
  // post-training quantisation of an 8-bit precision on a representative frame (scales + bias correction); the record can be saved and restored
  bool Calibrate(const ImageU8 &rgb, const ImageF32 &depth, const ImageU8 &mask, const std::string &target_name, int precision) {
    return ok(fp_calibrate(h_, rgb.data, depth.data, mask.data, FP_HOST, depth.rows, depth.cols, target_name.c_str(), precision));
  }
  // ... over several frames of the deployment's scene family (K >= 8 recommended: the common-mode correction then carries over to unseen frames)
  bool CalibrateBegin(int precision) { return ok(fp_calibrate_begin(h_, precision)); }
  bool CalibrateAddFrame(const ImageU8 &rgb, const ImageF32 &depth, const ImageU8 &mask, const std::string &target_name) {
    return ok(fp_calibrate_add_frame(h_, rgb.data, depth.data, mask.data, FP_HOST, depth.rows, depth.cols, target_name.c_str()));
  }
  bool CalibrateFinish() { return ok(fp_calibrate_finish(h_)); }
  void CalibrateAbort() { (void)fp_calibrate_abort(h_); }
  bool GetCalibrationBlob(int precision, std::vector<unsigned char> &blob) const {
    blob.resize(fp_calibration_size());
    return fp_get_calibration_blob(h_, precision, blob.data(), blob.size()) == 0;
  }
  bool SetCalibrationBlob(const std::vector<unsigned char> &blob) { return ok(fp_set_calibration_blob(h_, blob.data(), blob.size())); }
  bool GetCalibration(std::array<float, 32> &amax) const { return fp_get_calibration(h_, amax.data()) == 0; }
  bool SetCalibration(const std::array<float, 32> &amax) { return ok(fp_set_calibration(h_, amax.data())); }
  // float model of the rendering stage: FP_FLOAT_FMAD (default: contracted like the reference's nvcc build) or FP_FLOAT_SEPARATE
  bool SetFloatModel(int model) { return ok(fp_set_float_model(h_, model)); }
  // pose fit (foundationpose_amd.h "pose fit"): Track / Register also count how much of the model the depth under the pose agrees with.
  // LastTrackFit: one record per tracked object, of the pose the last refine iteration STARTED from (one frame late with refine_itr 1);
  // LastRegisterFit: the returned pose's record (all: every hypothesis'); PoseFit: any poses on the uploaded frame (fp_upload_frame)
  bool SetPoseFit(bool on, float tol_m = 0.005f) { return ok(fp_set_pose_fit(h_, on ? 1 : 0, tol_m)); }
  // depth filter (foundationpose_amd.h "depth filter"): Register, Track and the stage operators read bilateral(erode(depth)) instead
  // of the depth itself, like FoundationPose as published; default off
  bool SetDepthFilter(bool on) { return ok(fp_set_depth_filter(h_, on ? 1 : 0)); }
  bool DepthFilter() const { return fp_get_depth_filter(h_) == 1; }
  // vertex colours (new; the reference has no counterpart): colors = [V,3] RGB u8 of the target, nullptr = back to its texture
  bool SetVertexColors(const std::string &target_name, const uint8_t *colors, int num_vertices) {
    return ok(fp_set_vertex_colors(h_, target_name.c_str(), colors, num_vertices));
  }
  int ColorSource(const std::string &target_name) const { return fp_get_color_source(h_, target_name.c_str()); }
  bool LastTrackFit(std::vector<fp_pose_fit> &out, size_t objects = 1) {
    out.resize(objects);
    return ok(fp_last_track_fit(h_, out.data(), (int)objects));
  }
  bool LastRegisterFit(fp_pose_fit &winner, std::vector<fp_pose_fit> *all = nullptr) {
    if (all) all->resize((size_t)fp_num_hypotheses(h_));
    return ok(fp_last_register_fit(h_, &winner, all ? all->data() : nullptr, all ? (int)all->size() : 0));
  }
  bool PoseFit(const std::string &target_name, const std::vector<Pose> &poses, std::vector<fp_pose_fit> &out, float crop_ratio = 1.2f,
               float tol_m = 0.005f) {
    out.resize(poses.size());
    return ok(fp_pose_fit_eval(h_, target_name.c_str(), poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), crop_ratio, tol_m, out.data()));
  }
  // a pose at frame resolution (foundationpose_amd.h "a pose at frame resolution"): the target under `pose` rasterised at the size of
  // the uploaded frame (fp_upload_frame, a Register or a device-frame Track); every pointer of `out` is optional and lives in `memspace`.
  // FP_DEVICE: the kernel writes the caller's buffers directly -- out.visible_mask is the mask of the next fp_register_ex.
  // A pose that would need clipping (a vertex nearer than FP_RENDER_NEAR_M) is refused: false + last_error().
  bool RenderPose(const std::string &target_name, const Pose &pose, const fp_frame_render &out, float tol_m = 0.005f, int memspace = FP_HOST) {
    return ok(fp_render_pose(h_, target_name.c_str(), pose.data(), tol_m, &out, memspace));
  }
  // all tracked objects of a frame in one pass (foundationpose_amd.h "all tracked objects of a frame"): instance map, amodal coverage
  // bits, visible mask, overlay in per-object tints; `objects` (may be null) receives one record of pixel counts per object.
  bool RenderScene(const std::vector<std::string> &target_names, const std::vector<Pose> &poses, const fp_scene_render &out,
                   std::vector<fp_scene_object> *objects = nullptr, float tol_m = 0.005f, int memspace = FP_HOST) {
    if (target_names.size() != poses.size()) {
      err_ = "[FoundationPose] RenderScene: one pose per target name";
      return false;
    }
    std::vector<const char *> names;
    for (const auto &n : target_names) names.push_back(n.c_str());
    if (objects) objects->resize(poses.size());
    return ok(fp_render_scene(h_, (int)poses.size(), names.data(), poses.empty() ? nullptr : poses[0].data(), tol_m, &out,
                              objects ? objects->data() : nullptr, memspace));
  }

  // pose errors (foundationpose_amd.h "pose errors"): ADD, ADD-S, MSSD and MSPD of `est` against `gt` (one pose per estimate, or ONE for
  // all of them: every hypothesis of a Register against one truth).  symmetries: mesh frame, already discretised (BOP's models_info.json);
  // the identity is always symmetry 0 of best_sym.  adds = false skips the Vs^2 nearest-neighbour part (adds_m is NaN then).  Needs no frame.
  bool PoseErrors(const std::string &target_name, const std::vector<Pose> &est, const std::vector<Pose> &gt, std::vector<fp_pose_error> &out,
                  const std::vector<Pose> &symmetries = {}, int vertex_step = 1, bool adds = true) {
    out.resize(est.size());
    return ok(fp_pose_errors(h_, target_name.c_str(), est.empty() ? nullptr : est[0].data(), (int)est.size(), gt.empty() ? nullptr : gt[0].data(),
                             (int)gt.size(), symmetries.empty() ? nullptr : symmetries[0].data(), (int)symmetries.size(), vertex_step,
                             adds ? FP_POSE_ERROR_ADDS : 0, out.data()));
  }

  // visible surface discrepancy (foundationpose_amd.h "visible surface discrepancy"): BOP's VSD of `est` against `gt` (one pose per
  // estimate, or ONE for all of them) on the uploaded frame's raw depth.  taus: up to FP_VSD_MAX_TAUS tolerances, fractions of the target's
  // diameter when `normalized` (BOP19) and metres otherwise.  A pose that would need a clipper gets its status bit and vsd 1, not an error.
  bool PoseVsd(const std::string &target_name, const std::vector<Pose> &est, const std::vector<Pose> &gt, std::vector<fp_pose_vsd_t> &out,
               float delta_m = 0.015f, const std::vector<float> &taus = {0.05f, 0.10f, 0.15f, 0.20f, 0.25f, 0.30f, 0.35f, 0.40f, 0.45f, 0.50f},
               bool normalized = true) {
    out.resize(est.size());
    return ok(fp_pose_vsd(h_, target_name.c_str(), est.empty() ? nullptr : est[0].data(), (int)est.size(), gt.empty() ? nullptr : gt[0].data(),
                          (int)gt.size(), delta_m, taus.empty() ? nullptr : taus.data(), (int)taus.size(), normalized ? FP_VSD_NORMALIZED : 0,
                          out.data()));
  }

  // depth refinement (foundationpose_amd.h "depth refinement"): projective point-to-plane ICP of `poses` on the uploaded frame's raw depth;
  // `refined` gets the poses, `out` how each fits and how its refinement went.  max_dist_m: the gate along the ray, at most the target's
  // diameter.  translation_only: leave the rotation alone (symmetric objects).  A pose that would need a clipper comes back unchanged
  // with its status bit, not an error.
  bool RefineDepth(const std::string &target_name, const std::vector<Pose> &poses, std::vector<Pose> &refined, std::vector<fp_depth_refine_t> &out,
                   int iterations = 10, float max_dist_m = 0.02f, bool translation_only = false) {
    refined.resize(poses.size());
    out.resize(poses.size());
    return ok(fp_refine_depth(h_, target_name.c_str(), poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), iterations, max_dist_m,
                              translation_only ? FP_ICP_TRANSLATION_ONLY : 0, refined.empty() ? nullptr : refined[0].data(), out.data()));
  }

  // depth search (foundationpose_amd.h "depth search"): `poses` against the uploaded frame's raw depth, each at n_steps pushes of step_m
  // along the ray of its origin; `out` gets the counts at every pose's best step.  vertex_step: every vertex_step-th vertex is used.
  bool PoseSearch(const std::string &target_name, const std::vector<Pose> &poses, std::vector<fp_pose_search_t> &out, int n_steps, float step_m,
                  float tol_m = 0.005f, int vertex_step = 1) {
    out.resize(poses.size());
    return ok(fp_pose_search(h_, target_name.c_str(), poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), n_steps, step_m, tol_m, vertex_step,
                             out.data()));
  }

  // Register without weights (foundationpose_amd.h "Register without weights"): the hypothesis grid ranked by PoseSearch on the depth
  // alone, the top_k candidates refined by RefineDepth, the one that explains most of the depth wins.  0 for top_k, tol_m or
  // icp_iterations means the default (16, 0.005 m, 15).  The frame stays uploaded; `record` may be null.
  bool RegisterDepth(const ImageU8 &rgb, const ImageF32 &depth, const ImageU8 &mask, const std::string &target_name, Pose &out_pose_in_mesh,
                     fp_depth_register_t *record = nullptr, int top_k = 0, float tol_m = 0.0f, int icp_iterations = 0) {
    if (rgb.rows != depth.rows || rgb.cols != depth.cols || mask.rows != depth.rows || mask.cols != depth.cols) {
      err_ = "[FoundationPose] Got rgb/depth/mask with different size!";
      return false;
    }
    return ok(fp_register_depth(h_, rgb.data, depth.data, mask.data, FP_HOST, depth.rows, depth.cols, target_name.c_str(), top_k, tol_m, icp_iterations,
                                out_pose_in_mesh.data(), record));
  }

  // colour agreement (foundationpose_amd.h "colour agreement"): the model's unshaded colour (texture, or vertex colours) under `poses`
  // against the uploaded frame's RGB over the visible model pixels; `out` gets the integer sums and the zncc of each.  tol_m: the occlusion
  // tolerance of RenderPose.  A pose that would need a clipper gets its status bit and zncc 0, not an error.
  bool PoseColor(const std::string &target_name, const std::vector<Pose> &poses, std::vector<fp_pose_color_t> &out, float tol_m = 0.005f) {
    out.resize(poses.size());
    return ok(fp_pose_color(h_, target_name.c_str(), poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), tol_m, out.data()));
  }

  // symmetry resolution (foundationpose_amd.h "symmetry resolution"): of the equivalents pose * S_s of a symmetric object's pose the one
  // whose colour agrees best with the frame.  symmetries: mesh frame, already discretised, as for PoseErrors; the identity is always
  // symmetry 0 of best_sym.  `records` (may be null) gets the S + 1 records.  Fails when no equivalent has a usable record (untextured).
  bool ResolveSymmetry(const std::string &target_name, const Pose &pose, const std::vector<Pose> &symmetries, Pose &out_pose, int *best_sym = nullptr,
                       std::vector<fp_pose_color_t> *records = nullptr, float tol_m = 0.005f) {
    if (records) records->resize(symmetries.size() + 1);
    return ok(fp_resolve_symmetry(h_, target_name.c_str(), pose.data(), symmetries.empty() ? nullptr : symmetries[0].data(), (int)symmetries.size(), tol_m,
                                  out_pose.data(), best_sym, records ? records->data() : nullptr));
  }

  // silhouette agreement (foundationpose_amd.h "silhouette agreement"): the exact squared Euclidean distance transform of a u8 mask of the
  // uploaded frame's size (a mask pixel: byte > 0): per pixel the squared distance to the nearest mask pixel and to the nearest other
  // pixel, FP_SIL_D2_NONE where there is none.  Either output may be null, not both; they are resized to `pixels` = H * W of the frame.
  bool MaskDistance(const uint8_t *mask, size_t pixels, std::vector<uint32_t> *d2_to_mask, std::vector<uint32_t> *d2_to_bg, int memspace = FP_HOST) {
    if (d2_to_mask) d2_to_mask->resize(pixels);
    if (d2_to_bg) d2_to_bg->resize(pixels);
    return ok(fp_mask_distance(h_, mask, memspace, d2_to_mask ? d2_to_mask->data() : nullptr, d2_to_bg ? d2_to_bg->data() : nullptr));
  }

  // ... and the (visible) silhouette of the model under `poses` against that mask; `out` gets the counts, the integer sums and the IoU of
  // each.  tol_m: the occlusion tolerance of RenderPose; trunc_px > 0 clips every squared distance to trunc_px^2; flags: FP_SIL_AMODAL.
  // A pose that would need a clipper gets its status bit and nothing else, not an error.
  bool PoseSilhouette(const std::string &target_name, const uint8_t *mask, const std::vector<Pose> &poses, std::vector<fp_pose_silhouette_t> &out,
                      float tol_m = 0.005f, int trunc_px = 0, int flags = 0, int memspace = FP_HOST) {
    out.resize(poses.size());
    return ok(fp_pose_silhouette(h_, target_name.c_str(), mask, memspace, poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), tol_m, trunc_px,
                                 flags, out.data()));
  }

  // silhouette refinement (foundationpose_amd.h "silhouette refinement"): `poses` moved until the model's outline lies on the outline of
  // that mask; `refined` gets the poses, `out` the counts, the integer sums and how each iteration ended.  No depth is read unless flags
  // has FP_SILREF_OCCLUSION (tol_m is RenderPose's tolerance then); gate_px > 0 drops outline pixels farther than that from the mask's
  // outline; FP_SILREF_TRANSLATION_ONLY leaves the rotation alone.  A pose that would need a clipper comes back unchanged with its status bit.
  bool RefineSilhouette(const std::string &target_name, const uint8_t *mask, const std::vector<Pose> &poses, std::vector<Pose> &refined,
                        std::vector<fp_silhouette_refine_t> &out, int iterations = 15, int gate_px = 0, float tol_m = 0.005f, int flags = 0,
                        int memspace = FP_HOST) {
    refined.resize(poses.size());
    out.resize(poses.size());
    return ok(fp_refine_silhouette(h_, target_name.c_str(), mask, memspace, poses.empty() ? nullptr : poses[0].data(), (int)poses.size(), iterations,
                                   gate_px, tol_m, flags, refined.empty() ? nullptr : refined[0].data(), out.data()));
  }

  const std::string &last_error() const { return err_; }
  fp_model *handle() { return h_; }

private:
  bool ok(int rc) {
    err_ = rc ? fp_last_error() : "";
    return rc == 0;
  }
  fp_model *h_ = nullptr;
  std::string err_;
};

}  // namespace fp_amd
