/*
 * foundationpose_amd.h -- C ABI of the MI355X-native FoundationPose Register/Track hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / OpenCV / Eigen types.
 * Every entry point names the reference interface it replaces (path:line under zz990099/foundationpose_cpp,
 * D6F = detection_6d_foundationpose).  INTEGRATION.md shows the C++ shim that puts the reference's own
 * `detection_6d::Base6DofDetectionModel` header on top of these calls.
 *
 * Conventions
 *   - 4x4 poses are COLUMN-MAJOR float[16] (Eigen::Matrix4f::data()), translation at [12..14].
 *   - K is ROW-MAJOR float[9].
 *   - rgb: u8 [H,W,3] RGB order; depth: f32 [H,W] metres; mask: u8 [H,W], >0 = object.
 *   - returned poses are CENTRED-mesh -> camera, exactly like the reference (D6F/src/foundationpose_render.cpp:396-398);
 *     use the mesh centre to convert (D6F/include/detection_6d_foundationpose/mesh_loader.hpp:75-81).
 *   - every function returning int returns 0 on success, non-zero on failure; fp_last_error() describes it
 *     (the reference returns bool + a glog line, D6F/src/foundationpose_utils.hpp:76-84).
 *   - not re-entrant per model (like the reference: one renderer / scratch set per target,
 *     D6F/src/foundationpose.cpp:103-105); DIFFERENT models may be driven from different threads concurrently, each runs
 *     on its own non-blocking stream and their kernels overlap on the GPU.  fp_create / fp_destroy (fp_net_create / fp_net_destroy) and the
 *     entry points that load or rebuild networks (fp_set_precision, fp_set_calibration*, fp_set_float_model) are
 *     exclusive against every other call of the process: they wait for calls in progress and hold new ones back while they run.
 *   - memspace arguments: FP_HOST pointers are ordinary host memory, FP_DEVICE pointers are HIP device memory on
 *     the model's device (lets callers keep frames resident in HBM).
 */
#ifndef FOUNDATIONPOSE_AMD_H
#define FOUNDATIONPOSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP_HOST 0
#define FP_DEVICE 1

#define FP_CROP 160            /* crop_window_H/W, D6F/src/foundationpose.cpp:34-35 */
#define FP_NUM_HYP_DEFAULT 252 /* score_mode_poses_num_, D6F/src/foundationpose.cpp:85 */
/* Largest number of hypotheses one network call takes (refine-net / score-net batch, Register's hypothesis count, fp_net_create's
 * max_batch, a Register shard).  Several network kernels address activation tensors with 32-bit signed byte offsets; the largest such
 * tensor holds 903168 bytes per hypothesis (a bordered 42x42x256 map, or two 42x42x128 maps), so 2377 hypotheses keep every offset below
 * 2^31 ("Batch limit").  Larger batches are refused with an error before anything is launched. */
#define FP_MAX_BATCH 2377
#define FP_MAX_INPLANE_STEPS 56 /* 42 * 56 = 2352 <= FP_MAX_BATCH hypotheses */

typedef struct fp_model fp_model;

/* What detection_6d::BaseMeshLoader exposes (D6F/include/detection_6d_foundationpose/mesh_loader.hpp:25-61). */
typedef struct fp_mesh {
  const char *name;          /* GetName() */
  int num_vertices;          /* GetMeshNumVertices() */
  int num_faces;             /* GetMeshNumFaces() */
  const float *vertices;     /* GetMeshVertices()       [V,3], mesh frame (NOT centred) */
  const float *normals;      /* GetMeshVertexNormals()  [V,3] */
  const float *texcoords;    /* GetMeshTextureCoords()  [V,2] = (u,v) as loaded (v is flipped internally) */
  const uint32_t *faces;     /* GetMeshTriangleFaces()  [F,3]; a face whose centred corners are exactly collinear is never drawn
                              * (its number stays reserved): snapped to 1/16 px it could open into a sliver */
  const uint8_t *texture;    /* GetTextureMap()         [tex_height,tex_width,3] RGB u8 */
  int tex_height, tex_width;
  float diameter;            /* GetMeshDiameter() */
  float center[3];           /* GetMeshModelCenter() */
} fp_mesh;

/* ---- mesh loading: CreateAssimpMeshLoader(name, mesh_file_path) (mesh_loader.hpp:92-93, src/mesh_loader/assimp_mesh_loader.cpp:159-228)
 * without assimp/OpenCV.  Mesh files: Wavefront OBJ (+ MTL map_Kd) and Stanford PLY (ascii / binary, per-vertex or per-wedge UVs,
 * `comment TextureFile`: the form of the BOP / YCB-V object models); the name is historical.  Textures: PNG (any bit depth, interlaced
 * or not), baseline / progressive JPEG (decoded like libjpeg-turbo), BMP, PNM, TGA -> RGB u8 as cv::imread + BGR2RGB delivers it.  Returns NULL
 * (+ fp_last_error) where the reference throws: empty path, unreadable file, no texture coordinates; also for a texture file that
 * exists but cannot be decoded (never a silent grey texture).  Missing texture -> 2x2 (100,100,100) like the reference. */
typedef struct fp_loaded_mesh fp_loaded_mesh;
fp_loaded_mesh *fp_mesh_load_obj(const char *name, const char *mesh_file_path);
void fp_mesh_free(fp_loaded_mesh *mesh);
/* all BaseMeshLoader getters as one fp_mesh view (valid until fp_mesh_free) */
const fp_mesh *fp_mesh_view(const fp_loaded_mesh *mesh);
/* GetOrientBounds() (column-major 4x4: PCA axes | vertex mean) and GetObjectDimension() */
int fp_mesh_orient_bounds(const fp_loaded_mesh *mesh, float orient_bounds[16], float dimension[3]);
/* Colour source of a loaded mesh (new; the reference has no counterpart -- its loader refuses a mesh without texture coordinates).
 * A file with usable UVs is FP_COLOR_TEXTURE: the fp_mesh view is what it always was, whether or not the file also carries colours.
 * A file without usable UVs but with per-vertex colours -- PLY `red green blue` / `diffuse_red diffuse_green diffuse_blue` (integer types
 * 0..255, float types 0..1 stored as rint(clamp(c, 0, 1) * 255), alpha skipped), OBJ `v x y z r g b` (0..1) on EVERY `v` line -- loads as
 * FP_COLOR_VERTEX: the form of the LineMOD / LM-O / T-LESS / HomebrewedDB / ITODD models and of scanner output.  Its fp_mesh view carries
 * zero texcoords and the 2x2 (100,100,100) default texture, so fp_create takes it as it is and a caller that never hands the colours
 * over renders a grey object.  A file with neither still fails with the reference's message. */
#define FP_COLOR_TEXTURE 0
#define FP_COLOR_VERTEX 1
int fp_mesh_color_source(const fp_loaded_mesh *mesh);
/* [num_vertices,3] RGB u8 in the view's vertex order (a colour belongs to its position and follows it through the de-duplication),
 * valid until fp_mesh_free; NULL when the file had none.  Textured meshes that also carry colours return them too. */
const uint8_t *fp_mesh_vertex_colors(const fp_loaded_mesh *mesh);

/* ---- construction: CreateFoundationPoseModel (D6F/include/.../foundationpose.hpp:99-105, src/foundationpose.cpp:108-153,448-458).
 * refiner_weights / scorer_weights: paths of packed weight files (tools/pack_weights.py; replaces the TensorRT
 * engines of simple_tests/src/test_foundationpose.cpp:13-14).  NULL = geometry-only model (NN entry points fail).
 * K: the 3x3 intrinsics, row-major; all nine entries are copied.  Register, Track and the stage operators of their path take K as the
 * reference does, as a matrix, so a skew K[1] is honoured there.  The twelve frame-resolution calls -- fp_render_pose, fp_render_scene,
 * fp_pose_errors, fp_pose_vsd, fp_refine_depth, fp_pose_search, fp_register_depth, fp_pose_color, fp_resolve_symmetry,
 * fp_mask_distance, fp_pose_silhouette, fp_refine_silhouette -- read fx = K[0], fy = K[4], cx = K[2], cy = K[5]
 * only and REFUSE a model whose K is not a plain pinhole matrix (K[1] == K[3] == K[6] == K[7] == 0, K[8] == 1, K[0] and K[4] finite and
 * positive, K[2] and K[5] finite): on the host, before anything is uploaded or launched, with a message that names the entry, their
 * outputs untouched.  fx != fy and a principal point anywhere are fine everywhere. */
fp_model *fp_create(const fp_mesh *meshes, int n_meshes, const float K[9], const char *refiner_weights,
                    const char *scorer_weights, int max_input_image_height, int max_input_image_width);
/* The same on HIP device `device` (-1 = the calling thread's current device, which is what fp_create uses).  A model remembers its
 * device: every entry point makes it current for the duration of the call and restores the caller's afterwards, so a process that
 * drives several GPUs -- one host thread per GPU, the natural C++ shape of SURVEY.md section 8e, or one thread walking over the
 * models -- cannot launch a model's work on the wrong device.  FP_DEVICE pointers handed to a model must live on ITS device. */
fp_model *fp_create_on(int device, const fp_mesh *meshes, int n_meshes, const float K[9], const char *refiner_weights,
                       const char *scorer_weights, int max_input_image_height, int max_input_image_width);
int fp_device(const fp_model *m);
void fp_destroy(fp_model *m);
const char *fp_last_error(void);
/* number of in-plane rotations per icosphere view: 6 -> 252 hypotheses (reference), 24 -> 1008 (SURVEY.md §8a note); 1..FP_MAX_INPLANE_STEPS. */
int fp_set_inplane_steps(fp_model *m, int steps);
int fp_num_hypotheses(const fp_model *m);

/* ---- Base6DofDetectionModel::Register / Track (D6F/include/.../foundationpose.hpp:36-41,59-64; src/foundationpose.cpp:181-265). */
int fp_register(fp_model *m, const uint8_t *rgb, const float *depth, const uint8_t *mask, int H, int W,
                const char *target_name, int refine_itr, float out_pose[16]);
/* Track with refine_itr == 1 reads the frame only inside the observed-crop window of the hypothesis: from a host frame only that
 * window is uploaded -- packed into a pinned block of the model and fetched from there when it is at most half the frame wide,
 * whole rows otherwise (the stage operators below refuse the resulting partial copy until the next fp_upload_frame / Register). */
int fp_track(fp_model *m, const uint8_t *rgb, const float *depth, int H, int W, const float hyp_pose[16],
             const char *target_name, int refine_itr, float out_pose[16]);
/* Track in two halves for pipelined serving (one host thread, several models / objects in flight; the reference's un-vendored
 * async_pipeline plays this role, D6F/src/foundationpose_utils.hpp:33-37): fp_track_submit ENQUEUES the frame upload and the whole
 * refinement on the model's stream and returns; fp_track_wait returns the pose once the refinement has finished.  (It polls a flag the
 * last kernel raises in host-pinned memory right after storing the pose there -- ~13 us sooner per Track than a stream wait -- and
 * falls back to hipStreamSynchronize, which also reports device errors; later calls on the model are stream-ordered behind it.)
 * A host frame must stay valid until the wait; one submission per model at a time. */
int fp_track_submit(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, const float hyp_pose[16],
                    const char *target_name, int refine_itr);
int fp_track_wait(fp_model *m, float out_pose[16]);
/* Track of K (1..64) objects of one frame as ONE batch: hyp_poses / out_poses are K column-major 4x4 matrices, target_names K names
 * (objects with the same mesh should be adjacent).  The rendering runs per object, the refine-net once over all K crops; at this
 * size the step is launch-latency-bound, so K objects cost little more than one. */
int fp_track_multi(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, int K, const float *hyp_poses,
                   const char *const *target_names, int refine_itr, float *out_poses);
/* same, frame already resident in HBM (memspace FP_DEVICE for rgb/depth/mask) */
int fp_register_ex(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                   const char *target_name, int refine_itr, float out_pose[16]);
int fp_track_ex(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W,
                const float hyp_pose[16], const char *target_name, int refine_itr, float out_pose[16]);

/* ---- pose fit: is the answer any good? (new; the reference has no counterpart) ---------------------------------------------
 * Track returns a pose on every frame and Register the best of its hypotheses, whatever the frame shows.  With this option on, the
 * calls also compare, per hypothesis, the model rendered at the pose with the depth observed under it -- the two 160x160 crops the
 * networks are fed anyway, both in units of (p - t_hyp) / (diameter / 2) -- and report integer counts.
 * A crop pixel is a MODEL pixel when the rendered (x, y, z) is not (0, 0, 0); it is OBSERVED when, in addition, the observed z is not
 * 0 (no valid depth, outside the frame and more than two diameters away all read 0).  With d = observed z - rendered z (one f32
 * subtraction) and tol_n = (float)tol_m / ((float)diameter / 2), an observed pixel is an INLIER when |d| <= tol_n, in FRONT when
 * d < -tol_n (something nearer than the model: an occluder) and BEHIND when d > tol_n (the surface is not where the model says).
 * The record is bit-reproducible: the same frame and pose give the same record on every call.  It is computed from the crops the
 * networks are fed: with fp_set_depth_filter on, the observed z is that of the filtered depth. */
typedef struct fp_pose_fit {
  int32_t n_model, n_observed, n_inlier, n_front, n_behind; /* n_observed == n_inlier + n_front + n_behind */
  int32_t reserved;
  int64_t sum_dz_q20;   /* sum over inliers of rint((B.z - A.z) * 2^20), normalised units */
  float   mean_dz_m;    /* host-derived: sum_dz_q20 / 2^20 / n_inlier * diam/2; 0 when n_inlier == 0 */
  float   tol_n;        /* the f32 threshold the kernel used */
} fp_pose_fit;
/* Default off; tol_m in metres, finite and > 0 (a few times the sensor's depth noise).  While off, nothing is launched or allocated
 * for it.  Toggling, or changing tol_m, drops the captured graphs (the next two calls of each kind run eagerly / capture again). */
int fp_set_pose_fit(fp_model *m, int on, float tol_m);
int fp_get_pose_fit(const fp_model *m, int *on, float *tol_m);
/* The records of the last fp_track / _ex / _submit + _wait (one record) or fp_track_multi (one per object, in order) that ran with the
 * option on; out holds K >= that many.  A record describes the pose the LAST refine iteration STARTED FROM, against this frame: with
 * refine_itr == 1 that is the caller's hyp_pose -- usually the previous frame's answer -- so a lost object shows one frame late, and
 * costs no extra rendering.  (fp_pose_fit_eval scores any pose, the returned one included.)  Fails when the last Track had the
 * option off, refine_itr <= 0, failed, or has not been waited for. */
int fp_last_track_fit(fp_model *m, fp_pose_fit *out, int K);
/* The records of the last fp_register / _ex, or fp_register_shard_begin over ALL hypotheses + fp_register_shard_finish, that ran with
 * the option on: they describe the FINAL (refined) poses at the score pass's crop ratio 1.1.  winner = the record of the returned
 * pose; all (may be NULL) = every hypothesis, N >= fp_num_hypotheses() records, fetched with a diagnostic device -> host copy.
 * Out of scope: fp_register_sharded and shards smaller than the grid compute no fit (the winner's crop lives on one rank only);
 * the call fails after them.  The 8-bit precisions feed the networks the same 2-byte input tensor, so the records do not change. */
int fp_last_register_fit(fp_model *m, fp_pose_fit *winner, fp_pose_fit *all, int N);
/* Stage operator: the records of N (1..FP_MAX_BATCH) poses (host [N*16]) of `target_name` on the uploaded frame at `crop_ratio`
 * (Track refines at 1.2, Register scores at 1.1), through the same render / crop kernels and the same fit kernel, whether the option
 * is on or off.  Refuses a partially uploaded frame like the other stage operators. */
int fp_pose_fit_eval(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio, float tol_m, fp_pose_fit *out);

/* ---- vertex colours: meshes without texture coordinates (new; the reference has no counterpart) ------------------------------
 * FoundationPose as published renders a mesh without UVs by interpolating its vertex colours.  fp_set_vertex_colors makes
 * `colors` ([num_vertices,3] RGB u8, host memory, copied; num_vertices must equal the target's vertex count) the colour source of
 * `target_name`: a foreground pixel of its renderings is then sum_k b_k * (c_k / 255) over the triangle's corners -- the rule every
 * interpolated attribute follows, in the model's float model -- times the Lambert term, instead of a texture sample (DESIGN.md
 * section 4.1).  Geometry channels, triangle ids and the crop do not change.  colors == NULL returns the target to its texture.
 * Works on geometry-only models.  Like fp_set_pose_fit it waits for the model's work and drops the captured graphs; while no target
 * uses vertex colours nothing is allocated, launched or captured differently.  Errors: unknown target, count mismatch. */
int fp_set_vertex_colors(fp_model *m, const char *target_name, const uint8_t *colors, int num_vertices);
/* FP_COLOR_TEXTURE / FP_COLOR_VERTEX, or a negative value on an unknown target */
int fp_get_color_source(const fp_model *m, const char *target_name);

/* ---- depth filter: what FoundationPose as published feeds its networks (new; the reference filters for the sampler only) -----
 * Default off: exactly the behaviour without the option.  With the option on, every depth value a crop or warp reads is taken from
 * D' = bilateral(erode(D)) of the current frame instead of D: erode with radius 2, difference 0.001 m, ratio 0.8, zfar 100; bilateral
 * with radius 2, sigmaD 2, sigmaR 1e5 and |d - mean| < 0.01 -- the sampler's constants, so D' is the array fp_filter_depth returns as
 * bilateral_out, frame borders included (a neighbour outside the frame is skipped, not read as zero).  The caller's depth is never
 * modified, FP_DEVICE frames included.  RGB, the rendered half, triangle ids and the crop window transform do not change.
 * Applies to fp_register / _ex / _shard_begin / _shard_begin_packed / _sharded, fp_track / _ex / _submit / _multi, the Registers of
 * the 8-bit calibration (which then collect their statistics on filtered input: calibrate with the option set as it will be served)
 * and the stage operators on an uploaded frame: fp_render_and_transform, fp_pose_fit_eval and fp_get_xyz_map (the map of D', which
 * is what the networks see).  fp_filter_depth and fp_get_hyp_poses do not change.  The pose fit reads the crops the networks are
 * fed, so its records follow the option.
 * Erode zeroes depth below 0.1 m (not 0.001 m): with the option on, an object nearer than 10 cm has no observed geometry.
 * Register reuses the D' its sampler computes anyway; a Track with refine_itr == 1 filters only its crop window, in one kernel
 * (DESIGN.md section 4.7).  Works on geometry-only models.  Like fp_set_pose_fit it waits for the model's work and drops the captured
 * graphs; while the option is off nothing is allocated, launched or captured differently. */
int fp_set_depth_filter(fp_model *m, int on);
/* 1 / 0, or a negative value on a null model */
int fp_get_depth_filter(const fp_model *m);

/* ---- a pose at frame resolution: which pixels of this frame are the object? (new; the reference has no counterpart) ------------
 * fp_render_pose rasterises `target_name` under `pose` (centred-mesh -> camera, column-major: what Register and Track return) at the
 * size of the uploaded frame (fp_upload_frame, or whatever the last Register / device-frame Track left) with the model's K, and
 * compares it per pixel with the observed depth.  Geometry only: no texture, no vertex colours, no anti-aliasing.  Rules (DESIGN.md
 * section 4.8; every f32 operation separately rounded, independent of fp_set_float_model): vertices are projected and snapped to
 * 1/16 px; the sample point of pixel (c, r) is the image point (c, r) of K -- the convention of the xyz map, NOT c + 0.5; coverage is
 * decided by 64-bit integer edge functions with a top-left fill rule, both windings drawn; depth is perspective-correct; the nearest
 * triangle wins and at equal depth the lower index.  The result is bit-reproducible and independent of thread order.
 * With D the observed depth at the pixel, a model pixel is OCCLUDED when !(D < 0.001f) && D < z - tol_m (one f32 subtraction) and
 * VISIBLE otherwise: missing depth counts as visible.  tol_m must be finite and >= 0.
 * D is always the RAW uploaded depth, whether fp_set_depth_filter is on or off.
 * There is no clipper: a pose with any vertex at z < FP_RENDER_NEAR_M (1 cm; the depth VALIDITY threshold of the frame is 0.001 m), or
 * with a vertex that projects beyond FP_RENDER_SNAP_MAX sixteenths of a pixel (the range that keeps the edge functions exact), is
 * refused with an error before anything is rasterised.
 * Every output pointer is optional (NULL = not wanted; all NULL is an error) and lives in `memspace`.  FP_DEVICE outputs are written
 * by the kernel directly -- visible_mask can go straight into fp_register_ex as the mask of a re-Register;
 * FP_HOST outputs are copied on the model's stream, followed by one synchronisation.  H and W are the uploaded frame's.
 * Works on geometry-only models; refuses a partially uploaded frame like the other stage operators, and a model whose K is not a plain
 * pinhole matrix (see fp_create; so do the six calls below that share its projection).  Register, Track, their captured
 * graphs and every existing kernel are untouched: the call's buffers are its own, allocated at its first use. */
#define FP_RENDER_NEAR_M 0.01f
#define FP_RENDER_SNAP_MAX 67108864 /* 2^26 */
typedef struct fp_frame_render {      /* every pointer optional (NULL = not wanted); all in the call's memspace */
  float   *model_depth;   /* [H,W]   camera z of the nearest model surface, metres; 0 = background            */
  uint8_t *model_mask;    /* [H,W]   255 where the model covers the pixel, else 0                             */
  uint8_t *visible_mask;  /* [H,W]   255 where it does and nothing observed is in front of it, else 0         */
  int32_t *tri_id;        /* [H,W]   triangle index + 1, 0 = background (tests / debugging)                   */
  uint8_t *overlay;       /* [H,W,3] the uploaded rgb with the visible model pixels drawn flat-shaded over it */
} fp_frame_render;
int fp_render_pose(fp_model *m, const char *target_name, const float pose[16], float tol_m,
                   const fp_frame_render *out, int memspace);

/* ---- all tracked objects of a frame at frame resolution, in one pass (new; the reference has no counterpart) -------------------
 * fp_render_scene rasterises K (1..FP_SCENE_MAX_OBJECTS) objects -- target_names[o] under poses[o], K column-major 4x4 matrices as
 * fp_track_multi takes and returns them; names may repeat -- into ONE picture of the uploaded frame's size.  Per object the rules
 * are fp_render_pose's, unchanged (snap to 1/16 px, sample point (c, r), 64-bit edge functions with the top-left rule, both windings,
 * perspective-correct z, every f32 operation separately rounded, independent of fp_set_float_model).  The
 * objects meet in one z-buffer whose key is bits(z) << 32 | g, g = the number of faces of the objects before o in the call + the
 * triangle's index: the nearest surface wins, at equal depth the lower object index, then the lower triangle.  The face counts of
 * the call must sum to less than 2^32 - 1.
 * cover_bits: bit o of a pixel is set when ANY triangle of object o covers the sample point, whoever wins the depth test: the full
 * (amodal) silhouettes of all K objects.  A pixel is VISIBLE by fp_render_pose's rule applied to the winning z against the raw
 * uploaded depth D: occluded when !(D < 0.001f) && D < z - tol_m.  The overlay draws every visible model pixel as
 * (rgb + (tint * k + 127) / 255 + 1) >> 1 with k the flat shade of the winning triangle (as in fp_render_pose) and tint the entry
 * o % 8 of the palette (40,220,120) (230,80,60) (70,130,240) (240,200,40) (200,80,220) (40,210,220) (250,140,30) (160,230,60).
 * objects (HOST memory whatever the memspace; may be NULL): per object the integer pixel counts below; all are sums of integers, so
 * bit-identical from call to call.  n_hidden separates "behind another tracked object" from n_occluded, "behind something observed".
 * Refused with an error before anything is rasterised and before any output is written: K outside 1..64, an unknown name (the
 * message says which index), tol_m not finite or negative, no / a partial frame, a pending Track, all seven outputs NULL, and a
 * pose fp_render_pose would refuse (the message contains "pose refused" and the lowest refused object index).  An object wholly
 * outside the frame is not an error: its counts are zero.
 * Every image pointer is optional and lives in `memspace`; FP_DEVICE outputs are written by the kernel directly, FP_HOST outputs
 * are copied on the model's stream.  One synchronisation inside the call (refusal words + the size of the tile lists), one at its
 * end.  Works on geometry-only models.  fp_render_pose, Register, Track and their captured graphs are untouched: the call's buffers
 * are its own, allocated at its first use, grow-only. */
#define FP_SCENE_MAX_OBJECTS 64            /* = fp_track_multi's K limit */
typedef struct fp_scene_object {           /* one per object, all integers, order-independent */
  int32_t n_covered;   /* frame pixels inside the object's own silhouette (amodal)                         */
  int32_t n_front;     /* of those, pixels where this object is the nearest model                          */
  int32_t n_hidden;    /* n_covered - n_front: another object of the call is in front (or wins the tie)    */
  int32_t n_visible;   /* of n_front, pixels not occluded by the observed depth (fp_render_pose's rule)    */
  int32_t n_occluded;  /* n_front - n_visible                                                              */
  int32_t reserved[3];
} fp_scene_object;
typedef struct fp_scene_render {           /* every pointer optional; all in the call's memspace */
  float    *model_depth;   /* [H,W]   z of the nearest model surface over all objects, 0 = background                */
  uint8_t  *instance_id;   /* [H,W]   object index + 1 of that surface, 0 = background                               */
  uint8_t  *visible_mask;  /* [H,W]   255 where a model is nearest and nothing observed is in front of it            */
  int32_t  *tri_id;        /* [H,W]   triangle index + 1 WITHIN the winning object's mesh, 0 = background            */
  uint64_t *cover_bits;    /* [H,W]   bit o set where object o's silhouette covers the pixel (amodal masks of all K) */
  uint8_t  *overlay;       /* [H,W,3] the uploaded rgb with every visible model pixel drawn in its object's tint     */
} fp_scene_render;
int fp_render_scene(fp_model *m, int K, const char *const *target_names, const float *poses /* K column-major 4x4 */,
                    float tol_m, const fp_scene_render *out, fp_scene_object *objects /* host [K], may be NULL */, int memspace);

/* ---- pose errors: how wrong is a pose? ADD, ADD-S, MSSD, MSPD with object symmetries (new; the reference has no counterpart) ----
 * fp_pose_errors compares N (1..FP_MAX_BATCH) estimated poses of `target_name` with ground truth: est_poses and gt_poses are column-major
 * 4x4 matrices, centred-mesh -> camera, rigid (what Register and Track return); n_gt == N pairs estimate i with ground truth i,
 * n_gt == 1 compares every estimate with the one ground truth (all hypotheses of a Register against one truth).  With E the
 * estimate, G the ground truth and v the used vertices of the target's centred mesh:
 *   ADD   = mean_v |E v - G v|                            (Hinterstoisser et al.; what FoundationPose reports the AUC of)
 *   ADD-S = mean_u min_v |G u - E v|                      (the symmetric form: every ground-truth point to the NEAREST estimated point)
 *   MSSD  = min_s max_v |E v - G S_s v|                   (BOP: maximum symmetry-aware surface distance)
 *   MSPD  = min_s max_v |proj(E v) - proj(G S_s v)|       (BOP: ... projection distance, pixels, with the model's K)
 * Symmetries: S column-major 4x4 matrices in the MESH frame (NOT centred), already discretised, as BOP's models_info.json has them;
 * the library conjugates them with the target's centre on the host in double, x' = R_s (x + c) + t_s - c.  The identity is always
 * symmetry 0 and the caller's set follows as 1..S, so best_sym / best_sym_mspd index that combined list; S may be 0 (symmetries may
 * then be NULL).  best_sym is also the answer to "which symmetry-equivalent of G is nearest to E" (a serving loop that must not jump
 * between equivalents).  The composites G S_s are formed on the host in double and rounded to f32; rot_deg / trans_m compare E with
 * G S_best_sym on the host in double.
 * Vertices: 0, vertex_step, 2 vertex_step, ... < V of the target, so n_vertices = Vs = ceil(V / vertex_step); vertex_step >= 1.
 * ADD-S is brute force over Vs^2 point pairs per pose -- exact, no build step -- and is computed only with FP_POSE_ERROR_ADDS.
 * Projection: u = fx * (x / z) + cx, w = fy * (y / z) + cy, every f32 operation separately rounded.  If any used vertex has
 * z < FP_RENDER_NEAR_M under E or under any G S_s, the record gets mspd_px = INFINITY and best_sym_mspd = -1; its other fields
 * are unaffected.
 * Means: each distance d is an f32 and enters a 64-bit integer sum as llrintf(d * 2^20), so a record does not depend on thread order:
 * pose i's record is bit-identical alone, in a batch and from call to call.  add_m = (float)(add_sum_q20 / 2^20 / Vs), in double.
 * Refused with an error before anything is launched and before `out` is written: an unknown target, N outside 1..FP_MAX_BATCH, n_gt
 * not 1 or N, S outside 0..FP_MAX_SYMMETRIES, vertex_step < 1, unknown flag bits, a non-finite entry or a translation component
 * beyond +-1000 m in any matrix, a pending Track, with FP_POSE_ERROR_ADDS more than FP_POSE_ERROR_MAX_PAIRS point pairs N * Vs^2
 * (the message names the smallest vertex_step that fits), and more than FP_POSE_ERROR_MAX_PAIRS / 64 transformed vertex pairs
 * N * (S + 1) * Vs.  The caps keep the largest admitted call near one second of device time; no single launch covers more than a
 * tenth of a cap (the call is split over poses).
 * Needs no frame; works on geometry-only models; stream-ordered behind the model's work on the model's stream, one synchronisation
 * at the end.  Register, Track, their captured graphs and every existing kernel are untouched: the call's buffers are its own,
 * allocated at its first use, grow-only. */
#define FP_POSE_ERROR_ADDS 1          /* flags: also compute ADD-S (the N * Vs^2 part) */
#define FP_MAX_SYMMETRIES 1024
#define FP_POSE_ERROR_MAX_PAIRS 8000000000000LL /* N * Vs^2 of one call with FP_POSE_ERROR_ADDS: 0.84 s at the 9.5e12 pairs/s measured */
typedef struct fp_pose_error {
  float   add_m;          /* mean_v |E v - G v|                                   */
  float   adds_m;         /* mean_u min_v |G u - E v|   (NaN without the flag)    */
  float   mssd_m;         /* min_s max_v |E v - G S_s v|                          */
  float   mspd_px;        /* min_s max_v |proj(E v) - proj(G S_s v)|, model's K   */
  float   rot_deg, trans_m; /* E against G S_best_sym, host, computed in double   */
  int32_t best_sym;       /* arg-min of MSSD, lowest index on ties                */
  int32_t best_sym_mspd;  /* arg-min of MSPD, -1 when mspd_px is INFINITY         */
  int64_t add_sum_q20, adds_sum_q20;  /* the integer sums behind the two means (adds: -1 without the flag) */
  int32_t n_vertices;     /* Vs */
  int32_t reserved;
} fp_pose_error;
int fp_pose_errors(fp_model *m, const char *target_name, const float *est_poses, int N,
                   const float *gt_poses, int n_gt /* 1 or N */,
                   const float *symmetries /* S column-major 4x4, MESH frame; NULL = none */, int S,
                   int vertex_step, int flags, fp_pose_error *out /* host [N] */);

/* ---- visible surface discrepancy: BOP's VSD of N poses against the uploaded frame (new; the reference has no counterpart) ----
 * fp_pose_vsd compares, pixel by pixel, the surface visible under each estimate with the surface visible under its ground truth,
 * given the observed depth: the third of BOP's three errors next to MSSD and MSPD, ambiguity-invariant without a symmetry list.
 * Poses as in fp_pose_errors (column-major 4x4, centred-mesh -> camera; n_gt == 1: every estimate against the one truth).  The frame is
 * the uploaded one (fp_upload_frame, or what the last Register / device-frame Track left), read as the RAW depth whether
 * fp_set_depth_filter is on or off; K is the model's.  DESIGN.md section 4.11 has the rules; in short, per pixel (c, r):
 *   z_e, z_g   exactly fp_render_pose's model_depth of the estimate and of the truth
 *   q = sqrtf((X * X + Y * Y) + 1), X = ((float)c - cx) / fx, Y = ((float)r - cy) / fy;  d_t = D * q, d_e = z_e * q, d_g = z_g * q
 *              (BOP compares distances from the camera centre, not z; D the observed depth; every f32 operation separately rounded)
 *   hidden(d)  = !(D < 0.001f) && (d - d_t) > delta_m             (missing depth, and NaN, hide nothing)
 *   vis_g = model_g && !hidden(d_g);   vis_e = model_e && (!hidden(d_e) || vis_g)
 *   on vis_g && vis_e the pixel fails threshold t when fabsf(d_g - d_e) >= thr_t, thr_t = taus[t] (* the target's diameter, one f32
 *              product, with FP_VSD_NORMALIZED)
 *   vsd[t] = (n_fail[t] + n_union - n_inter) / n_union: BOP's step cost (the tau-linear cost is not built)
 * Every field but vsd is an integer pixel count, so pose i's record is byte-identical alone, in any batch, with n_gt == 1 or N copies
 * of the truth, and from call to call.
 * A refused pose (a vertex at z < FP_RENDER_NEAR_M, or beyond FP_RENDER_SNAP_MAX: fp_render_pose would fail) does not fail the call:
 * its record gets the status bit, all counts 0 and vsd[t] = 1 for t < T; the same for the truth of a pair when n_gt == N.  With
 * n_gt == 1 a refused truth fails the whole call before `out` is written.
 * Refused with an error before anything is launched and before `out` is written: an unknown target, N outside 1..FP_MAX_BATCH, n_gt
 * not 1 or N, T outside 1..FP_VSD_MAX_TAUS, a tau or delta_m that is not finite or is negative, unknown flag bits, a non-finite
 * matrix entry, no frame, a partial frame, a pending Track, and more than FP_VSD_MAX_WORK faces walked: the sum over the call's
 * (pose, 32 x 32 px tile) items -- the tiles of the union of the screen bounds of an estimate and its truth -- of the faces each walks
 * (F, or 2 F when n_gt == N), plus the truth's own tiles once when n_gt == 1.  No single launch covers more than a tenth of it.
 * Works on geometry-only models; stream-ordered on the model's stream; Register, Track, their captured graphs and every existing
 * kernel are untouched: the call's buffers are its own, allocated at its first use, grow-only. */
#define FP_VSD_MAX_TAUS 16
#define FP_VSD_NORMALIZED 1          /* flags: taus are fractions of the target's diameter (BOP19: yes) */
#define FP_VSD_EST_REFUSED_NEAR 1    /* status bits of a record */
#define FP_VSD_EST_REFUSED_RANGE 2
#define FP_VSD_GT_REFUSED_NEAR 4
#define FP_VSD_GT_REFUSED_RANGE 8
#define FP_VSD_MAX_WORK 250000000000LL /* faces walked by one call: 0.96 s at the 2.6e11 faces/s measured for 252 poses */
typedef struct fp_pose_vsd {
  int32_t n_model_est, n_model_gt;   /* frame pixels the rendering covers (before visibility) */
  int32_t n_visib_est, n_visib_gt;
  int32_t n_inter, n_union;          /* of the two visibility masks */
  int32_t n_fail[FP_VSD_MAX_TAUS];   /* intersection pixels with |dist_gt - dist_est| >= threshold t; entries >= T are 0 */
  float   vsd[FP_VSD_MAX_TAUS];      /* (n_fail[t] + n_union - n_inter) / n_union, in double, rounded once; 1.0 when n_union == 0; entries >= T are NaN */
  int32_t status, reserved;
} fp_pose_vsd_t; /* (C keeps typedef names and functions in one name space: the record is `struct fp_pose_vsd` or fp_pose_vsd_t) */
int fp_pose_vsd(fp_model *m, const char *target_name, const float *est_poses, int N,
                const float *gt_poses, int n_gt /* 1 or N */, float delta_m,
                const float *taus, int T, int flags, fp_pose_vsd_t *out /* host [N] */);

/* ---- depth refinement: projective point-to-plane ICP of N poses on the uploaded frame's depth (new; the reference has no counterpart) ----
 * fp_refine_depth improves N poses of one target from the depth the model already holds: each iteration renders every pose at frame
 * resolution (so self-occlusion is exact), associates each model pixel with the observed depth at the same pixel, sums the 6 x 6
 * point-to-plane normal system on the device in integers and solves it on the host in double.  Poses as in fp_pose_errors (column-major
 * 4x4, centred-mesh -> camera); the frame is the uploaded one, read as the RAW depth whether fp_set_depth_filter is on or off; K is the
 * model's.  DESIGN.md section 4.12 has the rules; in short, per pixel (c, r) of a pose with translation t:
 *   z, triangle  exactly fp_render_pose's model_depth and tri_id; n^ the unit normal of the triangle's camera-space corners (fp_render_pose's
 *                shading normal, divided by its length; a triangle without one is never used)
 *   X = ((float)c - cx) / fx, Y = ((float)r - cy) / fy, l = sqrtf((X * X + Y * Y) + 1), s = (n^x * X + n^y * Y) + n^z, dz = D - z
 *   valid    D >= 0.001f and finite;  front  dz * l < -max_dist_m (an occluder);  behind  dz * l > max_dist_m;
 *   grazing  neither, and fabsf(s) / l < FP_ICP_MIN_COS;  used  otherwise
 *   used:    rad = diameter * 0.5f, e = (dz * s) / rad, q = (D * X, D * Y, D), qc = (q - t) / rad, J = (qc x n^, n^)
 *   the 28 products J_i J_j (i <= j), J_i e, e e are one f32 multiplication each and enter 64-bit sums as llrintf(v * 2^32)
 * (every f32 operation separately rounded), so pose i's record and pose are byte-identical alone, in any batch and from call to call.
 * Per iteration the host solves (sum J J^T) xi = sum J e, xi = (omega, upsilon / rad), by a Jacobi eigen-decomposition in double, moves
 * only along eigen-directions with lambda >= FP_ICP_RANK_EPS * lambda_max, and applies R <- exp(omega) R, t <- t + upsilon (the twist
 * about the object's origin).  FP_ICP_TRANSLATION_ONLY solves the 3 x 3 translation block alone (a symmetric object's rotation about
 * its axis would follow the noise).  `iterations` = I allows at most I updates and I + 1 evaluations; I = 0 measures the fit only.
 * A pose stops when its update is below both epsilons (FP_ICP_CONVERGED; the update is applied, and the pose is evaluated once more
 * unless its f32 form did not change), when fewer than FP_ICP_MIN_PIXELS pixels are used (FP_ICP_TOO_FEW, no update), or when
 * fp_render_pose would refuse the updated pose (the status bit; the pose before that update and its record are returned, `iterations`
 * does not count it).  The record always describes the returned pose.
 * A pose refused at the input does not fail the call: its output equals its input, its counts are 0, its status bit is set.
 * Refused with an error before anything is launched and before the outputs are written: an unknown target, N outside 1..FP_MAX_BATCH,
 * iterations outside 0..FP_ICP_MAX_ITERATIONS, max_dist_m not finite, <= 0 or above the target's diameter, unknown flag bits, a
 * non-finite matrix entry, no frame, a partial frame, a frame of 2^26 pixels or more, a pending Track, and more than FP_ICP_MAX_WORK
 * faces walked: (iterations + 1) times the sum over the input poses' (pose, 32 x 32 px tile) items of F.  No launch covers more than a
 * tenth of it.  Works on geometry-only models; stream-ordered on the model's stream with one synchronisation per evaluation; Register,
 * Track, their captured graphs and every existing kernel are untouched: the call's buffers are its own, grow-only. */
#define FP_ICP_MAX_ITERATIONS 32
#define FP_ICP_TRANSLATION_ONLY 1        /* flags: solve the 3 x 3 translation block only (symmetric objects) */
#define FP_ICP_MIN_COS 0.2f              /* a pixel whose surface is seen at more than ~78 deg from its normal is not used */
#define FP_ICP_MIN_PIXELS 32             /* fewer used pixels: the pose stops */
#define FP_ICP_EPS_ROT_RAD 1e-5f
#define FP_ICP_EPS_TRANS_M 1e-6f         /* an update below both: converged, the pose stops */
#define FP_ICP_RANK_EPS 1e-8             /* an eigen-direction with lambda < eps * lambda_max is not moved along */
#define FP_ICP_MAX_WORK 280000000000LL /* faces walked by one call: 0.99 s at the 2.84e11 faces/s measured for 252 poses */
#define FP_ICP_CONVERGED 1               /* status bits of a record */
#define FP_ICP_TOO_FEW 2
#define FP_ICP_REFUSED_NEAR 4            /* fp_render_pose would refuse the pose (at the input, or after an update) */
#define FP_ICP_REFUSED_RANGE 8
typedef struct fp_depth_refine {
  int32_t n_model, n_valid, n_used, n_front, n_behind, n_grazing;  /* frame pixels; n_valid == n_used + n_front + n_behind + n_grazing */
  int32_t iterations;      /* updates applied to this pose */
  int32_t rank;            /* directions kept by the last solve (0 when none was made) */
  int32_t status, reserved;
  float   rms_m;           /* sqrt(sum e^2 / n_used) * (diameter / 2) at the RETURNED pose; 0 when n_used == 0 */
  float   cond;            /* lambda_min / lambda_max of the last solve (0 when none was made) */
  float   last_rot_rad, last_trans_m;   /* size of the last solve's update */
  int64_t sums_q32[28];    /* at the RETURNED pose: 21 upper-triangle entries of sum J J^T (row-major), 6 of sum J e, sum e^2 */
} fp_depth_refine_t;
int fp_refine_depth(fp_model *m, const char *target_name, const float *poses, int N, int iterations /* 0..32 */,
                    float max_dist_m, int flags, float *out_poses /* host [N*16] */, fp_depth_refine_t *out /* host [N] */);

/* ---- depth search: N poses ranked by the uploaded frame's depth alone (new; the reference has no counterpart) ----
 * fp_pose_search tests N poses of one target against the depth the model already holds, each at n_steps pushes along the ray of its own
 * origin, and returns per pose the counts at its best step.  Poses as in fp_pose_errors (column-major 4x4, centred-mesh -> camera); the
 * frame is the uploaded one, read as the RAW depth whether fp_set_depth_filter is on or off; K is the model's.  DESIGN.md section 4.13
 * has the rules; every f32 operation is separately rounded:
 *   points   the centred vertices 0, vertex_step, 2 vertex_step, ... with their vertex normals as loaded (not renormalised):
 *            P = ceil(V / vertex_step) <= FP_SEARCH_MAX_POINTS
 *   step k   of pose (R, t), k = 0 .. n_steps - 1: s_k = (float)k * step_m, t_k = (t.x + s_k * (t.x / t.z), t.y + s_k * (t.y / t.z), t.z + s_k)
 *   point    q = R p + t_k, n' = R n, each component ((r0 * x + r1 * y) + r2 * z) + t in that order.  q.z < FP_RENDER_NEAR_M for ANY point
 *            refuses that (pose, step): it competes with no score
 *   facing   a = -((n'.x * q.x + n'.y * q.y) + n'.z * q.z); a > 0 and a * a > 0.04f * ((q.x * q.x + q.y * q.y) + q.z * q.z).  Only facing
 *            points are counted
 *   pixel    uf = rintf(fx * (q.x / q.z) + cx), vf = rintf(fy * (q.y / q.z) + cy); outside unless 0 <= uf <= W - 1 and 0 <= vf <= H - 1,
 *            compared as floats (a NaN or a huge value is outside; nothing is read out of bounds)
 *   class    D the depth at (uf, vf): missing unless D >= 0.001f and finite; dz = D - q.z; inlier fabsf(dz) <= tol_m, front dz < -tol_m
 *            (an occluder), behind dz > tol_m (the pose claims a surface where the camera saw through)
 *   score    n_inlier - n_behind - n_outside; best_step is its arg-max over the steps that were not refused, the lowest step on ties
 * Everything is an integer count, so pose i's record is byte-identical alone, in any batch and from call to call.  A pose whose steps
 * were all refused does not fail the call: its counts and score are 0, best_step is -1, status is FP_SEARCH_REFUSED_NEAR.
 * Refused with an error before anything is launched and before `out` is written: an unknown target, N outside 1..FP_MAX_BATCH, n_steps
 * outside 1..FP_SEARCH_MAX_STEPS, step_m not finite or negative, tol_m not finite or <= 0, vertex_step < 1 or P above the cap (the message
 * names the smallest step that fits), a non-finite matrix entry, t.z < FP_RENDER_NEAR_M, no frame, a partial frame, a pending Track.
 * Works on geometry-only models; stream-ordered on the model's stream with one synchronisation at the end; Register, Track, their
 * captured graphs and every existing kernel are untouched: the call's buffers are its own, grow-only. */
#define FP_SEARCH_MAX_POINTS 4096
#define FP_SEARCH_MAX_STEPS 64
#define FP_SEARCH_REFUSED_NEAR 1         /* status: every step of the pose had a point nearer than FP_RENDER_NEAR_M */
typedef struct fp_pose_search {
  int32_t n_facing, n_inlier, n_front, n_behind, n_outside, n_missing; /* at best_step; n_facing == the sum of the other five */
  int32_t score;       /* n_inlier - n_behind - n_outside at best_step */
  int32_t best_step;   /* arg-max of score over the steps, lowest step on ties; -1 when every step was refused */
  int32_t n_points;    /* P */
  int32_t status;      /* FP_SEARCH_REFUSED_NEAR when every step was refused */
} fp_pose_search_t;
int fp_pose_search(fp_model *m, const char *target_name, const float *poses, int N,
                   int n_steps, float step_m, float tol_m, int vertex_step,
                   fp_pose_search_t *out /* host [N] */);

/* ---- Register without weights: depth search over the hypothesis grid, then fp_refine_depth on the best candidates (new) ----
 * fp_register_depth finds the pose of a target from the depth and the mask alone.  It composes calls of this header and gives, byte for
 * byte, what they give when called one after the other:
 *   1. the frame is uploaded as by fp_register_ex and the sampler runs on the mask: the N = fp_num_hypotheses() poses of
 *      fp_get_hyp_poses (fp_set_inplane_steps sets the density).  The sampler's errors (empty mask, no valid depth) are this call's.
 *   2. fp_pose_search over them: n_steps = 9, step_m = diameter / 16 (one f32 division), tol_m, the smallest vertex_step with P <= 1024
 *   3. candidates: the top_k poses by score, ties to the lower hypothesis index, refused poses dropped; each moved to its best step's t_k
 *   4. fp_refine_depth on the candidates: gate min(4 * tol_m, diameter), icp_iterations, no flags
 *   5. the winner: among candidates without a REFUSED or TOO_FEW status bit the largest n_used - n_behind, ties to the smaller
 *      sums_q32[27] (sum e^2), then to the lower hypothesis index.  No candidate left: the call fails and says so; out_pose is not written.
 * top_k = 0 means 16 (at most 64), tol_m = 0 means 0.005, icp_iterations = 0 means 15 (at most FP_ICP_MAX_ITERATIONS).  The frame stays
 * uploaded as after a Register, so fp_render_pose, fp_pose_vsd and fp_refine_depth can follow.  Works with NULL weights; takes the
 * guards of the calls it composes; never touches the networks or a captured graph.  A symmetric object's answer is one of its
 * equivalent poses. */
#define FP_REGISTER_DEPTH_MAX_TOP_K 64
typedef struct fp_depth_register {
  int32_t hypothesis;        /* index into the fp_get_hyp_poses grid of the returned pose's start */
  int32_t n_hypotheses, n_candidates;   /* searched; refined */
  int32_t rank_key;          /* n_used - n_behind of the winner */
  fp_pose_search_t search;   /* the winner's search record */
  fp_depth_refine_t refine;  /* the winner's fp_refine_depth record */
} fp_depth_register_t;
int fp_register_depth(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                      const char *target_name, int top_k /* 0 = 16, at most 64 */, float tol_m /* 0 = 0.005 */,
                      int icp_iterations /* 0 = 15, at most FP_ICP_MAX_ITERATIONS */,
                      float out_pose[16], fp_depth_register_t *out /* may be NULL */);

/* ---- colour agreement: does the picture agree with N poses? (new; the reference has no counterpart) ----
 * fp_pose_color compares, over the visible model pixels of each pose, the model's UNSHADED colour with the uploaded frame's RGB: the only
 * frame-resolution call that reads the colour.  Poses as in fp_pose_errors (column-major 4x4, centred-mesh -> camera); the frame is the
 * uploaded one, its RGB and its RAW depth whether fp_set_depth_filter is on or off; K is the model's (a plain pinhole matrix).  The
 * colour source is the target's current one: the texture, or the vertex colours after fp_set_vertex_colors.  DESIGN.md section 4.14 has
 * the rules; every f32 operation is separately rounded.  Per pixel (c, r) of a pose:
 *   triangle, z  exactly fp_render_pose's tri_id and model_depth; n_model counts these pixels
 *   visible      !(D >= 0.001f && D < z - tol_m), fp_render_pose's visible_mask (missing depth, and NaN, hide nothing); n_visible
 *   weights      a, b, c the winning triangle's snapped corners, e_0 e_1 e_2 its edge functions at (16 c, 16 r) and A its doubled area,
 *                all exact integers as the rasteriser forms them: w_k = (float)e_k / (float)A, g_k = (w_k / z_k) * z, z_k the corner depths
 *   texture      U = (g_0 * u_0 + g_1 * u_1) + g_2 * u_2, V likewise from the stored (u, 1 - v); fu = U - floorf(U);
 *                tx = min((int)(fu * (float)TW), TW - 1), ty likewise with TH: the nearest texel, with wrap.  A U or V that is not finite
 *                gives the pixel no colour (n_nocolor): it is not compared and nothing is read
 *   vertex col.  per channel v = (g_0 * c_0 + g_1 * c_1) + g_2 * c_2, c_k the corner's byte as float; the model's value is
 *                (int)rintf(fminf(fmaxf(v, 0), 255)); a NaN in any channel gives the pixel no colour
 *   compared     the visible pixels with a colour (n_compared): per channel R, G, B the exact integer sums of m, o, m m, o o and m o, m the
 *                model's value and o the frame's byte, both 0..255
 * On the host, in double, with n = n_compared: cov = sum_ch (sum_mo - sum_m sum_o / n), var_m = sum_ch (sum_mm - sum_m^2 / n), var_o
 * likewise, zncc = cov / sqrt(var_m var_o), rounded once.  The means are removed per channel and the gain is shared, so an illumination
 * gain, or an offset per channel, leaves the value as it is.  zncc is 0 with FP_COLOR_TOO_FEW when n < FP_COLOR_MIN_PIXELS, and 0 with
 * FP_COLOR_FLAT when either variance is <= 0 (the 2 x 2 grey default texture is this case).
 * Everything but zncc is an integer count or sum, so pose i's record is byte-identical alone, in any batch and from call to call.
 * A refused pose (a vertex at z < FP_RENDER_NEAR_M, or beyond FP_RENDER_SNAP_MAX: fp_render_pose would fail) does not fail the call:
 * its counts and sums are 0, its zncc is 0, its status bit is set.
 * Refused with an error before anything is launched and before `out` is written: an unknown target, N outside 1..FP_MAX_BATCH, a tol_m
 * that is not finite or is negative, a non-finite matrix entry, no frame, a partial frame, a frame of 2^26 pixels or more, a pending
 * Track, and more than FP_COLOR_MAX_WORK faces walked: the sum over the poses' (pose, 32 x 32 px tile) items of F.  No launch covers
 * more than a tenth of it.  Stream-ordered on the model's stream with one synchronisation at the end; Register, Track, their captured
 * graphs and every existing kernel are untouched: the call's buffers are its own, allocated at its first use, grow-only. */
#define FP_COLOR_MIN_PIXELS 32
#define FP_COLOR_REFUSED_NEAR 1      /* status bits of a record */
#define FP_COLOR_REFUSED_RANGE 2
#define FP_COLOR_TOO_FEW 4           /* n_compared < FP_COLOR_MIN_PIXELS */
#define FP_COLOR_FLAT 8              /* the model's or the frame's values have no variance over the compared pixels */
#define FP_COLOR_MAX_WORK 330000000000LL /* faces walked by one call: 0.99 s at the 3.32e11 faces/s measured for 252 poses */
typedef struct fp_pose_color {
  int32_t n_model, n_visible, n_compared, n_nocolor;   /* frame pixels; n_visible == n_compared + n_nocolor */
  int32_t status, reserved;
  int64_t sum_m[3], sum_o[3], sum_mm[3], sum_oo[3], sum_mo[3];  /* per channel R, G, B over the compared pixels */
  float   zncc;            /* host, double, rounded once; 0 when a status bit is set */
  float   reserved_f;
} fp_pose_color_t;
int fp_pose_color(fp_model *m, const char *target_name, const float *poses, int N, float tol_m,
                  fp_pose_color_t *out /* host [N] */);

/* ---- symmetry resolution: which equivalent of a pose does the picture show? (new) ----
 * fp_resolve_symmetry takes a pose of a symmetric object -- fp_register_depth's answer is one of its equivalents -- and returns the
 * equivalent whose colour agrees best with the frame.  It composes calls of this header and gives, byte for byte, what they give:
 *   1. the equivalents E_s = pose * S'_s, s = 0..S: symmetry 0 is the identity (E_0 is `pose` bit for bit), the caller's S column-major
 *      4x4 matrices of the MESH frame follow as 1..S, conjugated with the target's centre exactly as fp_pose_errors conjugates them;
 *      formed on the host in double, rounded to f32 once; the fourth row is that of `pose`
 *   2. fp_pose_color over the S + 1 equivalents with tol_m
 *   3. the winner: the largest zncc among the records with status 0, ties to the lower index.  No record with status 0 (an untextured
 *      model ends here): the call fails and says so; out_pose and best_sym are not written.
 * S in 0..FP_MAX_SYMMETRIES (symmetries may be NULL when S is 0); a non-finite entry or a translation beyond +-1000 m in a symmetry is
 * refused as by fp_pose_errors; otherwise the call takes the guards of the call it composes.  Continuous symmetries arrive discretised,
 * as BOP's models_info.json has them.  records, when not NULL, receives the S + 1 records of step 2. */
int fp_resolve_symmetry(fp_model *m, const char *target_name, const float pose[16],
                        const float *symmetries /* S column-major 4x4, MESH frame; NULL = none */, int S,
                        float tol_m, float out_pose[16], int *best_sym /* may be NULL */,
                        fp_pose_color_t *records /* host [S + 1], may be NULL */);

/* ---- silhouette agreement: does the segmentation mask agree with N poses? (new; the reference has no counterpart) ----
 * fp_pose_silhouette compares, over the pixels of each pose, the model's (visible) silhouette with a mask of the uploaded frame, and
 * weighs every pixel of disagreement with its exact squared Euclidean distance to the other side of the mask's outline.  Poses as in
 * fp_pose_errors (column-major 4x4, centred-mesh -> camera); the frame is the uploaded one, its RAW depth whether fp_set_depth_filter is on
 * or off; K is the model's (a plain pinhole matrix).  DESIGN.md section 4.15 has the rules.  The only f32 arithmetic is fp_render_pose's;
 * everything new is integer.
 *   mask         u8 [H, W] in `memspace`, H and W the uploaded frame's; a pixel is a MASK pixel when its byte is > 0 (the convention of
 *                fp_register's mask).  The caller's mask is never modified.
 *   distance     for a seed set S, d2_S(r, c) = min over (r', c') in S of (r - r')^2 + (c - c')^2: an exact integer, FP_SIL_D2_NONE when S
 *                is empty; nothing outside the frame is a seed.  d2_to_mask has S = the mask pixels (0 on the mask), d2_to_bg has S = the
 *                other pixels (0 off the mask, >= 1 on it).  fp_mask_distance returns the two maps (u32 [H, W], host; either may be NULL).
 * Per pixel of a pose:
 *   model, z     exactly fp_render_pose's model_mask and model_depth; n_model counts these pixels
 *   visible      !(D >= 0.001f && D < z - tol_m) on the raw depth, fp_render_pose's visible_mask; with FP_SIL_AMODAL simply `model`, and the
 *                depth is not read; n_visible
 *   inter        visible and mask (n_inter);   spill: visible and not mask (n_spill)
 *   clip(v)      min(v, trunc_px * trunc_px) when trunc_px > 0, else v
 * Per record: n_mask the mask pixels of the frame (the same in every record of a call), n_miss = n_mask - n_inter,
 *   sum_spill_d2 = sum of clip(d2_to_mask) over the spill pixels,
 *   sum_miss_d2  = T - sum of clip(d2_to_bg) over the inter pixels, T = the sum of clip(d2_to_bg) over all mask pixels (once per call): the
 *                  sum over the mask pixels the pose does not explain, weighted by how deep inside the mask they lie.
 * On the host, in double, rounded once: iou = n_inter / (n_mask + n_spill), rms_spill_px = sqrt(sum_spill_d2 / n_spill), rms_miss_px =
 * sqrt(sum_miss_d2 / n_miss); each is 0 when its denominator is 0.  FP_SIL_EMPTY is set when n_mask + n_spill == 0.
 * Every field is an integer or a host formula of integers, so pose i's record is byte-identical alone, in any batch, under any chunking
 * and from call to call.  A refused pose (a vertex at z < FP_RENDER_NEAR_M, or beyond FP_RENDER_SNAP_MAX: fp_render_pose would fail) does
 * not fail the call: its status bit is set and every other field is 0.
 * Refused with an error before anything is launched and before `out` is written: NULL arguments, a memspace that is neither FP_HOST nor
 * FP_DEVICE, N outside 1..FP_MAX_BATCH, a tol_m that is not finite or is negative (also with FP_SIL_AMODAL), trunc_px outside
 * 0..FP_SIL_MAX_TRUNC_PX, unknown flag bits, a pending Track, a K that is not a plain pinhole matrix, an unknown target, a non-finite
 * matrix entry, no frame, a partial frame, H or W above FP_SIL_MAX_DIM, and more than FP_SIL_MAX_WORK faces walked: the sum over the
 * poses' (pose, 32 x 32 px tile) items of F, as fp_pose_color counts them.  No launch covers more than a tenth of it.  fp_mask_distance
 * takes the pointer, memspace, camera, frame and dimension guards only.  Both work on geometry-only models, are stream-ordered on the model's stream with
 * one synchronisation at the end, and leave Register, Track, their captured graphs and every existing kernel untouched: the calls'
 * buffers (mask copy, the two maps, the column distances, the accumulators) are their own, allocated at first use, grow-only. */
#define FP_SIL_AMODAL 1              /* flags: every model pixel counts as visible; the depth is not read */
#define FP_SIL_D2_NONE 0x7fffffff    /* squared distance where the seed set is empty */
#define FP_SIL_MAX_DIM 8192          /* H and W of the frame, for these two calls */
#define FP_SIL_MAX_TRUNC_PX 32767
#define FP_SIL_REFUSED_NEAR 1        /* status bits of a record; 1 and 2 are the vertex rule's, as in fp_pose_color */
#define FP_SIL_REFUSED_RANGE 2
#define FP_SIL_EMPTY 4               /* n_mask + n_spill == 0 */
#define FP_SIL_MAX_WORK 340000000000LL /* faces walked by one call: 0.99 s at the 3.43e11 faces/s measured for 252 poses */
typedef struct fp_pose_silhouette {
  int32_t n_model, n_visible, n_inter, n_spill;   /* pixels of the pose; n_visible == n_inter + n_spill */
  int32_t n_mask, n_miss;                         /* mask pixels of the frame; n_mask - n_inter */
  int32_t status, reserved;
  int64_t sum_spill_d2, sum_miss_d2;
  float   iou, rms_spill_px, rms_miss_px;         /* host, double, rounded once */
  float   reserved_f;
} fp_pose_silhouette_t;
int fp_mask_distance(fp_model *m, const void *mask, int memspace,
                     uint32_t *d2_to_mask, uint32_t *d2_to_bg /* host [H,W]; either may be NULL, not both */);
int fp_pose_silhouette(fp_model *m, const char *target_name, const void *mask, int memspace,
                       const float *poses, int N, float tol_m, int trunc_px, int flags,
                       fp_pose_silhouette_t *out /* host [N] */);

/* ---- silhouette refinement: N poses moved onto the mask's outline, no depth needed (new; the reference has no counterpart) ----
 * fp_refine_silhouette improves N poses of one target from a mask of the uploaded frame alone: each iteration renders every pose at
 * frame resolution, takes the pixels of the pose's own outline, reads at each the signed distance to the mask's outline and its gradient,
 * sums the 6 x 6 normal system of "move the outline onto the mask's" on the device in integers and solves it on the host in double.
 * Poses, mask, memspace, K and the frame guards are fp_pose_silhouette's; the iteration protocol is fp_refine_depth's.  DESIGN.md section
 * 4.16 has the rules; in short (every f32 operation separately rounded):
 *   signed map   once per call, from fp_mask_distance's two maps: sd(r, c) = mask ? -d2_to_bg : d2_to_mask (an i32, never 0);
 *                psi = sd > 0 ? sqrtf((float)sd) : sd == 0 ? 0 : 1 - sqrtf((float)(-sd)): 0 on the mask's own contour pixels, 1 on the
 *                first ring outside, negative inside.  A mask that is empty or covers the whole frame fails the call.
 *   contour      a model pixel (fp_render_pose's model_mask, z its model_depth) with at least one of its four neighbours INSIDE the frame
 *                that is not a model pixel (a neighbour outside the frame is not background)
 *   classes      of a contour pixel, tested in this order:  occluded  only with FP_SILREF_OCCLUSION: D >= 0.001f && D < z - tol_m on the raw
 *                depth;  far  gate_px > 0 and |sd| > gate_px * gate_px;  flat  gx == 0 && gy == 0, with
 *                gx = (psi(r, min(c + 1, W - 1)) - psi(r, max(c - 1, 0))) * 0.5f and gy likewise over rows;  steep  one of J, e below is a
 *                NaN or above FP_SILREF_MAX_TERM in magnitude;  used  otherwise.  n_contour is the sum of the five.
 *   per pose     (host, f32) rad = diameter * 0.5f, s = (fx * rad) / t.z (the radius in pixels), kx = (fx * rad) / s, ky = (fy * rad) / s;
 *                a pose with !(t.z >= FP_RENDER_NEAR_M) is refused like one with such a vertex
 *   used:        X = ((float)c - cx) / fx, Y = ((float)r - cy) / fy, a = ((gx * kx) / z, (gy * ky) / z, -(ax * X + ay * Y)),
 *                pc = ((z * X - t.x) / rad, (z * Y - t.y) / rad, (z - t.z) / rad), J = (pc x a, a), e = -psi / s
 *   the 28 products J_i J_j (i <= j), J_i e, e e are one f32 multiplication each and enter 64-bit sums as llrintf(v * 2^24)
 * so pose i's record and pose are byte-identical alone, in any batch, under any chunking and from call to call.  Per iteration the host
 * solves (sum J J^T) xi = sum J e as fp_refine_depth does (the same decomposition, the same FP_ICP_RANK_EPS), scales the whole xi by
 * min(1, FP_SILREF_MAX_STEP_RAD / |omega|, 0.5 / |upsilon / rad|), and applies R <- exp(omega) R, t <- t + upsilon.
 * FP_SILREF_TRANSLATION_ONLY solves the 3 x 3 translation block alone: an outline that a rotation or a change of depth does not move
 * (a sphere's, an ellipsoid's about its axis) does not determine them.  `iterations` = I allows at most I updates and I + 1 evaluations;
 * I = 0 measures only.  A pose stops when its update BEFORE the scaling is below both epsilons (FP_SILREF_CONVERGED; the update is applied,
 * and the pose is evaluated once more unless its f32 form did not change), when fewer than FP_SILREF_MIN_PIXELS pixels are used
 * (FP_SILREF_TOO_FEW, no update), or when fp_render_pose would refuse the updated pose (the status bit; the pose before that update and
 * its record are returned, `iterations` does not count it).  The record always describes the returned pose.  A pose refused at the input
 * does not fail the call: its output equals its input, its counts are 0, its status bit is set.  There is no depth term: chain
 * fp_refine_depth afterwards where the depth is good.
 * Refused with an error before anything is launched and before the outputs are written: everything fp_pose_silhouette refuses (tol_m is
 * checked with and without FP_SILREF_OCCLUSION; gate_px in the place of trunc_px), iterations outside 0..FP_SILREF_MAX_ITERATIONS, and
 * more than FP_SILREF_MAX_WORK faces walked: (iterations + 1) times the sum over the input poses' (pose, 32 x 32 px tile) items of F.  No
 * launch covers more than a tenth of it.  An empty or full mask fails the call after the distance transform, before the outputs are
 * written.  Works on geometry-only models; stream-ordered on the model's stream with one synchronisation per evaluation; Register, Track,
 * their captured graphs and every existing kernel are untouched: the call's buffers are its own or fp_pose_silhouette's, grow-only. */
#define FP_SILREF_MAX_ITERATIONS 32
#define FP_SILREF_TRANSLATION_ONLY 1     /* flags: solve the 3 x 3 translation block only (symmetric outlines) */
#define FP_SILREF_OCCLUSION 2            /* flags: drop the contour pixels that fp_render_pose would call occluded (reads the depth) */
#define FP_SILREF_MAX_TERM 64.0f         /* a pixel with |J_i| or |e| above it is steep, not used: no sum can reach 2^62 */
#define FP_SILREF_MAX_STEP_RAD 0.2       /* the update is scaled down to at most this rotation ... */
#define FP_SILREF_MAX_STEP_RADII 0.5     /* ... and at most this translation, in object radii */
#define FP_SILREF_MIN_PIXELS 16          /* fewer used pixels: the pose stops */
#define FP_SILREF_EPS_ROT_RAD FP_ICP_EPS_ROT_RAD
#define FP_SILREF_EPS_TRANS_M FP_ICP_EPS_TRANS_M
#define FP_SILREF_MAX_WORK 250000000000LL /* faces walked by one call: 1.00 s at the 2.50e11 faces/s measured for 252 poses */
#define FP_SILREF_CONVERGED 1            /* status bits of a record, as FP_ICP_* */
#define FP_SILREF_TOO_FEW 2
#define FP_SILREF_REFUSED_NEAR 4
#define FP_SILREF_REFUSED_RANGE 8
typedef struct fp_silhouette_refine {
  int32_t n_model, n_contour, n_used, n_occluded, n_far, n_flat, n_steep;  /* frame pixels; n_contour is the sum of the five after it */
  int32_t iterations;      /* updates applied to this pose */
  int32_t rank;            /* directions kept by the last solve (0 when none was made) */
  int32_t status;
  float   rms_px;          /* sqrt(sum e^2 / n_used) * scale_px at the RETURNED pose; 0 when n_used == 0 */
  float   scale_px;        /* s, the object's radius in pixels at the returned pose */
  float   cond;            /* lambda_min / lambda_max of the last solve (0 when none was made) */
  float   last_rot_rad, last_trans_m;   /* size of the last update as applied (after the scaling) */
  float   reserved_f;
  int64_t sums_q24[28];    /* at the RETURNED pose: 21 upper-triangle entries of sum J J^T (row-major), 6 of sum J e, sum e^2 */
} fp_silhouette_refine_t;
int fp_refine_silhouette(fp_model *m, const char *target_name, const void *mask, int memspace,
                         const float *poses, int N, int iterations /* 0..32 */, int gate_px /* 0 = none, else 1..FP_SIL_MAX_TRUNC_PX */,
                         float tol_m, int flags, float *out_poses /* host [N*16] */, fp_silhouette_refine_t *out /* host [N] */);

/* ---- stage-level operators (what the reference's orchestrator calls; used by the parity tests) ---- */

/* UploadDataToDevice + convert_depth_to_xyz_map (src/foundationpose.cpp:267-315, src/foundationpose_utils.cu:3-32). */
int fp_upload_frame(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W);
/* optional readback of the xyz map [H,W,3] f32 (pixels with depth < 0.001 are 0). */
int fp_get_xyz_map(fp_model *m, float *xyz_host);

/* FoundationPoseSampler::GetHypPoses (src/foundationpose_sampling.hpp:18-22, .cpp:344-394) on the uploaded frame.
 * poses_out: host [fp_num_hypotheses()*16]. Fails on empty mask / no valid depth like the reference (.cpp:269,278). */
int fp_get_hyp_poses(fp_model *m, const void *mask, int memspace, float *poses_out, int *n_out);
/* erode_depth / bilateral_filter_depth (src/foundationpose_sampling.cu:172-204) on the uploaded frame; host outputs [H,W]. */
int fp_filter_depth(fp_model *m, float *eroded_out, float *bilateral_out);

/* FoundationPoseRenderer::RenderAndTransform (src/foundationpose_render.hpp:29-37, .cpp:814-857):
 * poses host [N*16]; render_out / transf_out: [N,160,160,6] f32 NHWC in `out_memspace` (either may be NULL). */
int fp_render_and_transform(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio,
                            float *render_out, float *transf_out, int out_memspace);
/* debug view of the rasteriser (CR::CudaRaster colour buffer + nvdiffrast rast_out, src/foundationpose_render.cu:184-232):
 * tri_id host [N,160,160] i32 (triangle index+1, raster/y-up order), rast_out host [N,160,160,4] f32; either may be NULL. */
int fp_debug_rasterize(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio,
                       int32_t *tri_id, float *rast_out);

/* refiner_core_->SyncInfer (src/foundationpose.cpp:206-208; blobs :78-81): inputs [N,160,160,6] f32 NHWC,
 * outputs host trans[N,3], rot[N,3]. */
int fp_refiner_infer(fp_model *m, const float *render_input, const float *transf_input, int memspace, int N,
                     float *trans_out, float *rot_out);
/* scorer_core_->SyncInfer (src/foundationpose.cpp:218-220; blob :83): outputs host scores[N]. */
int fp_scorer_infer(fp_model *m, const float *render_input, const float *transf_input, int memspace, int N,
                    float *scores_out);
/* RefinePostProcess (src/foundationpose.cpp:360-406): host in/out. */
int fp_refine_post_process(fp_model *m, const char *target_name, const float *poses, const float *trans,
                           const float *rot, int N, float *poses_out);
/* getMaxScoreIndex (src/foundationpose_decoder.cu:24-35): first maximum wins. scores host [N].  A NaN among the scores is an error
 * (the reference always returns an index in [0, N); thrust::max_element's answer on NaNs is unspecified). */
int fp_argmax(fp_model *m, const float *scores, int N, int *index_out);

/* ---- hypothesis sharding over GPUs (new).  One process per GPU calls:
 *   fp_register_shard_begin : sampler (redundant on every rank) + refine + score trunk for hypotheses
 *                             [shard_begin, shard_begin+shard_count) of the fp_num_hypotheses() grid;
 *                             leaves pooled score features [shard_count,512] f32 and refined poses [shard_count,16]
 *                             in device buffers returned through feat_dev / poses_dev;
 *   (caller all-gathers both over RCCL);
 *   fp_register_shard_finish: cross-hypothesis attention + Linear + arg-max over all N gathered rows. */
int fp_register_shard_begin(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H,
                            int W, const char *target_name, int refine_itr, int shard_begin, int shard_count,
                            float **feat_dev, float **poses_dev);
int fp_register_shard_finish(fp_model *m, const float *all_feat_dev, const float *all_poses_dev, int N_total,
                             float out_pose[16], int *best_index, float *scores_host /* may be NULL */);
/* Read a device buffer the library handed out (feat_dev / poses_dev above) back to the host: a copy ordered on the model's own
 * stream + one synchronisation.  For callers without a HIP runtime of their own (the ctypes host side, tests); never uses the
 * legacy stream (a plain hipMemcpy fails with hipErrorStreamCaptureImplicit while any thread of the process captures a graph). */
int fp_download(fp_model *m, void *dst_host, const void *src_dev, size_t bytes);
/* The same exchange without host stalls (what foundationpose_cpp_amd/distributed.py and bench.py --gpus N use):
 *   fp_register_shard_begin_packed : as above, but only ENQUEUES on the model's stream (fp_stream) and leaves one row
 *                                    [feature 512 | pose 16] per hypothesis in the CALLER's device buffer packed_dev
 *                                    [rows_per_rank, 528] f32 (rows >= shard_count zeroed; shard_count may be 0).  No
 *                                    synchronisation, no allocation: order the collective after it with an event on fp_stream.
 *   (caller: ONE all_gather of packed_dev into gathered [world * rows_per_rank, 528]; with contiguous shards of
 *    rows_per_rank hypotheses the gathered rows are already in global hypothesis order)
 *   fp_register_shard_finish_packed: make fp_stream wait for the collective, then call; the cross-hypothesis head and the
 *                                    arg-max run over rows [0, n_total); one synchronisation at the end. */
int fp_register_shard_begin_packed(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H,
                                   int W, const char *target_name, int refine_itr, int shard_begin, int shard_count,
                                   float *packed_dev, int rows_per_rank);
int fp_register_shard_finish_packed(fp_model *m, const float *gathered_dev, int n_total, float out_pose[16], int *best_index);

/* The whole sharded Register as ONE call, natively ("one ncclAllGather (RCCL over xGMI)"): every rank (one
 * model per GPU; ranks may be processes or threads of one process) passes its RCCL communicator (ncclComm_t as void*; rank and
 * world size are read from it).  Rank r refines and scores hypotheses [r * ceil(N / world), ...) of the fp_num_hypotheses() grid,
 * the rows [feature 512 | pose 16] are exchanged by one ncclAllGather enqueued on the model's stream (no host synchronisation,
 * no staging copies, persistent buffers), and every rank evaluates the cross-hypothesis head and the arg-max redundantly: all
 * ranks return the same pose / index without a second collective.  A rank whose own half fails still joins the collective (with
 * NaN rows, which every other rank reports) so that nobody hangs.  RCCL is bound at first use (dlopen: a copy already in the
 * process, else librccl.so.1): the library has no link-time RCCL dependency.  world == 1 works without RCCL traffic.
 * A rank that cannot even allocate its exchange buffers cannot join: it calls ncclCommAbort (the other ranks' collective returns an
 * error instead of hanging; the communicator must be re-created) and reports that.  With more than one rank the call does not take
 * the FP_SERIALIZE_MODELS lock (one thread per rank would deadlock on it; ranks live on different devices). */
int fp_register_sharded(fp_model *m, void *nccl_comm, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                        const char *target_name, int refine_itr, float out_pose[16], int *best_index /* may be NULL */);

/* ---- frame / dataset I/O of the acceptance harness (simple_tests/include/tests/help_func.hpp) without OpenCV ----
 * dataset layout test_data/download.md:6-15: <dir>/cam_K.txt, rgb/<id>.png, depth/<id>.png (u16 mm), masks/<id>.png, mesh/ */
/* generic PNG decode (8/16-bit, grey/RGB/palette/alpha, non-interlaced): samples widened to u16, `channels` interleaved.
 * out may be NULL to query the size. */
int fp_image_read_png(const char *path, int *H, int *W, int *channels, int *bit_depth, uint16_t *out, size_t out_capacity);
int fp_frame_size(const char *rgb_path, int *H, int *W);
/* ReadRgbDepthMask / ReadRgbDepth (help_func.hpp:10-53): rgb u8 [H,W,3] RGB; depth f32 [H,W] = u16 / 1000; mask u8 [H,W]
 * (first channel).  Any of the three outputs (with its path) may be NULL. */
int fp_read_rgb_depth_mask(const char *rgb_path, const char *depth_path, const char *mask_path, int H, int W,
                           uint8_t *rgb, float *depth, uint8_t *mask);
/* ReadCamK (help_func.hpp:108-129): nine whitespace-separated numbers, row-major. */
int fp_read_cam_k(const char *cam_K_path, float K[9]);
/* cv::imwrite stand-in: 8-bit RGB PNG. */
int fp_image_write_png_rgb(const char *path, const uint8_t *rgb, int H, int W);
/* draw3DBoundingBox (help_func.hpp:55-106): green 12-edge box of `dimension` under the column-major bbox->camera `pose`
 * (= ConvertPoseMesh2BBox(pose_in_mesh, loader), mesh_loader.hpp:75-81), drawn into rgb in place. */
int fp_draw_bbox3d(uint8_t *rgb, int H, int W, const float K[9], const float pose[16], const float dimension[3]);

/* ---- a network on its own: the infer-core contract ----------------------------------------------------------------
 * The reference hands two deploy_core `BaseInferCore`s to the model and drives them through blobs
 * (GetBuffer / GetTensor(name) / SetBufferLocation / RawPtr / SetShape / SyncInfer: D6F/src/foundationpose.cpp:126-139,
 * 331-354,410-436; factory call shape simple_tests/src/test_foundationpose.cpp:24-35).  fp_net is that contract in C;
 * include/infer_core_amd.hpp puts the C++ names on top.  Blobs: "render_input", "transf_input" f32 [max_batch,160,160,6]
 * (foundationpose.cpp:78-83); refiner outputs "trans", "rot" [max_batch,3]; scorer output "scores" [max_batch]. */
typedef struct fp_net fp_net;
fp_net *fp_net_create(const char *packed_weights_path, int is_scorer, int max_batch);
void fp_net_destroy(fp_net *net);
int fp_net_max_batch(const fp_net *net);
/* pointer of a blob's FP_HOST (pinned) or FP_DEVICE copy; NULL + fp_last_error for an unknown name */
void *fp_net_blob(fp_net *net, const char *name, int memspace);
/* SyncInfer over the first `batch` entries; *_loc say which copy of each input holds the data and whether the outputs are
 * also wanted on the host */
int fp_net_infer(fp_net *net, int batch, int render_loc, int transf_loc, int out_loc);

/* ---- network precision ----------------------------------------------------------------------------------------------
 * The reference runs TensorRT engines built with --fp16 (tools/cvt_onnx2trt.bash:3-15): FP_PREC_F16 is the default and
 * the parity baseline.  FP_PREC_BF16: every tensor and MFMA operand in bf16 (BASELINE configs[1]).
 * FP_PREC_FP8 / FP_PREC_INT8 -- EXPERIMENTAL (round 6: BASELINE configs[4] runs in f16; no subset of trunk stages holds its parity bar,
 * >= 95 % of the refined poses within 1 mm / 1 deg of the 16-bit path on every unseen frame with < 0.3 mm of common mode, on 8-bit operands:
 * DESIGN.md section 4.4) -- the 8-bit MFMA conv path: the 13 3x3 trunk convolutions from encodeA.2 on
 * (91 % of the FLOPs) on 8-bit operands -- OCP e4m3 (v_mfma_f32_16x16x128_f8f6f4) or signed / unsigned 8-bit integers
 * (v_mfma_i32_16x16x64_i8, the same matrix-pipe rate class) -- with per-output-channel weight scales, per-input-channel
 * activation scales folded into the weights, an f16 residual stream (a skip connection is never re-quantised) and a data-driven
 * bias correction; everything else f16.  Each needs ITS OWN fp_calibrate / fp_set_calibration_blob first (the record holds the
 * statistics and the corrections solved against them; fp_set_calibration, the round-2 per-tensor form, serves both).  INT8 is the closer
 * of the two (85-90 % of the poses inside the bar on average, e4m3 under 1 %: uniform 8-bit steps over a ReLU output's range round 5-7x
 * finer than e4m3's 3 mantissa bits; DESIGN.md section 4.4 has the measurements).  Networks of a precision are built from the weight files given
 * to fp_create the first time the precision is selected. */
#define FP_PREC_F16 0
#define FP_PREC_BF16 1
#define FP_PREC_FP8 2
#define FP_PREC_INT8 3
int fp_set_precision(fp_model *m, int precision);
int fp_get_precision(const fp_model *m);
/* Post-training static quantisation for `precision` (FP_PREC_FP8 / FP_PREC_INT8) over the frames of a calibration session:
 *   fp_calibrate_begin(m, precision); fp_calibrate_add_frame(m, frame ...) x K; fp_calibrate_finish(m);
 * finish runs one f16 Register per frame to collect per-channel |max| and mean of the 15 trunk activations of both networks OVER ALL
 * FRAMES, quantises the 8-bit networks from them, then solves the bias / token / output correction layer by layer (~30 Registers per
 * frame).  Use K >= 8 frames of the deployment's scene family (object distances, orientations, sensor noise): the common-mode part of
 * the correction solved on ONE frame is partly that frame's own.  Frames are copied (host) when added; any
 * target / size the model accepts.  The precision's record is replaced only if every step succeeds -- on failure the previous record
 * (or "uncalibrated") stays; the pose is discarded; the model's precision is unchanged.  fp_calibrate_abort drops an open session;
 * fp_calibrate_frames = number of frames added so far (-1: no session).  Only the loading of networks not yet in memory is
 * exclusive against other calls of the process; the Registers of the calibration run like any Register.
 * fp_calibrate(..., precision) = begin + one add_frame + finish; fp_calibrate_fp8 = fp_calibrate(..., FP_PREC_FP8) (the round-2 name). */
int fp_calibrate_begin(fp_model *m, int precision);
int fp_calibrate_add_frame(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                           const char *target_name);
int fp_calibrate_finish(fp_model *m);
int fp_calibrate_abort(fp_model *m);
int fp_calibrate_frames(const fp_model *m);
int fp_calibrate(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                 const char *target_name, int precision);
int fp_calibrate_fp8(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                     const char *target_name);
/* The calibration record of a precision (scales + corrections + the calibration frames' channel means the INT8 weights were rounded
 * against; fp_calibration_size() bytes, versioned: records written by the previous version are still accepted) so that a deployment
 * calibrates once and reuses it; fp_set_calibration_blob reads the precision from the record. */
size_t fp_calibration_size(void);
int fp_get_calibration_blob(const fp_model *m, int precision, void *out, size_t capacity);
int fp_set_calibration_blob(fp_model *m, const void *blob, size_t bytes);
/* Per-tensor view of the same (the round-2 interface): |max| per trunk activation, [refiner 16 | scorer 16], 15 used each.
 * fp_set_calibration gives every channel of a tensor the tensor's scale and NO corrections -- the round-3 behaviour, kept for
 * records made then; prefer the blob. */
int fp_get_calibration(const fp_model *m, float amax_out[32]);
int fp_set_calibration(fp_model *m, const float amax[32]);

/* ---- float model of the rendering stage --------------------------------------------------------------------------
 * The reference's CUDA kernels are compiled by nvcc with its default -fmad=true (D6F/CMakeLists.txt:5 sets only -O3), so
 * the vertex transforms (foundationpose_render.cu:321-443), the nvdiffrast shader / interpolator / texture unit and
 * CudaRaster's clipper run with multiply-adds contracted.  1 (default): the same contraction, spelled with explicit fmaf
 * under one documented rule; 0: every operation separately rounded.  The CPU oracle implements both. */
#define FP_FLOAT_SEPARATE 0
#define FP_FLOAT_FMAD 1
int fp_set_float_model(fp_model *m, int float_model);
int fp_get_float_model(const fp_model *m);

/* ---- measurement hooks ---- */
/* When enabled, every kernel launch is bracketed with HIP events on the model's stream and accumulated per kernel
 * family; fp_profile_report writes "name calls total_ms flops bytes" lines. */
int fp_profile_enable(fp_model *m, int on);
int fp_profile_reset(fp_model *m);
int fp_profile_report(fp_model *m, char *buf, int buf_len);
/* stream used for all launches (hipStream_t as void*), so callers can order their own work / events. */
void *fp_stream(fp_model *m);
int fp_synchronize(fp_model *m);

#ifdef __cplusplus
}
#endif
#endif
