// Internal declarations shared by the HIP translation units of libfoundationpose_amd.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#define FP_CROP_HW 160
#define FP_NN_IN_BORDER 2  // zero border (in space-to-depth pixels) around each network-input image
// halfs per network-input image: [84,84,32]
#define FP_NN_IN_IMG_HALFS ((size_t)(FP_CROP_HW / 2 + 2 * FP_NN_IN_BORDER) * (FP_CROP_HW / 2 + 2 * FP_NN_IN_BORDER) * 32)
#define FP_MIN_DEPTH 0.001f  // FoundationPoseRenderer min_depth (foundationpose_render.hpp:26)
#define FP_MAX_DEPTH 4.0f    // FoundationPoseRenderer max_depth (foundationpose_render.hpp:27)

namespace fp {

// ---------------------------------------------------------------------------------------------
// error plumbing: C ABI returns 0 / non-zero + fp_last_error()
// ---------------------------------------------------------------------------------------------
void set_error(const std::string &msg);
// fp_image_io.cpp: 8-bit PNG (grey / RGB / palette / alpha variants) -> RGB u8
bool load_png_rgb(const std::string &path, std::vector<uint8_t> &rgb, int &H, int &W);
// any texture container the library decodes (PNG incl. 16-bit / sub-byte / interlaced, baseline + progressive JPEG, BMP, PNM, TGA) -> RGB u8 like cv::imread + BGR2RGB
bool load_texture_rgb(const std::string &path, std::vector<uint8_t> &rgb, int &H, int &W, std::string *why);
// Synchronous copies / fills WITHOUT the legacy (null) stream: hipMemcpy / hipMemset fail with hipErrorStreamCaptureImplicit (906)
// while ANY thread of the process captures a hipGraph (another model replaying its warm-up), so the library never touches the
// legacy stream -- these go through a per-thread non-blocking utility stream and wait for it.
hipError_t memcpy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t memset_sync(void *dst, int value, size_t bytes);
// Per-DEVICE once for launch sites that opt a kernel into > 64 KB of dynamic LDS: hipFuncSetAttribute acts on the current device's
// copy of the function, so a process that drives several GPUs (one model per device) has to repeat it on each.  BLOCKING [r5]: a second
// thread on the same device (another model: the documented concurrency model) waits until the first has applied the attribute --
// a flag that is set before the attribute call would let it launch a > 64 KB kernel without the opt-in (std::call_once per device).
struct PerDeviceOnce {
  std::once_flag once[64];
  template <class F>
  void run(F &&f) {   // f runs exactly once per device, and every caller returns only after it has (devices >= 64: every time, harmless)
    int d = 0;
    (void)hipGetDevice(&d);
    if (d < 0 || d >= 64) { f(); return; }
    std::call_once(once[d], f);
  }
};
// bumped whenever a device buffer that kernels may have baked into a captured hipGraph is (re)allocated
extern std::atomic<unsigned long> g_alloc_epoch;
#define FP_HIP_OK(expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) {                                                                          \
      fp::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));                       \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)
#define FP_CHECK(cond, msg)                                                                          \
  do {                                                                                               \
    if (!(cond)) {                                                                                   \
      fp::set_error(msg);                                                                            \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

// ---------------------------------------------------------------------------------------------
// profiling: optional HIP-event bracket around every launch, accumulated per kernel family
// ---------------------------------------------------------------------------------------------
struct ProfEntry {
  std::string name;
  long calls = 0;
  double flops = 0, bytes = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double ms = 0;
};
struct Profiler {
  bool on = false;
  std::vector<ProfEntry> entries;
  std::vector<hipEvent_t> pool;
  ProfEntry &get(const char *name);
  hipEvent_t ev();
  void begin(hipStream_t s, const char *name, double flops, double bytes);
  void end(hipStream_t s);
  void collect();
  void reset();
  ProfEntry *cur = nullptr;
  hipEvent_t cur_start = nullptr;
};
// roctx ranges (SURVEY.md section 5 "tracing / profiling": roctx + rocprofv3): every ProfScope -- one per kernel launch site, named
// "<layer>/<kernel>" -- and the stage scopes of fp_api.hip (RoctxRange) push / pop a range, so `rocprofv3 --marker-trace` sees
// labelled stages instead of a stream of 60 anonymous kernels.  The roctx library is bound at first use with dlopen
// (librocprofiler-sdk-roctx, else libroctx64); without it the calls are no-ops.  Host-side markers: inside a replayed hipGraph
// there is no host code per launch, so profile with graphs off (the first, eager call of a configuration) to see per-launch ranges.
void roctx_push(const char *name);
void roctx_pop();
struct RoctxRange {
  explicit RoctxRange(const char *name) { roctx_push(name); }
  ~RoctxRange() { roctx_pop(); }
  RoctxRange(const RoctxRange &) = delete;
  RoctxRange &operator=(const RoctxRange &) = delete;
};
struct ProfScope {
  Profiler *p;
  hipStream_t s;
  ProfScope(Profiler *p_, hipStream_t s_, const char *name, double flops = 0, double bytes = 0) : p(p_), s(s_) {
    roctx_push(name);
    if (p && p->on) p->begin(s, name, flops, bytes);
  }
  ~ProfScope() {
    if (p && p->on) p->end(s);
    roctx_pop();
  }
};

// ---------------------------------------------------------------------------------------------
// geometry kernels (fp_geometry.hip)
// ---------------------------------------------------------------------------------------------

// test build: the launch log of fp_nn.hip (fpt_launch_log_*) armed with 2 also records every launch outside the networks -- frame
// upload, record publication, depth filters, sampler, render, crop, pose fit -- with net = -1, for tests that count a call's launches
#ifdef FP_TEST_HOOKS
void log_geometry_launch(const char *name);
#define FP_GEOM_LOG(name) fp::log_geometry_launch(name)
#else
#define FP_GEOM_LOG(name) ((void)0)
#endif

// Per-hypothesis record produced by the pose-setup kernel; everything the reference computes on the host per
// pose (ComputeCropWindowTF, ConstructBBox2D, ProjectMatrixFromIntrinsics, foundationpose_render.cpp:25-186,590).
struct PoseRec {
  float M[16];     // Proj * GLcam * pose, column-major
  float pose[16];  // column-major
  float a00, a11, a30, a31;  // generate_pose_clip remap (foundationpose_render.cu:382-384)
  float m0, m2, m4, m5;      // inverse crop transform: src = (m0*x + m2, m4*y + m5)
  float tf[9];               // forward crop transform, row-major (debug / tests)
  float bbox[4];
};

struct DeviceMesh {
  int V = 0, F = 0, TH = 0, TW = 0;
  float diameter = 0;
  float center[3] = {0, 0, 0};
  float max_norm = 0;        // largest vertex norm of the centred mesh (the screen bound of fp_render_pose)
  float *verts = nullptr;    // [V,3] centred
  float *normals = nullptr;  // [V,3]
  float *uvs = nullptr;      // [V,2] (u, 1-v)
  int32_t *faces = nullptr;  // [F,3]
  uint8_t *tex = nullptr;    // [TH,TW,3]
  uint32_t *vcol = nullptr;  // [V] r | g << 8 | b << 16 (fp_set_vertex_colors); null: the colour source is the texture
};

enum OutMode { OUT_F32X6 = 0, OUT_F16X8 = 1, OUT_BF16X8 = 2 };  // F32X6: the reference's blob; *X8: the networks' s2d input tensor

void launch_pose_setup(hipStream_t s, const float *poses_dev, int N, const float *K9_host, int img_h, int img_w,
                       float crop_ratio, float diameter, PoseRec *recs);
#ifdef FP_TEST_HOOKS
extern float4 *g_vertex_dbg;  // race hunt: per-vertex intermediates (null = off)
#endif
// fmad: float model of the vertex stage / shader / interpolator / texture unit (fp_geometry.hip "float model")
void launch_vertex(hipStream_t s, const DeviceMesh &m, const PoseRec *recs, int N, float4 *clip, float4 *attr, bool fmad);
// the two above in ONE launch (recs is an output)
void launch_setup_vertex(hipStream_t s, const DeviceMesh &m, const float *poses_dev, int N, const float *K9_host, int img_h, int img_w,
                         float crop_ratio, float diameter, PoseRec *recs, float4 *clip, float4 *attr, bool fmad);
#ifdef __HIPCC__
// RefinePostProcess for hypothesis i (foundationpose.cpp:360-406): one function for pose_update_kernel and for the Track head
// kernel of fp_nn.hip that applies it in place (one launch less per frame); identical arithmetic in both.
__device__ __forceinline__ void pose_update_one(float *poses, const float *__restrict__ trans, const float *__restrict__ rot, int i, float diameter,
                                                const float *poses_in, float *extra_out) {
  // fp_geometry.hip is compiled with -ffp-contract=off (the oracle's float model), fp_nn.hip is not: pin it
  // here so that both translation units evaluate exactly the same operations
#pragma clang fp contract(off)
  const float NORM = 0.349065850398865f;
  float P[16];
  for (int k = 0; k < 16; k++) P[k] = poses_in[(size_t)i * 16 + k];
  float td[3], v[3];
  for (int k = 0; k < 3; k++) { td[k] = trans[i * 3 + k] * (diameter / 2); v[k] = tanhf(rot[i * 3 + k]) * NORM; }
  float n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  float ang = sqrtf(n2);
  float ax[3] = {v[0], v[1], v[2]};
  if (n2 > 0.0f) { ax[0] /= ang; ax[1] /= ang; ax[2] /= ang; }
  float s = sinf(ang), c = cosf(ang);
  float sa[3] = {s * ax[0], s * ax[1], s * ax[2]}, ca[3] = {(1.0f - c) * ax[0], (1.0f - c) * ax[1], (1.0f - c) * ax[2]};
  float R[9], tmp;
  tmp = ca[0] * ax[1]; R[1] = tmp - sa[2]; R[3] = tmp + sa[2];
  tmp = ca[0] * ax[2]; R[2] = tmp + sa[1]; R[6] = tmp - sa[1];
  tmp = ca[1] * ax[2]; R[5] = tmp - sa[0]; R[7] = tmp + sa[0];
  R[0] = ca[0] * ax[0] + c; R[4] = ca[1] * ax[1] + c; R[8] = ca[2] * ax[2] + c;
  float O[16];
  for (int k = 0; k < 16; k++) O[k] = P[k];
  O[12] = P[12] + td[0]; O[13] = P[13] + td[1]; O[14] = P[14] + td[2];
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      float sacc = R[0 * 3 + r] * P[cc * 4 + 0];
      sacc = sacc + R[1 * 3 + r] * P[cc * 4 + 1];
      sacc = sacc + R[2 * 3 + r] * P[cc * 4 + 2];
      O[cc * 4 + r] = sacc;
    }
  for (int k = 0; k < 16; k++) poses[(size_t)i * 16 + k] = O[k];
  if (extra_out)
    for (int k = 0; k < 16; k++) extra_out[(size_t)i * 16 + k] = O[k];
}
#endif
struct FrameRef;
// tiny batches: the same + the observed-crop warp of hypotheses [0, n_crop) in ONE launch, 2-byte output modes only (plan_render asks
// for it in no other); tri_rows non-null: the launch also leaves the [N, F] row ranges launch_tri_rows would compute from its clip coordinates
void launch_setup_vertex_crop(hipStream_t s, const DeviceMesh &m, const float *poses_dev, int N, const float *K9_host, int img_h, int img_w,
                              float crop_ratio, float diameter, PoseRec *recs, float4 *clip, float4 *attr, bool fmad, const FrameRef *frame,
                              int n_crop, OutMode mode, void *out_b, unsigned *tri_rows);
// [N, F] row ranges of the triangles of these clip coordinates (a strip of the rasteriser then skips the triangles that miss it)
void launch_tri_rows(hipStream_t s, const DeviceMesh &m, int N, const float4 *clip, unsigned *rows);

// The render + crop schedule: which kernels one render_and_crop call (fp_api.hip) launches and in which shape is
// plan_render's decision alone -- a pure host function (no HIP call; the test build's fpt_plan_render asks it without a GPU,
// tests/test_render_plan_cpu.py), like plan_conv of fp_nn.hip.  The thresholds, each the LARGEST batch of its row of the table:
constexpr int RENDER_FUSED_FRONT_MAX_N = 4;   // set-up + vertex stage + crop warp (+ row ranges) as one launch (Track)
constexpr int RENDER_ROWS4_MAX_N = 2;         // 4-row strips of 1024 threads
constexpr int RENDER_NT1024_MAX_N = 25;       // 8-row strips of 1024 threads
constexpr int RENDER_ROWS8_MAX_N = 47;        // 8-row strips (of 512 threads); above: 20-row strips of 256 threads
constexpr int RENDER_TRI_ROWS_MAX_N = 99;     // row ranges; above: two 80-row strips of 1024 threads that walk every triangle
struct RenderQuery {
  int N = 0;
  OutMode mode = OUT_F16X8;
  bool out_a = false, out_b = false;   // a rendered / an observed output is wanted
  bool taps = false;                   // debug taps (triangle ids, rasteriser output) are attached
  bool prof = false;                   // the profiler is on: every stage is its own, bracketed launch
  int F = 0;                           // triangles of the target
  size_t tri_cap = 0;                  // entries of the model's row-range buffer, 0: none
};
enum RenderFront { FRONT_SETUP = 0, FRONT_SETUP_VERTEX = 1, FRONT_SETUP_VERTEX_CROP = 2 };   // pose set-up alone (crop without render) | + vertex stage | + crop warp
enum RowRanges { ROW_RANGES_NONE = 0, ROW_RANGES_BY_FRONT = 1, ROW_RANGES_OWN_LAUNCH = 2 };    // BY_FRONT: written by the fused front launch
struct RenderPlan {
  RenderFront front;
  RowRanges row_ranges;
  int strip_rows, threads;   // the rasteriser's instantiation (meaningless after FRONT_SETUP: nothing is rendered)
  int lds;                   // its dynamic LDS: the strip's z-buffer (+ the triangle list with row ranges)
  bool lds_optin;            // the instantiation needs the > 64 KB opt-in
  bool crop_launch;          // crop_kernel as its own launch
};
RenderPlan plan_render(const RenderQuery &q);
// the rasteriser instantiation the plan names; tri_rows non-null exactly when plan.row_ranges says so.  false: no such instantiation
bool launch_raster_shade(hipStream_t s, const RenderPlan &plan, const DeviceMesh &m, const PoseRec *recs, int N, const float4 *clip,
                         const float4 *attr, OutMode mode, void *out, int32_t *tri_id_dbg, float *rast_dbg, bool fmad,
                         const unsigned *tri_rows);
// the frame a replayed hipGraph reads: kernels inside graphs take the frame through this device-resident record, so a caller's
// device frame is used in place (no copy into model-owned buffers) and the graph stays valid when the pointers change
// how the kernels of a (replayed) graph find the current frame.  Whole frames: pitch = 0 (rows are W pixels apart), window = all.
// [r4] Track's packed crop window of a host frame: rgb / depth are VIRTUAL origins (the address pixel (0, 0) would have if the packed
// window were part of a frame with rows `pitch` pixels apart), and only pixels inside [wx0, wx1) x [wy0, wy1) exist.
struct FrameRef {
  const uint8_t *rgb;
  const float *depth;
  int pitch = 0;
  int wx0 = 0, wy0 = 0, wx1 = 0x7fffffff, wy1 = 0x7fffffff;
  // depth filter (fp_set_depth_filter; unused while the option is off): `depth` is then a model-owned buffer
  // that depth_filter_rect_kernel fills inside [wx0, wx1) x [wy0, wy1) from the unfiltered depth `raw`, which is addressed like
  // `depth` (same pitch, same virtual origin) and exists inside [ux0, ux1) x [uy0, uy1)
  const float *raw = nullptr;
  int ux0 = 0, uy0 = 0, ux1 = 0, uy1 = 0;
};
static_assert(sizeof(FrameRef) <= 64, "a frame record is one 64-byte slot of the record ring and the head of the window block");
inline bool same_record(const FrameRef &a, const FrameRef &b) {
  return a.rgb == b.rgb && a.depth == b.depth && a.pitch == b.pitch && a.wx0 == b.wx0 && a.wy0 == b.wy0 && a.wx1 == b.wx1 && a.wy1 == b.wy1 &&
         a.raw == b.raw && a.ux0 == b.ux0 && a.uy0 == b.uy0 && a.ux1 == b.ux1 && a.uy1 == b.uy1;
}
// The window of the frame a Track with one refine iteration reads (DESIGN.md sections 4.2, 4.7): ComputeCropWindowTF
// (foundationpose_render.cpp:25-70) restated on the host in double with a margin, grown by `reach` pixels on every side (the depth
// filter reads 4 pixels around every pixel the crop may read) and clamped to the frame.  A pure host function like plan_render
// (the test build's fpt_plan_track_window asks it without a GPU); WHICH outcome it is never depends on reach.
enum TrackWindowKind { TRACK_WINDOW_WHOLE = 0, TRACK_WINDOW_OUTSIDE = 1, TRACK_WINDOW_ROWS = 2, TRACK_WINDOW_RECT = 3 };
struct TrackWindow {
  TrackWindowKind kind;        // WHOLE: no estimate, the whole frame | OUTSIDE: the crop window misses the frame, nothing is read
  int row0, row1, col0, col1;  // ROWS: rows [row0, row1) of every column | RECT: those rows of columns [col0, col1)
};
TrackWindow plan_track_window(const float K[9], float diameter, const float pose[16], int H, int W, int reach);
// depth filter of a rectangle in ONE launch: D' = bilateral(erode(raw)) inside the record's window (clamped to the frame), written to
// the record's `depth` -- the same values, bit for bit, as launch_erode + launch_bilateral give there.  Every argument that changes
// with the pose comes from the record in device memory: the launch may be captured and replayed for any window of an H x W frame.
constexpr int DEPTH_FILTER_TILE_W = 32, DEPTH_FILTER_TILE_H = 16;
void launch_depth_filter_rect(hipStream_t s, const FrameRef *frame_dev, int H, int W);
void launch_crop(hipStream_t s, const FrameRef *frame_dev, int H, int W, const float *K9_host,
                 const PoseRec *recs, int N, float diameter, OutMode mode, void *out);
void launch_depth_to_xyz(hipStream_t s, const float *depth, int H, int W, const float *K9_host, float *xyz);
// copies `bytes` (rounded up to 16) from a host-pinned, device-mapped block into device memory with a kernel
void launch_window_fetch(hipStream_t s, const void *src_host_mapped, void *dst, size_t bytes);
void launch_erode(hipStream_t s, const float *depth, float *out, int H, int W);
void launch_bilateral(hipStream_t s, const float *depth, float *out, int H, int W);
// device-side refine post process: poses updated in place from trans/rot [N,3] (foundationpose.cpp:360-406)
// poses_in (optional): read the poses from there instead of `poses`; extra_out (optional): a second copy of the result (Track: both
// are host-pinned, so no copy kernels run around the graph)
void launch_pose_update(hipStream_t s, float *poses, const float *trans, const float *rot, int N, float diameter,
                        const float *poses_in = nullptr, float *extra_out = nullptr);
// first-max arg-max over scores[N] -> *index (foundationpose_decoder.cu:24-35)
void launch_argmax(hipStream_t s, const float *scores, int N, int *index_dev, const float *poses = nullptr,
                   float *best_pose_dev = nullptr);
// GuessTranslation + hypothesis poses on the device; state = int[8] (status in state[6]: 0 ok, 1 empty mask, 2 no valid depth)
void launch_sampler(hipStream_t s, const float *filtered_depth, const uint8_t *mask_dev, int H, int W, float min_depth,
                    const float *K9_host, const float *grid_dev, int first, int N, int *state, float *vals, float *poses);
// f32 [N,160,160,6] -> the networks' 2-byte s2d input tensor (blob-mode entry points); mode = OUT_F16X8 / OUT_BF16X8
void launch_pack_f32x6(hipStream_t s, const float *in, void *out, size_t pixels, OutMode mode);

// pose fit: per hypothesis n, image A = img_a + n * a_stride (rendered) against image B = img_b + n * b_stride
// (observed), both single images of the networks' input tensor in `mode`'s element type; strides in elements.  tol: the f32
// threshold per hypothesis (uniform: v[0] for all; otherwise N <= 64).  acc: [N, 4] 64-bit accumulators that are ZERO on entry and
// zero again when the kernel has finished (the host zeroes them once, at allocation); out: [N] records, device or host-mapped.
struct PoseFitTol {
  float v[64];
  int uniform;
};
struct PoseFitRec {   // the integer part of fp_pose_fit (include/foundationpose_amd.h)
  int32_t n_model, n_observed, n_inlier, n_front, n_behind, reserved;
  long long sum_dz_q20;
};
int pose_fit_split(int N);   // workgroups per hypothesis
void launch_pose_fit(hipStream_t s, const void *img_a, size_t a_stride, const void *img_b, size_t b_stride, int N, const PoseFitTol &tol,
                     OutMode mode, unsigned long long *acc, PoseFitRec *out);

// how many of the wave's 64 lanes hold b: wave-uniform, so one lane can add it to an integer counter (the tile kernels and the search)
__device__ __forceinline__ unsigned wave_count(bool b) { return (unsigned)__popcll(__ballot(b)); }

// frame-resolution rendering of one pose (fp_render_pose; fp_frame_render.hip)
constexpr float FRAME_RENDER_NEAR = 0.01f;          // = FP_RENDER_NEAR_M: a vertex with z below it refuses the pose (there is no clipper)
constexpr int FRAME_RENDER_SNAP_MAX = 1 << 26;      // = FP_RENDER_SNAP_MAX: largest |snapped coordinate| (1/16 px); edge functions stay below 2^56
constexpr int FRAME_RENDER_FLAG_NEAR = 1, FRAME_RENDER_FLAG_RANGE = 2;
constexpr int FRAME_RENDER_TILE = 32, FRAME_RENDER_THREADS = 256;   // a 32 x 32 px tile per workgroup: 8 KB of 64-bit keys in LDS
constexpr int FRAME_RENDER_TINT_R = 40, FRAME_RENDER_TINT_G = 220, FRAME_RENDER_TINT_B = 120;
struct FramePose {
  float r[9];   // linear part, ROW-major
  float t[3];
  float fx, fy, cx, cy;
};
struct FrameRenderOut {   // device pointers, null = not wanted
  float *depth;
  uint8_t *mask, *vis;
  int32_t *tri;
  uint8_t *overlay;
};
struct FrameTileBound {
  int tx0, ty0, tx1, ty1;   // tiles [tx0, tx1] x [ty0, ty1] walk the triangles, the others write background
};
// pure host function: the conservative screen bound of the object, in tiles
FrameTileBound frame_tile_bound(const FramePose &pose, double radius, int H, int W);
// snap [V] = {xi, yi, bits(z), 0}, cam [V] = {x, y, z, 0}; *flag must be zero on entry
void launch_frame_vertex(hipStream_t s, const DeviceMesh &m, const FramePose &pose, int4 *snap, float4 *cam, int *flag);
// the same for a batch of poses out of device memory (fp_pose_vsd, fp_refine_depth): pose p of the launch is poses_a[p] (p < n_a) or
// poses_b[p - n_a] (n_b may be 0); snap [(n_a + n_b) V] and cam likewise (null: not stored) in the formats above; pose p raises
// flags_a[p] or flags_b[p - n_a], which must be zero on entry.  log_name: the launch's name in the test build's launch log.
void launch_pose_vertices(hipStream_t s, const char *log_name, const DeviceMesh &m, const FramePose *poses_a, int n_a, const FramePose *poses_b, int n_b,
                          int4 *snap, float4 *cam, int *flags_a, int *flags_b);
void launch_frame_raster(hipStream_t s, const DeviceMesh &m, const int4 *snap, const float4 *cam, const uint8_t *rgb, const float *depth,
                         int H, int W, const FrameTileBound &bound, float tol_m, const FrameRenderOut &out);

// frame-resolution rendering of all tracked objects of a frame in one pass (fp_render_scene; fp_scene_render.hip).
// Per object the rules and constants are those of section 4.8 above; the objects meet in one z-buffer of keys bits(z) << 32 | g with
// g the GLOBAL triangle index (face_start[o] + t).
constexpr int SCENE_MAX_OBJECTS = 64;               // = FP_SCENE_MAX_OBJECTS
constexpr int SCENE_PALETTE[8][3] = {               // tint of object o is SCENE_PALETTE[o % 8]; entry 0 is fp_render_pose's
    {FRAME_RENDER_TINT_R, FRAME_RENDER_TINT_G, FRAME_RENDER_TINT_B}, {230, 80, 60}, {70, 130, 240}, {240, 200, 40},
    {200, 80, 220}, {40, 210, 220}, {250, 140, 30}, {160, 230, 60}};
constexpr long long SCENE_MAX_ENTRIES = 0x7fffffffll;   // (tile, triangle) entries of one call: the lists are indexed with 32 bits
struct SceneTable {   // device-resident description of the call's objects, in call order
  FramePose pose[SCENE_MAX_OBJECTS];
  const float *verts[SCENE_MAX_OBJECTS];
  const int32_t *faces[SCENE_MAX_OBJECTS];
  int vert_start[SCENE_MAX_OBJECTS + 1];        // object o owns scene vertices [vert_start[o], vert_start[o + 1])
  unsigned face_start[SCENE_MAX_OBJECTS + 1];   // ... and global triangles [face_start[o], face_start[o + 1])
  int K;
};
struct SceneRenderOut {   // device pointers, null = not wanted
  float *depth;
  uint8_t *inst, *vis;
  int32_t *tri;
  unsigned long long *cover;
  uint8_t *overlay;
  int *counters;   // [K, 3] {covered, front, visible}, zero on entry
};
// pure host functions: the tile grid of a frame, and the int32 words of the binning block [flags 64 | total 2 | counters 192 |
// count ntiles | offset ntiles + 1 | cursor ntiles]
constexpr int SCENE_WORK_FLAGS = 0, SCENE_WORK_TOTAL = 64, SCENE_WORK_COUNTERS = 66, SCENE_WORK_COUNT = 258;
inline int scene_tiles_x(int W) { return (W + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE; }
inline int scene_tiles_y(int H) { return (H + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE; }
inline size_t scene_work_words(int H, int W) { return (size_t)SCENE_WORK_COUNT + (size_t)3 * scene_tiles_x(W) * scene_tiles_y(H) + 1; }
// snap / cam [vert_start[K]] in frame_vertex_kernel's format; flags [K] must be zero on entry
void launch_scene_vertex(hipStream_t s, const SceneTable *table, int total_verts, int4 *snap, float4 *cam, int *flags);
// count [ntiles] must be zero on entry; leaves offset [ntiles + 1] (exclusive scan), cursor = offset and *total (64-bit) = all entries
void launch_scene_bin_count(hipStream_t s, const SceneTable *table, unsigned total_faces, const int4 *snap, int H, int W, unsigned *count,
                            unsigned *offset, unsigned *cursor, unsigned long long *total);
// list [total]: the global triangle indices of every tile, tile after tile (order inside a tile: whatever the atomics gave)
void launch_scene_bin_fill(hipStream_t s, const SceneTable *table, unsigned total_faces, const int4 *snap, int H, int W, unsigned *cursor,
                           unsigned *list);
void launch_scene_raster(hipStream_t s, const SceneTable *table, const int4 *snap, const float4 *cam, const unsigned *offset,
                         const unsigned *list, const uint8_t *rgb, const float *depth, int H, int W, float tol_m, const SceneRenderOut &out);

// pose errors (fp_pose_errors; fp_pose_error.hip).  Matrices are 12 floats: the linear part ROW-major, then t.
constexpr int POSE_ERROR_THREADS = 256;
constexpr int POSE_ERROR_QUERIES = 4;      // query points a lane of the nearest-neighbour kernel keeps in registers
constexpr int POSE_ERROR_TILE = 1024;      // target points staged in LDS at a time (structure of arrays, 12 KB)
struct PoseErrPair {                       // what the paired kernel leaves per (pose, symmetry)
  unsigned max_d_bits, max_px_bits;        // bit patterns of max_v |a - b| and of the largest projected distance (both >= 0)
  int near, pad;                           // non-zero: a used vertex has !(z >= FRAME_RENDER_NEAR) under either transform
  long long sum_q20;                       // sum_v llrintf(|a - b| * 2^20)
};
// pair p = pose * S1 + s of [pair0, pair0 + n_pairs): a = est[pose] v, b = comp[p] v over the vertices 0, step, ... (Vs of them); one
// workgroup per pair, every entry of out [pair0, pair0 + n_pairs) is written
void launch_pose_error_pairs(hipStream_t s, const float *verts, int Vs, int step, float fx, float fy, float cx, float cy, const float *est,
                             const float *comp, int S1, long long pair0, int n_pairs, PoseErrPair *out);
// poses [pose0, pose0 + n_poses): sums[pose] += sum_u llrintf(min_v |rel[pose] u - v| * 2^20) over the same Vs vertices on both sides
void launch_pose_error_nn(hipStream_t s, const float *verts, int Vs, int step, const float *rel, int pose0, int n_poses,
                          unsigned long long *sums);

// visible surface discrepancy (fp_pose_vsd; fp_pose_vsd.hip).  The renderings follow section 4.8's rules through
// fp_frame_rules.h; a pose's counters are VSD_WORDS 32-bit words: n_model_est, n_model_gt, n_visib_est, n_visib_gt, n_inter, n_union,
// n_fail[16], two unused.
constexpr int VSD_MAX_TAUS = 16;                    // = FP_VSD_MAX_TAUS
constexpr int VSD_WORDS = 24;
constexpr size_t VSD_SCRATCH_BYTES = 128u << 20;    // snapped vertices of one chunk of poses (estimates + their ground truths) stay below this
struct VsdParams {
  float fx, fy, cx, cy;
  float delta;               // the visibility tolerance delta_m
  int T;                     // thresholds in use
  float thr[VSD_MAX_TAUS];   // in metres (already multiplied by the diameter when normalised)
};
// items [n_items] = {pose of the chunk, tile}: counters[(pose0 + pose) VSD_WORDS ..] += the tile's pixel counts.  snap_g non-null: ground
// truth `pose` of the chunk is walked like the estimate; null: plane_g [H,W] holds the one ground truth's model depth (0 = background)
void launch_vsd_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap_e, const int4 *snap_g, const float *plane_g, const int2 *items, int n_items,
                      const float *depth, int H, int W, const VsdParams &P, int pose0, int *counters);

// projective ICP on the observed depth (fp_refine_depth; fp_pose_icp.hip).  The renderings follow section 4.8's
// rules through fp_frame_rules.h; a pose's accumulator is ICP_WORDS 64-bit words: the 21 upper-triangle entries of sum J J^T (row-major),
// the 6 of sum J e, sum e^2 -- each term llrintf(product * 2^32) -- then n_model, n_valid, n_used, n_front, n_behind, n_grazing.
constexpr int ICP_SUMS = 28, ICP_COUNTS = 6, ICP_WORDS = ICP_SUMS + ICP_COUNTS;
constexpr float ICP_MIN_COS = 0.2f;                 // = FP_ICP_MIN_COS
constexpr size_t ICP_SCRATCH_BYTES = 128u << 20;    // snapped + camera-space vertices of one chunk of poses stay below this
struct IcpParams {
  float fx, fy, cx, cy;
  float max_dist;   // the gate max_dist_m
  float rad;        // diameter * 0.5f
  float t[3];       // the pose's translation
  float pad;
};
// items [n_items] = {pose of the chunk, tile}: acc[(pose0 + pose) ICP_WORDS ..] += the tile's sums and counts, under params[pose0 + pose];
// an item whose flags[pose0 + pose] is not zero does nothing
void launch_icp_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const float4 *cam, const int2 *items, int n_items, const float *depth,
                      int H, int W, const IcpParams *params, const int *flags, int pose0, unsigned long long *acc);

// colour agreement (fp_pose_color; fp_pose_color.hip).  The renderings follow section 4.8's rules through
// fp_frame_rules.h; a pose's accumulator is COLOR_WORDS 64-bit words: per channel R, G, B the sums of m, o, m m, o o, m o (m the model's
// value, o the frame's byte; 15 words in that order), then n_model, n_visible, n_compared, n_nocolor.
constexpr int COLOR_SUMS = 15, COLOR_COUNTS = 4, COLOR_WORDS = COLOR_SUMS + COLOR_COUNTS;
constexpr size_t COLOR_SCRATCH_BYTES = 128u << 20;  // snapped vertices of one chunk of poses stay below this
// items [n_items] = {pose of the chunk, tile}: acc[(pose0 + pose) COLOR_WORDS ..] += the tile's sums and counts; an item whose
// flags[pose0 + pose] is not zero does nothing.  The colour source is the mesh's current one (vcol, else the texture).
void launch_color_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const uint8_t *rgb, const float *depth,
                        int H, int W, float tol_m, const int *flags, int pose0, unsigned long long *acc);

// silhouette agreement (fp_pose_silhouette / fp_mask_distance; fp_pose_silhouette.hip).  The exact squared
// Euclidean distance transform of a u8 mask [H, W] (a mask pixel: byte > 0), H and W at most FP_SIL_MAX_DIM, in two launches:
//   columns  g [2, H, W] = per set (0: the mask pixels, 1: the others) the distance along the column to its nearest seed, 0xFFFF: the column
//            has none; any [2] (zero on entry) |= 1 where a set has a seed at all
//   rows     d2 [2, H, W] = the squared distance to the nearest seed of each set, FP_SIL_D2_NONE where the set is empty; tot [2] (zero on
//            entry) += {the mask pixels, the sum over them of d2[1], clipped to t2 where t2 > 0}
void launch_mask_edt_cols(hipStream_t s, const uint8_t *mask, int H, int W, uint16_t *g, int *any);
void launch_mask_edt_rows(hipStream_t s, const uint16_t *g, const int *any, int H, int W, uint32_t *d2, long long t2, unsigned long long *tot);
// a pose's accumulator is SIL_WORDS 64-bit words: n_model, n_visible, n_inter, n_spill, the sum of clip(d2[0]) over the spill pixels, the
// sum of clip(d2[1]) over the inter pixels.  items [n_items] = {pose of the chunk, tile}: acc[(pose0 + pose) SIL_WORDS ..] += the tile's
// counts and sums; an item whose flags[pose0 + pose] is not zero does nothing.  amodal: every model pixel is visible, depth is not read.
constexpr int SIL_WORDS = 6;
constexpr size_t SIL_SCRATCH_BYTES = 128u << 20;  // snapped vertices of one chunk of poses stay below this
void launch_silhouette_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const float *depth,
                             const uint8_t *mask, const uint32_t *d2, int H, int W, float tol_m, long long t2, bool amodal, const int *flags, int pose0,
                             unsigned long long *acc);

// silhouette refinement (fp_refine_silhouette; fp_refine_silhouette.hip).  sd [H, W] is the signed squared distance
// of the call's mask: -d2[1] on a mask pixel, d2[0] elsewhere (never 0).  A pose's accumulator is SILREF_WORDS 64-bit words: the 21
// upper-triangle entries of sum J J^T (row-major), the 6 of sum J e, sum e^2 -- each term llrintf(product * 2^24) -- then n_model,
// n_contour, n_used, n_occluded, n_far, n_flat, n_steep.
constexpr int SILREF_SUMS = 28, SILREF_COUNTS = 7, SILREF_WORDS = SILREF_SUMS + SILREF_COUNTS;
constexpr float SILREF_MAX_TERM = 64.0f;            // = FP_SILREF_MAX_TERM
struct SilrefParams {
  float fx, fy, cx, cy;
  float kx, ky;     // (fx * rad) / s, (fy * rad) / s
  float s, rad;     // the object's radius in pixels, (fx * rad) / t.z; diameter * 0.5f
  float t[3];       // the pose's translation
  float pad;
};
void launch_mask_signed_d2(hipStream_t s, const uint8_t *mask, const uint32_t *d2, int H, int W, int32_t *sd);
// items [n_items] = {pose of the chunk, tile}: acc[(pose0 + pose) SILREF_WORDS ..] += the tile's sums and counts, under params[pose0 + pose];
// an item whose flags[pose0 + pose] is not zero does nothing.  gate2 > 0: a contour pixel with |sd| > gate2 is far.  occlusion: a contour
// pixel that frame_occluded(depth, z, tol_m) hides is dropped; otherwise the depth is not read.
void launch_silref_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const float *depth,
                         const int32_t *sd, int H, int W, int gate2, float tol_m, bool occlusion, const SilrefParams *params, const int *flags,
                         int pose0, unsigned long long *acc);

// depth search (fp_pose_search; fp_pose_search.hip): per pose the sampled vertices and their normals against the
// frame's raw depth at n_steps pushes along the ray of the pose's origin; a record is ten 32-bit words, fp_pose_search_t's layout.
constexpr int SEARCH_THREADS = 256;
constexpr int SEARCH_MAX_STEPS = 64;                // = FP_SEARCH_MAX_STEPS (one wave picks the best step)
constexpr int SEARCH_MAX_POINTS = 4096;             // = FP_SEARCH_MAX_POINTS
constexpr int SEARCH_CLASSES = 6;                   // n_facing, n_inlier, n_front, n_behind, n_outside, n_missing
constexpr float SEARCH_MIN_COS2 = 0.04f;            // a point faces the camera when cos(normal, -ray) > 0.2, tested on squares
constexpr int SEARCH_STATUS_REFUSED_NEAR = 1;       // = FP_SEARCH_REFUSED_NEAR
struct SearchParams {
  int H, W;
  int P, vertex_step;   // points vertex_step * i, i < P = ceil(V / vertex_step)
  int n_steps;
  float step_m, tol_m;
};
struct SearchRec {
  int32_t n[SEARCH_CLASSES];
  int32_t score, best_step, n_points, status;
};
// pose p of the launch is poses[p] and writes out[p]; depth [H,W] is the raw depth
void launch_pose_search(hipStream_t s, const DeviceMesh &m, const FramePose *poses, int n, const float *depth, const SearchParams &S, SearchRec *out);

// host helpers (fp_host.cpp part of fp_api.hip)
std::vector<float> make_rotation_grid(int min_views, int inplane_steps);

}  // namespace fp
