// fp_api.hip -- the C ABI (include/foundationpose_amd.h) and the host-side orchestration that mirrors
// detection_6d::FoundationPose (reference D6F/src/foundationpose.cpp:108-458), MI355X-first:
//   * all per-hypothesis host work of the reference (crop windows, bbox, projection, pose update, arg-max) runs
//     on the device, so a Register is one stream of launches with a single D2H of the winning pose;
//   * render/crop kernels write the networks' fp16 input tensor directly (no fp32 blob, no concat pass);
//   * device buffers are allocated once per model and grown on demand (no per-call hipMalloc).
#include "../../include/foundationpose_amd.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <thread>
#include <cstring>
#include <dlfcn.h>
#include <link.h>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "fp_internal.h"
#include "fp_nn.h"

namespace fp {

static thread_local std::string g_last_error;
// Concurrency contract: a model is NOT re-entrant (like the reference, foundationpose.cpp:103-105: one renderer and its
// scratch per target), but different models may be driven from different host threads at the same time, each on its own
// non-blocking stream; their kernels overlap on the GPU.  (Round 1 serialised all models behind a process-wide lock to
// hide wrong results under exactly that overlap; the cause -- packed-f32 VALU instructions returning wrong values in lanes
// 48-63 while waves of another queue's kernel share the SIMD -- and the fix are in DESIGN.md section 9.)
void set_error(const std::string &msg) { g_last_error = msg; }

// One non-blocking utility stream per DEVICE, shared by all host threads under a lock (creation / loading / calibration paths only:
// nothing on the serving path uses it).  Per device, not per thread: a stream belongs to the device that was current when it was
// created, and a stream made by a transient host thread would outlive that thread inside the runtime.
static std::mutex g_util_mu;
static hipError_t utility_stream(hipStream_t *out) {
  static hipStream_t streams[64] = {nullptr};
  int d = 0;
  hipError_t e = hipGetDevice(&d);
  if (e != hipSuccess) return e;
  if (d < 0 || d >= 64) return hipErrorInvalidDevice;
  if (!streams[d] && (e = hipStreamCreateWithFlags(&streams[d], hipStreamNonBlocking)) != hipSuccess) { streams[d] = nullptr; return e; }
  *out = streams[d];
  return hipSuccess;
}
// Host <-> device copies of the creation / loading / calibration paths go through a PINNED staging buffer (two 4 MB halves,
// double-buffered) instead of handing the caller's pageable memory to hipMemcpyAsync: the runtime never has to lock or stage user
// pages, and it is the faster copy.  (Also tried against the fp_create SIGSEGV of DESIGN.md section 9; the fault is elsewhere.)
static hipError_t staging(unsigned char **buf, size_t *half) {
  static unsigned char *p = nullptr;   // (under g_util_mu)
  constexpr size_t HALF = (size_t)4 << 20;
  if (!p) {
    const hipError_t e = hipHostMalloc((void **)&p, 2 * HALF, hipHostMallocPortable | hipHostMallocMapped);
    if (e != hipSuccess) { p = nullptr; return e; }
  }
  *buf = p; *half = HALF;
  return hipSuccess;
}
// Host -> device through a KERNEL that reads the pinned, device-mapped staging block [r5]: no copy command on the creation / loading /
// calibration paths.  (The one native backtrace of the fp_create crash under a concurrent PyTorch stream -- DESIGN.md section 9 --
// ends inside hipMemcpyAsync's signal wait in the HIP 7.0 runtime PyTorch bundles; a kernel launch does not take that path.  The same
// trick carries Track's window upload, window_fetch_kernel.)
__global__ __launch_bounds__(256) void staged_upload_kernel(const unsigned char *__restrict__ src_mapped, unsigned char *__restrict__ dst, size_t n) {
  const size_t n16 = n / 16;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
    reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src_mapped)[i];
  if (blockIdx.x == 0 && threadIdx.x < (n & 15)) dst[n16 * 16 + threadIdx.x] = src_mapped[n16 * 16 + threadIdx.x];
}
// [r6] the Register's read-back {winner index, sampler status, pose} written straight into the model's pinned, device-mapped result
// block: one 18-lane kernel instead of three device -> host copy commands in front of the call's only synchronisation
__global__ void publish_result_kernel(const int *__restrict__ argmax, const int *__restrict__ sampler_status, const float *__restrict__ best_pose,
                                      int *__restrict__ out_mapped) {
  const int i = threadIdx.x;
  int v = 0;
  if (i == 0) v = argmax[0];
  else if (i == 1) v = sampler_status ? sampler_status[0] : 0;
  else if (i < 18) v = __float_as_int(best_pose[i - 2]);
  if (i < 18) out_mapped[i] = v;
  __threadfence_system();
}
// its neighbour for the pose fit: the winner's record into the model's pinned block (a second tiny publish, no copy command)
__global__ void publish_fit_kernel(const int *__restrict__ argmax, const PoseFitRec *__restrict__ recs, int N, PoseFitRec *__restrict__ out_mapped) {
  const int i = argmax[0];
  PoseFitRec r = {0, 0, 0, 0, 0, 0, 0};
  if (i >= 0 && i < N) r = recs[i];
  *out_mapped = r;
  __threadfence_system();
}
hipError_t memcpy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  std::lock_guard<std::mutex> lk(g_util_mu);
  hipStream_t s = nullptr;
  hipError_t e = utility_stream(&s);
  if (e != hipSuccess) return e;
  if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToHost) {
    e = hipMemcpyAsync(dst, src, bytes, kind, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
  }
  unsigned char *stage = nullptr;
  size_t half = 0;
  if ((e = staging(&stage, &half)) != hipSuccess) return e;
  hipEvent_t done[2] = {nullptr, nullptr};
  for (auto &ev : done) if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) { if (done[0]) (void)hipEventDestroy(done[0]); return e; }
  size_t off = 0;
  int slot = 0;
  bool used[2] = {false, false};
  while (off < bytes && e == hipSuccess) {
    const size_t n = std::min(half, bytes - off);
    unsigned char *h = stage + slot * half;
    if (used[slot]) e = hipEventSynchronize(done[slot]);   // the copy that last used this half has finished
    if (e != hipSuccess) break;
    if (kind == hipMemcpyHostToDevice) {
      std::memcpy(h, (const unsigned char *)src + off, n);
      unsigned char *h_dev = nullptr;
      if (((uintptr_t)((unsigned char *)dst + off) & 15) == 0 && hipHostGetDevicePointer((void **)&h_dev, h, 0) == hipSuccess) {
        const unsigned blocks = (unsigned)std::min<size_t>(1024, (n / 16 + 255) / 256 + 1);
        hipLaunchKernelGGL(staged_upload_kernel, dim3(blocks), dim3(256), 0, s, h_dev, (unsigned char *)dst + off, n);
        e = hipGetLastError();
      } else e = hipMemcpyAsync((unsigned char *)dst + off, h, n, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipEventRecord(done[slot], s);
      used[slot] = true;
    } else {   // device -> host: wait for the chunk, then hand it over
      e = hipMemcpyAsync(h, (const unsigned char *)src + off, n, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e == hipSuccess) std::memcpy((unsigned char *)dst + off, h, n);
    }
    off += n;
    slot ^= 1;
  }
  const hipError_t e2 = hipStreamSynchronize(s);
  for (auto &ev : done) (void)hipEventDestroy(ev);
  return e != hipSuccess ? e : e2;
}
hipError_t memset_sync(void *dst, int value, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_util_mu);
  hipStream_t s = nullptr;
  hipError_t e = utility_stream(&s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(dst, value, bytes, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}
std::atomic<unsigned long> g_alloc_epoch{0};

// ---- streams are RECYCLED, never destroyed [r4]: destroyed models park their stream here, new models take one.  (Tried as a remedy for
// the fp_create SIGSEGV under a concurrent PyTorch stream -- a signal wait inside the HIP 7.0 runtime PyTorch bundles, DESIGN.md
// section 9 -- where it changed nothing; kept because a serving process that adds and removes objects should not churn HSA queues.)
namespace {
std::mutex g_stream_pool_mu;
std::vector<std::pair<int, hipStream_t>> g_stream_pool;   // (device, stream)
}  // namespace
hipError_t stream_acquire(hipStream_t *out) {
  int d = 0;
  hipError_t e = hipGetDevice(&d);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lk(g_stream_pool_mu);
    for (size_t i = 0; i < g_stream_pool.size(); i++)
      if (g_stream_pool[i].first == d) {
        *out = g_stream_pool[i].second;
        g_stream_pool.erase(g_stream_pool.begin() + (long)i);
        return hipSuccess;
      }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);   // non-blocking: no implicit synchronisation with the legacy null stream
}
void stream_release(hipStream_t s) {   // (the caller has synchronised it; its device is current)
  int d = 0;
  if (!s || hipGetDevice(&d) != hipSuccess) return;
  std::lock_guard<std::mutex> lk(g_stream_pool_mu);
  g_stream_pool.emplace_back(d, s);
}

// ---- roctx (fp_internal.h): bound once, no-ops when the library is not there
namespace {
struct RoctxApi {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
};
const RoctxApi &roctx_api() {
  static const RoctxApi api = [] {
    RoctxApi a;
    void *h = nullptr;
    for (const char *name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (h) {
      a.push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
      a.pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!a.push || !a.pop) a.push = nullptr, a.pop = nullptr;
    }
    return a;
  }();
  return api;
}
}  // namespace
void roctx_push(const char *name) { if (roctx_api().push) (void)roctx_api().push(name); }
void roctx_pop() { if (roctx_api().pop) (void)roctx_api().pop(); }
#ifdef FP_TEST_HOOKS
static int g_icp_chunk = 0;   // fpt_icp_set_chunk: poses per chunk of fp_refine_depth (0: sized by ICP_SCRATCH_BYTES); only the test build changes it
static int g_vsd_chunk = 0;   // fpt_vsd_set_chunk: poses per chunk of fp_pose_vsd (0: sized by VSD_SCRATCH_BYTES); only the test build changes it
static int g_color_chunk = 0; // fpt_color_set_chunk: poses per chunk of fp_pose_color (0: sized by COLOR_SCRATCH_BYTES); only the test build changes it
static int g_silref_chunk = 0;   // fpt_silref_set_chunk: poses per chunk of fp_refine_silhouette (0: sized by SIL_SCRATCH_BYTES); only the test build changes it
static int g_sil_chunk = 0;   // fpt_silhouette_set_chunk: poses per chunk of fp_pose_silhouette (0: sized by SIL_SCRATCH_BYTES); only the test build changes it
static int g_calib_sweeps = 2, g_calib_tok = 1, g_calib_out = 1;   // A/B (fpt_set_calib_opts): steps of the 8-bit calibration
#else
static constexpr int g_icp_chunk = 0;
static constexpr int g_vsd_chunk = 0;
static constexpr int g_color_chunk = 0;
static constexpr int g_silref_chunk = 0;
static constexpr int g_sil_chunk = 0;
static constexpr int g_calib_sweeps = 2, g_calib_tok = 1, g_calib_out = 1;
#endif

// ------------------------------------------------------------------------------------------------
// Profiler
// ------------------------------------------------------------------------------------------------
ProfEntry &Profiler::get(const char *name) {
  for (auto &e : entries)
    if (e.name == name) return e;
  entries.emplace_back();
  entries.back().name = name;
  return entries.back();
}
hipEvent_t Profiler::ev() {
  if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void Profiler::begin(hipStream_t s, const char *name, double flops, double bytes) {
  // entries is a vector: take the index, pointers may move
  ProfEntry &e = get(name);
  e.calls++; e.flops += flops; e.bytes += bytes;
  cur = &e;
  cur_start = ev();
  (void)hipEventRecord(cur_start, s);
}
void Profiler::end(hipStream_t s) {
  hipEvent_t stop = ev();
  (void)hipEventRecord(stop, s);
  cur->pending.emplace_back(cur_start, stop);
  cur = nullptr;
}
void Profiler::collect() {
  for (auto &e : entries) {
    for (auto &pr : e.pending) {
      (void)hipEventSynchronize(pr.second);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, pr.first, pr.second);
      e.ms += ms;
      pool.push_back(pr.first);
      pool.push_back(pr.second);
    }
    e.pending.clear();
  }
}
void Profiler::reset() {
  collect();
  entries.clear();
}

// ------------------------------------------------------------------------------------------------
// a7: rotation grid (D6F/src/foundationpose_sampling.cpp:56-121,178-237); 42 icosphere views x inplane_steps
// ------------------------------------------------------------------------------------------------
namespace {
struct V3 { float x, y, z; };
V3 normalized(V3 p) {
  float n2 = p.x * p.x + p.y * p.y + p.z * p.z;
  if (n2 > 0.0f) { float n = std::sqrt(n2); p.x /= n; p.y /= n; p.z /= n; }
  return p;
}
std::vector<V3> icosphere(unsigned min_views) {
  std::vector<V3> verts;
  std::vector<std::array<int, 3>> faces;
  std::map<int64_t, int> cache;
  float t = (float)((1.0 + std::sqrt(5.0)) / 2.0);
  const float init[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                             {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  for (auto &p : init) verts.push_back(normalized(V3{p[0], p[1], p[2]}));
  const int f0[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                         {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                         {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  for (auto &f : f0) faces.push_back({f[0], f[1], f[2]});
  auto middle = [&](int i, int j) {
    int64_t sm = std::min(i, j), gr = std::max(i, j), key = (sm << 32) + gr;
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    V3 a = verts[i], b = verts[j];
    verts.push_back(normalized(V3{(a.x + b.x) / 2.0f, (a.y + b.y) / 2.0f, (a.z + b.z) / 2.0f}));
    cache[key] = (int)verts.size() - 1;
    return (int)verts.size() - 1;
  };
  while (verts.size() < min_views) {
    std::vector<std::array<int, 3>> nf;
    for (auto &f : faces) {
      int a = f[0], b = f[1], c = f[2];
      int ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
      nf.push_back({a, ab, ca}); nf.push_back({b, bc, ab}); nf.push_back({c, ca, bc}); nf.push_back({ab, bc, ca});
    }
    faces.swap(nf);
  }
  return verts;
}
}  // namespace

std::vector<float> make_rotation_grid(int min_views, int inplane_steps) {
  std::vector<float> out;
  auto verts = icosphere((unsigned)min_views);
  const double step = 360.0 / inplane_steps;
  for (auto &pos : verts) {
    V3 z = normalized(V3{-pos.x, -pos.y, -pos.z});
    V3 up{0, 0, 1};
    V3 x{up.y * z.z - up.z * z.y, up.z * z.x - up.x * z.z, up.x * z.y - up.y * z.x};
    if (x.x == 0.0f && x.y == 0.0f && x.z == 0.0f) x = V3{1, 0, 0};
    x = normalized(x);
    V3 y = normalized(V3{z.y * x.z - z.z * x.y, z.z * x.x - z.x * x.z, z.x * x.y - z.y * x.x});
    // cam_in_ob rotation columns x,y,z ; translation pos
    for (int k = 0; k < inplane_steps; k++) {
      float a = (float)((k * step) * M_PI / 180.0f);
      float s = std::sin(a), c = std::cos(a);
      // R = [x y z] * Rz(a): columns
      double cx[3] = {(double)(x.x * c + y.x * s), (double)(x.y * c + y.y * s), (double)(x.z * c + y.z * s)};
      double cy[3] = {(double)(x.x * -s + y.x * c), (double)(x.y * -s + y.y * c), (double)(x.z * -s + y.z * c)};
      double cz[3] = {(double)z.x * ((1.0f - c) + c), (double)z.y * ((1.0f - c) + c), (double)z.z * ((1.0f - c) + c)};
      double tt[3] = {pos.x, pos.y, pos.z};
      // ob_in_cam = inverse: rotation R^T (rows = columns of R), translation -R^T t
      float o[16];
      const double *cols[3] = {cx, cy, cz};
      for (int r = 0; r < 3; r++)
        for (int cc = 0; cc < 3; cc++) o[cc * 4 + r] = (float)cols[r][cc];
      for (int r = 0; r < 3; r++) o[12 + r] = (float)(-(cols[r][0] * tt[0] + cols[r][1] * tt[1] + cols[r][2] * tt[2]));
      o[3] = o[7] = o[11] = 0; o[15] = 1;
      out.insert(out.end(), o, o + 16);
    }
  }
  return out;
}

// GuessTranslation (D6F/src/foundationpose_sampling.cpp:250-298) on host buffers
template <typename T>
static int dev_alloc(T **p, size_t count) {
  FP_HIP_OK(hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T)));
  return 0;
}
template <typename T>
static void dev_free(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}
// Device scratch of the stage operators (a model's st_*, fr_*, sc_*, pe_*, vsd_*, icp_*, ps_*, col_*, sil_* blocks, used on stream s): grow-only,
// and nothing of the stream may still read a block that is replaced.  No captured graph reads these blocks, so unlike
// ensure_capacity / ensure_window this leaves the allocation epoch alone.
template <typename T>
static int grow_scratch(hipStream_t s, T *&p, size_t &cap, size_t need) {
  if (need <= cap) return 0;
  FP_HIP_OK(hipStreamSynchronize(s));
  dev_free(p);
  cap = 0;
  if (dev_alloc(&p, need)) return 1;
  cap = need;
  return 0;
}
// Two host steps of the stage operators (the others stand next to render_preconditions below; templates cannot, inside extern "C").
// A column-major 4 x 4 matrix as the linear part ROW-major and the translation, in the caller's number type: the one loop behind
// frame_pose (f32, what the kernels read) and rigid_from_colmajor (double, fp_pose_errors' host algebra).
template <typename T>
static void rigid_parts(const float *p, T *r, T *t) {
  for (int i = 0; i < 3; i++) {
    for (int c = 0; c < 3; c++) r[i * 3 + c] = (T)p[c * 4 + i];
    t[i] = (T)p[12 + i];
  }
}
// The (pose, tile) items of fp_pose_vsd and fp_refine_depth: launch(first, count) over the items [first, end) in runs of at most
// work_cap / 10 / walk items (walk: the faces an item walks), one at least: no launch above a tenth of the call's work cap.  The
// counters are integer atomics indexed by pose, so where a run is cut changes no result.
template <typename Launch>
static int launch_item_runs(size_t first, size_t end, long long work_cap, long long walk, Launch launch) {
  const size_t per_launch = (size_t)std::max<long long>(work_cap / 10 / walk, 1);
  while (first < end) {
    const size_t cnt = std::min(end - first, per_launch);
    if (launch(first, (int)cnt)) return 1;
    first += cnt;
  }
  return 0;
}
// pinned host memory and the device's address of it; a block whose device address cannot be had is freed again (*host stays as it was)
template <typename T>
static hipError_t pinned_mapped_alloc(T **host, T **dev, size_t bytes, unsigned flags) {
  T *h = nullptr;
  hipError_t e = hipHostMalloc((void **)&h, bytes, flags);
  if (e != hipSuccess) return e;
  if ((e = hipHostGetDevicePointer((void **)dev, h, 0)) != hipSuccess) { (void)hipHostFree(h); return e; }
  *host = h;
  return hipSuccess;
}

}  // namespace fp

using namespace fp;

struct Target {
  std::string name;
  DeviceMesh mesh;
};

// a calibration frame kept on the host between fp_calibrate_add_frame and fp_calibrate_finish
struct CalibFrame {
  std::vector<uint8_t> rgb, mask;
  std::vector<float> depth;
  int H = 0, W = 0;
  std::string target;
};

// the calibration record of one 8-bit precision (fp_calibrate; what fp_get_calibration_blob carries), [refiner, scorer] each: the
// per-channel |max| of the 15 trunk activations of the f16 networks the precision was quantised with ([15][512]) and the corrections
// solved against them (bias [13][512], token [512], output layer: refiner [8] = trans 3 | rot 3 | 0 0, scorer [512])
struct CalibRecord {
  std::vector<float> amax[2], bias_fix[2], tok_fix[2], out_fix[2];
  // [r5] per-frame channel means of the f16 trunk activations ([slots][15][512], slots <= 16: frame f goes to slot f % slots): the
  // INT8 weights are rounded with error feedback against them (fp_nn.hip quantise_q8)
  std::vector<float> fmeans[2];
  int slots = 0;
  bool valid() const { return !amax[0].empty(); }   // (a default-constructed record: the precision is not calibrated)
};

// what a begin leaves on the model for the finish of a LATER call: every begin starts from a cleared record, every finish takes it
struct RegisterPending {
  bool sampler = false;   // packed protocol: the begin ran the sampler and left its verdict to the finish
  int fit_n = 0;          // the begin enqueued the pose fit over this many (= all) hypotheses
};

struct fp_model {
  int device = 0;            // the HIP device the model lives on (fp_create_on); every entry point makes it current for its duration
  hipStream_t stream = nullptr;
  Profiler prof;
  float K[9];
  int max_h = 1080, max_w = 1920;
  int inplane_steps = 6;
  std::vector<Target> targets;
  std::vector<float> grid_host;  // [n_hyp*16]

  // frame
  int H = 0, W = 0;
  uint8_t *rgb_own = nullptr;
  float *depth_own = nullptr;
  FrameRef *frame_dev = nullptr;   // what kernels inside graphs read the frame through
  // [r6] a ring of 8 pinned, device-MAPPED record slots of 64 bytes each: a changed record reaches frame_dev through a kernel
  // (window_fetch_kernel), not a copy command
  uint8_t *frame_pinned = nullptr, *frame_pinned_dev = nullptr;
  // [r6] Register from HOST frames: rgb | depth | mask are packed into this pinned, device-mapped block (grown on demand) and fetched by
  // staged_upload_kernel -- no copy command and no runtime-internal staging of the caller's pageable pages on a serving path
  uint8_t *host_stage = nullptr, *host_stage_dev = nullptr;
  size_t host_stage_cap = 0;
  hipEvent_t host_stage_done = nullptr;   // recorded behind the last fetch: the block is rewritten only after it
  bool host_stage_pending = false;
  bool host_stage_fresh = false;   // this call's frame upload has just claimed the block (the mask goes behind it without waiting again)
  // [r4] frame_dev heads a device block [FrameRef, padded to 64 bytes | packed window]: Track's crop window of a host frame is packed
  // (record, rgb rows, depth rows) into the pinned twin win_stage and fetched from there by window_fetch_kernel, record included
  uint8_t *win_stage = nullptr, *win_stage_dev = nullptr;   // (host address / the device's mapping of it)
  size_t win_cap = 0;             // bytes of either block (0: no window path)
  FrameRef frame_pub = {nullptr, nullptr};                 // last published value
  unsigned frame_pub_count = 0;
  float *multi_io = nullptr, *multi_io_dev = nullptr;  // host-pinned [64 poses in | 64 poses out] of fp_track_multi
  std::vector<Target *> mg_sig;                        // the object sequence the multi-object graph was captured for
  bool track_pending = false;  // fp_track_submit without its fp_track_wait
  bool frame_partial = false;  // the model's copy of a host frame holds only the rows Track needed (stage operators refuse it)
  const uint8_t *rgb = nullptr;   // device
  const float *depth = nullptr;   // device
  float *erode = nullptr, *bilat = nullptr, *xyz = nullptr;
  // device-side sampler (GuessTranslation): rotation grid, scan state (int[8]), compacted depth list, mask copy
  float *grid_dev = nullptr;
  int *samp_state = nullptr;
  float *samp_vals = nullptr;
  uint8_t *mask_dev = nullptr;
  size_t samp_px_cap = 0;
  size_t frame_cap = 0;

  // per-hypothesis scratch
  int cap = 0;
  size_t vert_cap = 0;
  PoseRec *recs = nullptr;
  float *poses_dev = nullptr;
  float4 *clip = nullptr, *attr = nullptr;
  unsigned *tri_rows = nullptr;   // [cap, max_faces] row range of every triangle of every hypothesis (launch_tri_rows)
  size_t tri_cap = 0, max_faces = 0;
  __half *nn_in = nullptr;                  // [2*cap,84,84,32] (s2d, zero border 2)
  float *blob_a = nullptr, *blob_b = nullptr;  // [cap,160,160,6] f32 (blob-mode entry points only)
  float *trans_dev = nullptr, *rot_dev = nullptr, *scores_dev = nullptr, *feat_dev = nullptr;
  int *argmax_dev = nullptr;
  // one read-back per Register: device [pose16] + pinned host mirror {idx, sampler status, pose16}
  float *best_pose_dev = nullptr;
  int *result_pinned = nullptr, *result_pinned_dev = nullptr;  // 18 words, device-mapped [r6]: publish_result_kernel writes them (no D2H copy command)
  RegisterPending reg_pending;
  float *scores_all = nullptr;  // scores of the gathered hypotheses of every rank (sharded Register)
  int scores_all_cap = 0;
  float *gath_feat = nullptr, *gath_poses = nullptr;  // [n_total,512] / [n_total,16] unpacked from the all-gathered rows
  int gath_cap = 0;
  float *shard_send = nullptr, *shard_recv = nullptr;  // fp_register_sharded: persistent exchange buffers [per,528] / [world*per,528]
  size_t shard_send_cap = 0, shard_recv_cap = 0;
  int32_t *dbg_tri = nullptr;
  float *dbg_rast = nullptr;

  // networks per precision (loaded on demand from the weight files), activation arenas per precision (the border
  // positions of a tensor depend on its element size, so an arena serves one precision)
  std::string refiner_path, scorer_path;
  Net *refiner_p[N_PREC] = {nullptr}, *scorer_p[N_PREC] = {nullptr};
  NNScratch *ws_p[N_PREC] = {nullptr};
  int prec = PREC_F16;
  // float model of the rendering stage: true = multiply-adds contracted like the reference's nvcc -fmad=true build
  // (fp_geometry.hip "float model"), false = every operation separately rounded
  bool fmad = true;
  Net *refiner = nullptr, *scorer = nullptr;  // = refiner_p[prec], scorer_p[prec]
  NNScratch *ws = nullptr;                    // = ws_p[prec]
  int calib_session_prec = -1;                 // fp_calibrate_begin .. fp_calibrate_finish: the precision being calibrated (-1: no session)
  std::vector<CalibFrame> calib_frames; // host copies of the session's frames
  CalibRecord calib[N_PREC];   // (per precision: each may have been calibrated on other frames; applied when its networks are loaded / re-calibrated)
  bool calibrated(int prec) const { return prec >= 0 && prec < N_PREC && calib[prec].valid(); }
  // pinned staging for hypothesis poses: Register returns from its asynchronous section while the H2D copy may still be
  // queued, so the source must outlive the call (a local std::vector did not: found by the two-model serving test)
  float *track_io = nullptr, *track_io_dev = nullptr;  // host-pinned [hypothesis 16 | refined pose 16 | done flag] of Track and its device address
  bool track_flag_armed = false;   // the submitted Track ends in the kernel that raises the done flag (fp_track_wait polls it)
  float *poses_pinned = nullptr;
  int poses_pinned_cap = 0;
  unsigned long long *digests = nullptr;  // [16] device, debug checkpoints (null = off)

  // pose fit (fp_set_pose_fit).  Nothing below is allocated before the option is first used.
  bool fit_on = false;
  float fit_tol_m = 0.005f;
  unsigned long long *fit_acc = nullptr;   // device [FP_MAX_BATCH, 4]: zeroed once, left zeroed by every launch of the kernel
  PoseFitRec *fit_rec = nullptr;           // device [2 * FP_MAX_BATCH]: Register's records | fp_pose_fit_eval's
  PoseFitRec *fit_io = nullptr, *fit_io_dev = nullptr;   // host-pinned, device-mapped [64 Track records | the Register winner's]
  int fit_track_n = 0;                     // records the last Track left in fit_io (0: none, fit_track_why says why)
  std::string fit_track_why = "no Track has run", fit_reg_why = "no Register has run";
  float fit_track_tol[64] = {0}, fit_track_diam[64] = {0};
  int fit_reg_n = 0, fit_reg_index = -1;   // records of the last Register in fit_rec (0: none) and its winner
  float fit_reg_tol = 0, fit_reg_diam = 0;

  // depth filter (fp_set_depth_filter): the crops read D' = bilateral(erode(depth)) out of `bilat` through the frame
  // record.  No buffer of its own: Register's sampler leaves the whole frame's D' there anyway, Track fills its window of it.
  bool dfilt_on = false;

  // Scratch of the stage operators (DESIGN.md sections 4.8 - 4.16: fp_render_pose, fp_render_scene, fp_pose_errors, fp_pose_vsd,
  // fp_refine_depth, fp_pose_search, fp_pose_color, fp_pose_silhouette, fp_refine_silhouette).  Nothing below is allocated before the first call that needs it, and every block only grows
  // (grow_scratch).  One rule makes all of it safe, and lets the calls share the st_* blocks: every one of these calls holds the
  // SerialGuard from its first line to its last and leaves the stream synchronised, so no two of them are ever live together
  // (fp_register_depth runs the search and then the ICP, each to its end); and no captured graph reads any of these blocks, so
  // growing one never touches the allocation epoch.
  int4 *st_snap = nullptr;                 // [st_snap_cap] {xi, yi, bits(z), 0}: the vertices of one mesh under one pose or a chunk of poses (VSD: estimates | truths), or all objects' of a scene
  float4 *st_cam = nullptr;                // [st_cam_cap] their camera-space copies, for the calls that shade or need normals
  FramePose *st_poses = nullptr;           // [st_pose_cap] the poses of a call (VSD: estimates [N] | truths [n_gt]; ICP: of one evaluation pass)
  int2 *st_items = nullptr;                // [st_item_cap] the (pose of the chunk, tile) work list of a chunk (VSD) or a pass (ICP)
  size_t st_snap_cap = 0, st_cam_cap = 0, st_pose_cap = 0, st_item_cap = 0;
  std::vector<FramePose> st_poses_host;    // (owned by the model: the source of an asynchronous copy must outlive the call's frame)
  std::vector<int2> st_items_host;

  // what only the frame-resolution renderers need (sections 4.8 and 4.9, which share fr_out)
  int *fr_flag = nullptr;       // fp_render_pose's refusal word
  uint8_t *fr_out = nullptr;    // [fr_out_bytes] FP_HOST outputs are rendered here first: the call's wanted planes, each 256-byte aligned
  size_t fr_out_bytes = 0;

  // what only fp_render_scene needs
  SceneTable *sc_table = nullptr;          // device copy of sc_table_host
  SceneTable *sc_table_host = nullptr;     // (owned by the model: the source of an asynchronous copy must outlive the call's frame)
  int *sc_work = nullptr;                  // [sc_work_cap] flags | total | counters | tile counts | offsets | cursors (scene_work_words)
  unsigned *sc_list = nullptr;             // [sc_list_cap] the tiles' triangle lists
  size_t sc_work_cap = 0, sc_list_cap = 0;

  // pose errors (fp_pose_errors)
  float *pe_mats = nullptr;                // [pe_mat_cap] floats: estimates [N, 12] | relative transforms [N, 12] | composites [N (S + 1), 12]
  PoseErrPair *pe_pairs = nullptr;         // [pe_pair_cap] the paired kernel's record per (pose, symmetry)
  unsigned long long *pe_sums = nullptr;   // [FP_MAX_BATCH] the nearest-neighbour kernel's sums
  size_t pe_mat_cap = 0, pe_pair_cap = 0;
  std::vector<float> pe_mats_host;         // (owned by the model: the source of an asynchronous copy must outlive the call's frame)
  std::vector<PoseErrPair> pe_pairs_host;

  // visible surface discrepancy (fp_pose_vsd): the blocks whose layout is the call's own
  int *vsd_words = nullptr;                // [vsd_word_cap] counters [N, VSD_WORDS] | refusal words of the estimates [N] | of the truths [n_gt]
  float *vsd_plane = nullptr;              // [vsd_plane_cap] n_gt == 1: the one truth's model depth [H, W]
  size_t vsd_word_cap = 0, vsd_plane_cap = 0;

  // depth refinement (fp_refine_depth): likewise
  IcpParams *icp_params = nullptr;         // [icp_param_cap] of the poses of one evaluation pass
  unsigned long long *icp_acc = nullptr;   // [icp_acc_cap] accumulators [n, ICP_WORDS] | refusal words [n] (32-bit, behind the accumulators)
  size_t icp_param_cap = 0, icp_acc_cap = 0;
  std::vector<IcpParams> icp_params_host;  // (owned by the model, like st_poses_host)
  std::vector<unsigned long long> icp_acc_host;

  // colour agreement (fp_pose_color): likewise
  unsigned long long *col_acc = nullptr;   // [col_acc_cap] accumulators [N, COLOR_WORDS] | refusal words [N] (32-bit, behind the accumulators)
  size_t col_acc_cap = 0;
  std::vector<unsigned long long> col_acc_host;

  // silhouette agreement (fp_mask_distance / fp_pose_silhouette): likewise
  uint8_t *sil_mask = nullptr;             // [sil_mask_cap] the copy of a host mask
  uint16_t *sil_g = nullptr;               // [sil_g_cap] the column distances of the two seed sets, [2, H, W]
  uint32_t *sil_d2 = nullptr;              // [sil_d2_cap] the squared distances to the mask | to the other pixels, [2, H, W]
  size_t sil_mask_cap = 0, sil_g_cap = 0, sil_d2_cap = 0;
  unsigned long long *sil_acc = nullptr;   // [sil_acc_cap] {n_mask, T} | accumulators [N, SIL_WORDS] | 32-bit words: seeds [2], refusals [N]
  size_t sil_acc_cap = 0;
  std::vector<unsigned long long> sil_acc_host;
  // silhouette refinement (fp_refine_silhouette): likewise; the mask copy, the column distances and the two maps are the block above
  int32_t *silref_sd = nullptr;            // [silref_sd_cap] the signed squared distance of the call's mask, [H, W]
  size_t silref_sd_cap = 0;
  SilrefParams *silref_params = nullptr;   // [silref_param_cap] of the poses of one evaluation pass
  unsigned long long *silref_acc = nullptr;   // [silref_acc_cap] {n_mask, T} | seeds (two 32-bit words) | accumulators [n, SILREF_WORDS] | refusal words [n] (32-bit)
  size_t silref_param_cap = 0, silref_acc_cap = 0;
  std::vector<SilrefParams> silref_params_host;
  std::vector<unsigned long long> silref_acc_host;

  // depth search (fp_pose_search): likewise
  SearchRec *ps_recs = nullptr;            // [ps_rec_cap] the records of the call's poses
  size_t ps_rec_cap = 0;
  std::vector<SearchRec> ps_recs_host;

  // Track is launch-bound (~60 short kernels): after one eager call (allocations settle) the launch chain is captured
  // into a hipGraph and replayed.  The graph bakes buffer addresses, so it is keyed by g_alloc_epoch.
  // (Register's ~110 launches are replayed the same way: inter-kernel gaps are ~4 % of a 12 ms Register.)
  struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    Target *target = nullptr;
    int H = 0, W = 0, itr = 0, n = 0, prec = 0;
    unsigned long epoch = 0;
    int eager_calls = 0;
  } tg, rg, mg;  // Track body / Register body / multi-object Track body
  bool use_graphs = true;

  Target *find(const char *name) {
    for (auto &t : targets)
      if (t.name == name) return &t;
    return nullptr;
  }
  int n_hyp() const { return 42 * inplane_steps; }
};


// ---- debug checkpoints (tools/dbg_concurrent.py): order-independent 64-bit digest of a device buffer per pipeline stage
__global__ void fp_digest_kernel(const uint32_t *p, size_t n, unsigned long long *out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long acc = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) acc += (unsigned long long)p[i] * (2654435761ull + 2 * (i % 1000003ull));
  if (acc) atomicAdd(out, acc);
}
static void checkpoint(fp_model *m, int slot, const void *buf, size_t bytes) {
#ifndef FP_TEST_HOOKS
  (void)m; (void)slot; (void)buf; (void)bytes;
  return;
#endif
  if (!m->digests || !buf) return;
  hipLaunchKernelGGL(fp_digest_kernel, dim3(512), dim3(256), 0, m->stream, (const uint32_t *)buf, bytes / 4, m->digests + slot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) std::fprintf(stderr, "checkpoint %d (%p, %zu B): %s\n", slot, buf, bytes, hipGetErrorString(e));
}

static int ensure_capacity(fp_model *m, int N, size_t V) {
  if (N > m->cap) {
    g_alloc_epoch++;
    dev_free(m->recs); dev_free(m->poses_dev); dev_free(m->nn_in); dev_free(m->blob_a); dev_free(m->blob_b);
    dev_free(m->trans_dev); dev_free(m->rot_dev); dev_free(m->scores_dev); dev_free(m->feat_dev);
    dev_free(m->clip); dev_free(m->attr); dev_free(m->dbg_tri); dev_free(m->dbg_rast);
    m->vert_cap = 0;
    int cap = std::max(N, 8);
    if (dev_alloc(&m->recs, cap)) return 1;
    if (dev_alloc(&m->poses_dev, (size_t)cap * 16)) return 1;
    if (dev_alloc(&m->nn_in, (size_t)2 * cap * FP_NN_IN_IMG_HALFS)) return 1;
    // zero borders are written once here; the raster / crop kernels only ever store image interiors
    FP_HIP_OK(hipMemsetAsync(m->nn_in, 0, (size_t)2 * cap * FP_NN_IN_IMG_HALFS * sizeof(__half), m->stream));
    if (dev_alloc(&m->trans_dev, (size_t)cap * 3)) return 1;
    if (dev_alloc(&m->rot_dev, (size_t)cap * 3)) return 1;
    if (dev_alloc(&m->scores_dev, (size_t)cap)) return 1;
    if (dev_alloc(&m->feat_dev, (size_t)cap * 512)) return 1;
    m->cap = cap;
  }
  if ((size_t)m->cap * V > m->vert_cap) {
    g_alloc_epoch++;
    dev_free(m->clip); dev_free(m->attr);
    if (dev_alloc(&m->clip, (size_t)m->cap * V)) return 1;
    if (dev_alloc(&m->attr, (size_t)m->cap * V)) return 1;
    m->vert_cap = (size_t)m->cap * V;
  }
  // row ranges: for the largest mesh of the model (any target may be rendered) and for the batch sizes plan_render uses them at
  const size_t tri_need = (size_t)std::min(m->cap, RENDER_TRI_ROWS_MAX_N) * m->max_faces;
  if (V > 0 && tri_need > m->tri_cap) {
    g_alloc_epoch++;
    dev_free(m->tri_rows);
    m->tri_cap = 0;
    if (dev_alloc(&m->tri_rows, tri_need)) return 1;
    m->tri_cap = tri_need;
  }
  return 0;
}

static int ensure_blobs(fp_model *m) {
  size_t n = (size_t)m->cap * FP_CROP_HW * FP_CROP_HW * 6;
  if (!m->blob_a && dev_alloc(&m->blob_a, n)) return 1;
  if (!m->blob_b && dev_alloc(&m->blob_b, n)) return 1;
  return 0;
}

static int check_frame_args(fp_model *m, int H, int W, const char *target_name, Target **t) {
  // CheckInputArguments (D6F/src/foundationpose.cpp:155-179)
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(H > 0 && W > 0 && H <= m->max_h && W <= m->max_w, "[FoundationPose] Got rgb/depth/mask with unexpected size !");
  if (target_name) {
    *t = m->find(target_name);
    FP_CHECK(*t != nullptr,
             "[FoundationPose] Register Got Invalid `target_name` which was not provided to FoundationPose instance!!!");
  }
  return 0;
}

// render + crop for N poses already in m->poses_dev; writes the fp16 network input (both halves) or fp32 blobs.  WHAT is launched
// is plan_render's decision (fp_geometry.hip); this function builds the query and runs the plan's steps
// n_crop: number of observed crops to produce (N, or 1 when every hypothesis shares the same translation)
static int render_and_crop(fp_model *m, Target *t, int N, float crop_ratio, OutMode mode, void *out_a, void *out_b,
                           int32_t *dbg_tri, float *dbg_rast, int n_crop = -1, const float *poses_src = nullptr, PoseRec *recs = nullptr) {
  if (n_crop < 0) n_crop = N;
  if (!recs) recs = m->recs;   // (fp_track_multi: the records of one object group inside the batch)
  hipStream_t s = m->stream;
  const size_t out_bytes = (mode == OUT_F32X6 ? 24.0 : 16.0) * FP_CROP_HW * FP_CROP_HW;  // both 2-byte modes: 16 B per pixel
  const float *poses = poses_src ? poses_src : m->poses_dev;
  const DeviceMesh &mesh = t->mesh;
  RenderQuery q;
  q.N = N; q.mode = mode; q.out_a = out_a != nullptr; q.out_b = out_b != nullptr; q.taps = dbg_tri || dbg_rast; q.prof = m->prof.on;
  q.F = mesh.F; q.tri_cap = m->tri_rows ? m->tri_cap : 0;
  const RenderPlan plan = plan_render(q);
  unsigned *const rows = plan.row_ranges != ROW_RANGES_NONE ? m->tri_rows : nullptr;
  switch (plan.front) {
    case FRONT_SETUP: {
      ProfScope ps(&m->prof, s, "pose_setup");
      launch_pose_setup(s, poses, N, m->K, m->H, m->W, crop_ratio, mesh.diameter, recs);
    } break;
    case FRONT_SETUP_VERTEX: {   // pose set-up (crop window, bounding box, projection) is computed inside the vertex kernel: one launch less per render
      ProfScope ps(&m->prof, s, "vertex", 0, (double)N * mesh.V * 32.0 + mesh.V * 24.0);
      launch_setup_vertex(s, mesh, poses, N, m->K, m->H, m->W, crop_ratio, mesh.diameter, recs, m->clip, m->attr, m->fmad);
    } break;
    case FRONT_SETUP_VERTEX_CROP:   // tiny batches (Track): set-up + vertex stage + crop warp + the triangles' row ranges as ONE launch
      launch_setup_vertex_crop(s, mesh, poses, N, m->K, m->H, m->W, crop_ratio, mesh.diameter, recs, m->clip, m->attr, m->fmad, m->frame_dev,
                               n_crop, mode, out_b, plan.row_ranges == ROW_RANGES_BY_FRONT ? rows : nullptr);
      break;
  }
  if (plan.row_ranges == ROW_RANGES_OWN_LAUNCH) {
    ProfScope ps(&m->prof, s, "tri_rows", 0, (double)N * mesh.F * (12.0 + 48.0 + 4.0));
    launch_tri_rows(s, mesh, N, m->clip, rows);
  }
  if (plan.front != FRONT_SETUP) {
    ProfScope ps(&m->prof, s, "raster_shade", 0, (double)N * (out_bytes + mesh.V * 32.0 + mesh.F * 12.0));
    FP_CHECK(launch_raster_shade(s, plan, mesh, recs, N, m->clip, m->attr, mode, out_a, dbg_tri, dbg_rast, m->fmad, rows),
             "[FoundationPose] internal error: no rasteriser instantiation for the render plan");
  }
  if (plan.crop_launch) {
    ProfScope ps(&m->prof, s, "crop_warp", 0, (double)n_crop * out_bytes);
    launch_crop(s, m->frame_dev, m->H, m->W, m->K, recs, n_crop, mesh.diameter, mode, out_b);
  }
  FP_HIP_OK(hipGetLastError());
  return 0;
}

static int upload_frame_async(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, int row0 = 0, int row1 = -1, int col0 = 0, int col1 = -1,
                              const TrackWindow *filt = nullptr);
static int set_rotation_grid(fp_model *m, int steps);
static int publish_record(fp_model *m, const FrameRef &want);

static void drop_graph(fp_model::GraphSlot &g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr; g.graph = nullptr; g.eager_calls = 0;
}

// every captured body bakes the float model, the precision and (FP8) the per-tensor activation scales in as kernel arguments:
// anything that changes one of them drops ALL three graphs
static void invalidate_graphs(fp_model *m) {
  drop_graph(m->tg);
  drop_graph(m->rg);
  drop_graph(m->mg);
}

// whether a call's launch chain may be captured and replayed: not while profiling events or debug digests sit between the launches
static bool graphable(const fp_model *m, int refine_itr) { return m->use_graphs && !m->prof.on && !m->digests && refine_itr >= 1; }

// Runs `body` (a chain of launches on m->stream reading / writing only model-owned buffers): eagerly the first time a
// (target, H, W, itr, n) configuration is seen, captured into a hipGraph on the second call once allocations have
// settled (the graph bakes buffer addresses, so it is keyed by g_alloc_epoch), replayed from then on.
template <class Body>
static int run_graphed(fp_model *m, fp_model::GraphSlot &g, Target *t, int H, int W, int itr, int n, bool graphable, Body body) {
  const bool same = g.target == t && g.H == H && g.W == W && g.itr == itr && g.n == n && g.prec == m->prec && g.epoch == g_alloc_epoch;
  if (graphable && same && g.exec) {
    FP_HIP_OK(hipGraphLaunch(g.exec, m->stream));
  } else if (graphable && same && g.eager_calls >= 1) {
    drop_graph(g);
    FP_HIP_OK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
    int rc = body();
    hipError_t e = hipStreamEndCapture(m->stream, &g.graph);
    if (rc || e != hipSuccess || hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0) != hipSuccess) {
      drop_graph(g);
      m->use_graphs = false;  // fall back to eager launches for good
      if (body()) return 1;
    } else {
      g.eager_calls = 1;
      FP_HIP_OK(hipGraphLaunch(g.exec, m->stream));
    }
  } else {
    if (!same) { drop_graph(g); g.target = t; g.H = H; g.W = W; g.itr = itr; g.n = n; g.prec = m->prec; }
    if (body()) return 1;
    g.epoch = g_alloc_epoch;  // allocations made by this eager call are now settled
    g.eager_calls = graphable ? g.eager_calls + 1 : 0;
  }
  return 0;
}

// ---- packed exchange buffers of a sharded Register: row = [pooled score feature 512 | refined pose 16]
// sampler_status: the device-side verdict word of THIS rank's sampler run (0 = poses valid): anything else poisons the rows with
// NaNs, so that every rank's finish reports the failure -- a rank whose sampler failed must not feed garbage rows to ranks that
// would otherwise succeed (the verdict itself reaches the host only with the finish half's single synchronisation)
__global__ void pack_shard_kernel(const float *__restrict__ feat, const float *__restrict__ poses, int count, int per,
                                  float *__restrict__ packed, const int *__restrict__ sampler_status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per * 528) return;
  const int r = i / 528, c = i - r * 528;
  if (sampler_status && *sampler_status != 0) { packed[i] = __int_as_float(0x7fc00000); return; }
  packed[i] = r >= count ? 0.f : (c < 512 ? feat[(size_t)r * 512 + c] : poses[(size_t)r * 16 + (c - 512)]);
}
// gathered rows are already in global hypothesis order (contiguous shards of `per` rows, padding only behind row n_total)
__global__ void unpack_shards_kernel(const float *__restrict__ gathered, int n_total, float *__restrict__ feat,
                                     float *__restrict__ poses) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_total * 528) return;
  const int r = i / 528, c = i - r * 528;
  if (c < 512) feat[(size_t)r * 512 + c] = gathered[i];
  else poses[(size_t)r * 16 + (c - 512)] = gathered[i];
}

// Escape hatch (off by default): FP_SERIALIZE_MODELS=1 in the environment makes the synchronous entry points of ALL models in the
// process (Register, Track, fp_track_multi, FP8 calibration) take one process-wide lock for their whole duration, so that kernels
// of two models are never co-resident.  This is the round-1 behaviour; it exists because the packed-f32 erratum behind the
// removal of that lock was mitigated, not reproduced in isolation.  The pipelined fp_track_submit /
// fp_track_wait pair is not covered (it exists to overlap models).
// Lifetime lock [r3]: every compute entry point holds it SHARED for the duration of the call, fp_create / fp_destroy / fp_net_create /
// fp_net_destroy hold it EXCLUSIVE -- a model is never built or torn down (hundreds of allocations, uploads, a stream) while another
// thread of the process is inside a Register / Track call capturing or replaying its graphs.  (Two of ~20 runs of the widened
// concurrency test died with SIGSEGV inside fp_register_shard_begin on two threads while the main thread was inside fp_create;
// the calls themselves share nothing but the HIP runtime.)  Calls still run concurrently with each other; GPU work already enqueued
// keeps running during a creation.  A guard nested inside another of the same thread takes it once (thread-local depth).
static std::shared_mutex g_life_rw;
static thread_local int g_life_depth = 0;
struct LifeExclusive {   // (entry points nested inside -- fp_calibrate_fp8 runs a Register -- see depth > 0 and take nothing)
  LifeExclusive() { g_life_rw.lock(); ++g_life_depth; }
  ~LifeExclusive() { --g_life_depth; g_life_rw.unlock(); }
  LifeExclusive(const LifeExclusive &) = delete;
  LifeExclusive &operator=(const LifeExclusive &) = delete;
};
// Device affinity [r4]: a model remembers the device it was created on and every entry point makes that device current for the
// duration of the call (and puts the caller's device back), so a single-process multi-GPU host -- one thread per GPU, or one thread
// walking over the models -- cannot launch a model's work on the wrong device.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  explicit DeviceScope(int dev) {
    if (dev < 0) return;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) { prev = cur; switched = true; }
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope &) = delete;
  DeviceScope &operator=(const DeviceScope &) = delete;
};
// fp_register_sharded with more than one rank runs WITHOUT the FP_SERIALIZE_MODELS lock: a host with one thread per rank would
// deadlock on it (the thread inside the finish half's stream synchronisation holds the lock while its all-gather waits for ranks
// whose threads cannot enqueue theirs), and the ranks of a collective live on different devices, where the co-residency the lock
// exists to prevent cannot happen.
static thread_local bool g_no_serial = false;
struct SerialGuard {
  std::unique_lock<std::recursive_mutex> lk;
  bool shared_held = false;
  DeviceScope dev;
  explicit SerialGuard(int device) : dev(device) {
    if (g_life_depth++ == 0) { g_life_rw.lock_shared(); shared_held = true; }
    static const bool on = [] { const char *e = std::getenv("FP_SERIALIZE_MODELS"); return e && *e && *e != '0'; }();
    static std::recursive_mutex mu;
    if (on && !g_no_serial) lk = std::unique_lock<std::recursive_mutex>(mu);
  }
  ~SerialGuard() {
    if (lk.owns_lock()) lk.unlock();
    --g_life_depth;
    if (shared_held) g_life_rw.unlock_shared();
  }
  SerialGuard(const SerialGuard &) = delete;
  SerialGuard &operator=(const SerialGuard &) = delete;
};

// Exception barrier of the C ABI: every entry point below that can allocate on the host (std::vector / std::string / new) is a
// function-try-block ending in one of these; nothing is thrown across the extern "C" boundary.
static int caught_exception() noexcept {
  try {
    try { throw; }
    catch (const std::bad_alloc &) { set_error("[FoundationPose] out of host memory"); }
    catch (const std::exception &e) { set_error(std::string("[FoundationPose] internal error: ") + e.what()); }
    catch (...) { set_error("[FoundationPose] internal error (unknown exception)"); }
  } catch (...) {
  }
  return 1;
}
#define FP_CATCH_INT catch (...) { return caught_exception(); }
#define FP_CATCH_PTR catch (...) { caught_exception(); return nullptr; }

extern "C" {

#ifdef FP_TEST_HOOKS
// fp_pose_vsd works through its poses in chunks of `poses` (0: the library's own size): a batch test of the chunk seams at small N
void fpt_vsd_set_chunk(int poses) { g_vsd_chunk = poses > 0 ? poses : 0; }
// the same for fp_refine_depth
void fpt_icp_set_chunk(int poses) { g_icp_chunk = poses > 0 ? poses : 0; }
// the same for fp_pose_color
void fpt_color_set_chunk(int poses) { g_color_chunk = poses > 0 ? poses : 0; }
// the same for fp_pose_silhouette
void fpt_silhouette_set_chunk(int poses) { g_sil_chunk = poses > 0 ? poses : 0; }
// the same for fp_refine_silhouette
void fpt_silref_set_chunk(int poses) { g_silref_chunk = poses > 0 ? poses : 0; }
void fpt_set_calib_opts(int sweeps, int tok, int out) { g_calib_sweeps = sweeps; g_calib_tok = tok; g_calib_out = out; }
// A/B hook: hipGraph replay of the Track / Register bodies on or off for one model
int fpt_model_use_graphs(fp_model *m, int on) {
  m->use_graphs = on != 0;
  invalidate_graphs(m);
  return 0;
}

// poison the current precision's network scratch (nn_scratch_poison; kind 0 quiet NaN, 1 +-largest finite) and wait for it
int fpt_model_poison(fp_model *m, int kind) {
  if (!m->ws) return 0;
  if (nn_scratch_poison(m->ws, m->prec == PREC_BF16 ? DT_BF16 : DT_F16, kind, m->stream)) return 1;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

// Plan-only forward pass (tests/test_layers_gpu.py): grows the model's buffers to N like a real call, then runs the host side of one
// network call at the model's precision -- kind 0 = refiner_forward (shared_b as Register's first refine iteration), 1 = scorer_features +
// scorer_head over N, 2 = scorer_features alone (a Register shard) -- with every network launch suppressed, so that the armed launch log
// (fpt_launch_log_arm) holds exactly what the real call would launch.  The inputs are whatever nn_in holds: nothing is uploaded.
int fpt_plan_forward(fp_model *m, int kind, int N, int shared_b) try {
  FP_CHECK(m && kind >= 0 && kind <= 2 && N >= 1 && N <= FP_MAX_BATCH, "[FoundationPose] fpt_plan_forward: invalid arguments");
  FP_CHECK(kind == 0 ? m->refiner != nullptr : m->scorer != nullptr, "[FoundationPose] fpt_plan_forward: weights not loaded");
  SerialGuard serial(m->device);
  if (ensure_capacity(m, N, 0)) return 1;
  struct PlanOnly {
    PlanOnly() { nn_plan_only(true); }
    ~PlanOnly() { nn_plan_only(false); }
  } plan;
  if (kind == 0) {
    if (refiner_forward(m->stream, &m->prof, m->refiner, m->ws, m->nn_in, N, m->trans_dev, m->rot_dev, shared_b ? 1 : 0)) return 1;
  } else {
    if (scorer_features(m->stream, &m->prof, m->scorer, m->ws, m->nn_in, N, m->feat_dev)) return 1;
    if (kind == 1 && scorer_head(m->stream, &m->prof, m->scorer, m->ws, m->feat_dev, N, m->scores_dev)) return 1;
  }
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// bit 0: graphs still enabled (a failed capture disables them), bit 1: Track graph instantiated, bit 2: Register graph
int fpt_model_graph_state(fp_model *m) { return (m->use_graphs ? 1 : 0) | (m->tg.exec ? 2 : 0) | (m->rg.exec ? 4 : 0); }

// fp_render_pose's host-side screen bound without a GPU (tests/test_frame_render_bound_cpu.py): tiles [tx0, tx1] x [ty0, ty1] of an H x W frame
// for a column-major pose, row-major K and a vertex-norm bound
int fpt_frame_tile_bound(const float pose[16], const float K[9], double radius, int H, int W, int out4[4]) {
  FramePose P;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) P.r[r * 3 + c] = pose[c * 4 + r];
    P.t[r] = pose[12 + r];
  }
  P.fx = K[0]; P.cx = K[2]; P.fy = K[4]; P.cy = K[5];
  const FrameTileBound b = frame_tile_bound(P, radius, H, W);
  out4[0] = b.tx0; out4[1] = b.ty0; out4[2] = b.tx1; out4[3] = b.ty1;
  return 0;
}

// fp_render_scene's sizing without a GPU (tests/test_scene_render_ref_cpu.py): the tile grid of an H x W frame and the 32-bit words of the
// binning block that holds the refusal words, the counters and three per-tile arrays
int fpt_scene_sizing(int H, int W, int out3[3]) {
  out3[0] = scene_tiles_x(W); out3[1] = scene_tiles_y(H);
  out3[2] = (int)scene_work_words(H, W);
  return 0;
}

// debug: enable the stage digests and read them back (16 slots; zeroed by every read)
int fpt_digests(fp_model *m, unsigned long long out[16]) {
  if (!m->digests) {
    FP_HIP_OK(hipMalloc((void **)&m->digests, 16 * 8));
    FP_HIP_OK(fp::memset_sync(m->digests, 0, 16 * 8));
    return 0;
  }
  FP_HIP_OK(hipMemcpyAsync(out, m->digests, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipMemsetAsync(m->digests, 0, 16 * 8, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

// debug: digests of every long-lived device buffer of an (idle) model: recs, poses, clip, attr, nn_in, trans, rot,
// scores, feat, arena, arena f32 (11 values) -- to detect writes coming from OTHER models' kernels
int fpt_digest_buffers(fp_model *m, unsigned long long out[16]) {
  unsigned long long *d = nullptr;
  FP_HIP_OK(hipMalloc((void **)&d, 16 * 8));
  FP_HIP_OK(hipMemsetAsync(d, 0, 16 * 8, m->stream));
  const void *ab = nullptr, *af = nullptr;
  size_t abytes = 0, afbytes = 0;
  if (m->ws) nn_scratch_debug_info(m->ws, &ab, &abytes, &af, &afbytes);
  size_t V = m->targets.empty() ? 0 : (size_t)m->targets[0].mesh.V;
  const DeviceMesh *dm = m->targets.empty() ? nullptr : &m->targets[0].mesh;
  struct { const void *p; size_t n; } bufs[16] = {
      {m->recs, (size_t)m->cap * sizeof(PoseRec)}, {m->poses_dev, (size_t)m->cap * 64}, {m->clip, m->vert_cap * 16},
      {m->attr, m->vert_cap * 16}, {m->nn_in, (size_t)2 * m->cap * FP_NN_IN_IMG_HALFS * 2}, {m->trans_dev, (size_t)m->cap * 12},
      {m->rot_dev, (size_t)m->cap * 12}, {m->scores_dev, (size_t)m->cap * 4}, {m->feat_dev, (size_t)m->cap * 2048},
      {ab, abytes}, {af, afbytes},
      {dm ? dm->verts : nullptr, V * 12}, {dm ? dm->normals : nullptr, V * 12}, {dm ? dm->uvs : nullptr, V * 8},
      {dm ? (const void *)dm->faces : nullptr, dm ? (size_t)dm->F * 12 : 0}, {dm ? (const void *)dm->tex : nullptr, dm ? (size_t)dm->TH * dm->TW * 3 : 0}};
  for (int i = 0; i < 16; i++)
    if (bufs[i].p && bufs[i].n >= 4)
      hipLaunchKernelGGL(fp_digest_kernel, dim3(1024), dim3(256), 0, m->stream, (const uint32_t *)bufs[i].p, bufs[i].n / 4, d + i);
  FP_HIP_OK(hipMemcpyAsync(out, d, 16 * 8, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  (void)hipFree(d);
  return 0;
}

// debug: allocate the vertex-stage intermediates buffer (launches with N == 64 fill it) / read it back
long long fpt_vertex_dbg(fp_model *m, void *dst, long long bytes) {
  if (!fp::g_vertex_dbg) {
    float4 *p = nullptr;
    if (hipMalloc((void **)&p, (size_t)bytes) != hipSuccess) return -1;
    fp::g_vertex_dbg = p;
    return 0;
  }
  if (hipMemcpyAsync(dst, fp::g_vertex_dbg, (size_t)bytes, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return -1;
  return bytes;
}
// debug: copy one of the model's device buffers to the host (0 recs, 1 clip, 2 attr, 3 nn_in, 4 poses); returns bytes copied
long long fpt_read_buffer(fp_model *m, int which, void *dst, long long max_bytes) {
  size_t V = m->targets.empty() ? 0 : (size_t)m->targets[0].mesh.V;
  const void *src[5] = {m->recs, m->clip, m->attr, m->nn_in, m->poses_dev};
  size_t n[5] = {(size_t)m->cap * sizeof(PoseRec), (size_t)m->cap * V * 16, (size_t)m->cap * V * 16,
                 (size_t)2 * m->cap * FP_NN_IN_IMG_HALFS * 2, (size_t)m->cap * 64};
  if (which < 0 || which > 4 || !src[which]) return -1;
  size_t b = std::min<size_t>(n[which], (size_t)max_bytes);
  if (hipMemcpyAsync(dst, src[which], b, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return -1;
  return (long long)b;
}

// the fused depth filter (depth_filter_rect_kernel) on [x0, x1) x [y0, y1) of the uploaded frame -> out_host, the rectangle's D' row by
// row ((y1 - y0) * (x1 - x0) floats; the rectangle is clamped to the frame first).  The kernel writes into `erode`, which is filled with
// NaN before: a pixel of the rectangle it did not write comes back as NaN.  The model's frame record is put back afterwards.
int fpt_depth_filter_rect(fp_model *m, int x0, int y0, int x1, int y1, float *out_host) try {
  FP_CHECK(m && out_host && m->depth && !m->frame_partial, "[FoundationPose] fpt_depth_filter_rect: no whole frame uploaded");
  SerialGuard serial(m->device);
  x0 = std::max(x0, 0); y0 = std::max(y0, 0); x1 = std::min(x1, m->W); y1 = std::min(y1, m->H);
  FP_CHECK(x1 > x0 && y1 > y0, "[FoundationPose] fpt_depth_filter_rect: empty rectangle");
  const FrameRef before = m->frame_pub;
  FrameRef r{};
  r.rgb = m->rgb; r.depth = m->erode; r.raw = m->depth;
  r.wx0 = x0; r.wy0 = y0; r.wx1 = x1; r.wy1 = y1; r.ux1 = m->W; r.uy1 = m->H;
  FP_HIP_OK(hipMemsetAsync(m->erode, 0xff, (size_t)m->H * m->W * 4, m->stream));
  if (publish_record(m, r)) return 1;
  launch_depth_filter_rect(m->stream, m->frame_dev, m->H, m->W);
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipMemcpy2DAsync(out_host, (size_t)(x1 - x0) * 4, m->erode + (size_t)y0 * m->W + x0, (size_t)m->W * 4, (size_t)(x1 - x0) * 4, (size_t)(y1 - y0),
                             hipMemcpyDeviceToHost, m->stream));
  if (before.rgb && publish_record(m, before)) return 1;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// the product's launch site launch_sampler on caller-given values (tests/test_pose_rules_gpu.py): vals_hw [H, W] f32 stands for the filtered
// depth, mask_hw [H, W] u8, K and min_depth are the caller's; N = 1 pose of the model's rotation grid.  The scan state is the MODEL's
// (m->samp_state, which a first fp_get_hyp_poses has allocated and every launch leaves reset), so a sequence of calls on one model
// runs the way a sequence of frames does.  center_out [3] = the translation written into the pose (quiet NaNs when the status is not
// 0: the kernel then writes none), *status_out = state[6], state_out [5] = state[0..4] after the call.  The compacted list `vals` the
// two kernels share lies between SAMPLER_RAW_GUARD canary words.  Returns 0, 1 on failure (fp_last_error), 2 when a canary word changed.
static constexpr size_t SAMPLER_RAW_GUARD = 1024;
int fpt_sampler_raw(fp_model *m, const float *vals_hw, const uint8_t *mask_hw, int H, int W, const float K[9], float min_depth,
                    float center_out[3], int *status_out, int state_out[5]) try {
  FP_CHECK(m && vals_hw && mask_hw && K && center_out && status_out && state_out, "[FoundationPose] fpt_sampler_raw: null argument");
  FP_CHECK(H >= 1 && W >= 1 && (long long)H * W <= (1 << 24), "[FoundationPose] fpt_sampler_raw: invalid frame size");
  FP_CHECK(m->samp_state && m->grid_dev, "[FoundationPose] fpt_sampler_raw: call fp_get_hyp_poses once first (it allocates the scan state)");
  SerialGuard serial(m->device);
  const size_t px = (size_t)H * W, G = SAMPLER_RAW_GUARD;
  const uint32_t canary = 0xA5C3F00Du;
  struct Bufs {
    float *depth = nullptr, *pose = nullptr;
    uint32_t *vals = nullptr;
    uint8_t *mask = nullptr;
    ~Bufs() { dev_free(depth); dev_free(pose); dev_free(vals); dev_free(mask); }
  } b;
  if (dev_alloc(&b.depth, px) || dev_alloc(&b.mask, px) || dev_alloc(&b.vals, px + 2 * G) || dev_alloc(&b.pose, 16)) return 1;
  std::vector<uint32_t> hv(px + 2 * G, canary);
  const std::vector<uint32_t> qnan(16, 0x7FC00000u);
  FP_HIP_OK(fp::memcpy_sync(b.depth, vals_hw, px * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(b.mask, mask_hw, px, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(b.vals, hv.data(), hv.size() * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(b.pose, qnan.data(), qnan.size() * 4, hipMemcpyHostToDevice));
  {   // the scan appends at state[4]: a count that is not zero on entry would carry the list past its guard words, so nothing is launched then
    int before[8];
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    FP_HIP_OK(fp::memcpy_sync(before, m->samp_state, sizeof(before), hipMemcpyDeviceToHost));
    FP_CHECK(before[0] == 0x7fffffff && before[1] == -1 && before[2] == 0x7fffffff && before[3] == -1 && before[4] == 0,
             "[FoundationPose] fpt_sampler_raw: the scan state is not the reset state on entry");
  }
  launch_sampler(m->stream, b.depth, b.mask, H, W, min_depth, K, m->grid_dev, 0, 1, m->samp_state, reinterpret_cast<float *>(b.vals + G), b.pose);
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  float pose[16];
  int state[8];
  FP_HIP_OK(fp::memcpy_sync(pose, b.pose, sizeof(pose), hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(state, m->samp_state, sizeof(state), hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(hv.data(), b.vals, hv.size() * 4, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) center_out[k] = pose[12 + k];
  *status_out = state[6];
  for (int k = 0; k < 5; k++) state_out[k] = state[k];
  for (size_t i = 0; i < G; i++)
    if (hv[i] != canary || hv[G + px + i] != canary) { fp::set_error("[FoundationPose] fpt_sampler_raw: the kernels wrote outside the value list"); return 2; }
  return 0;
} FP_CATCH_INT

#endif  // FP_TEST_HOOKS

const char *fp_last_error(void) { return g_last_error.c_str(); }

// Host phase of loading the networks of a precision that are not in memory yet (file I/O + five weight re-layouts per layer: 0.3-1 s)
// -- runs BEFORE the caller takes the exclusive lifetime lock, so other models keep serving meanwhile; adopt() (under the lock) does
// the device phase (one allocation + upload per network) and hands them to the model.
struct PreparedNets {
  Net *r = nullptr, *s = nullptr;
  int prec = -1;
  PreparedNets() = default;
  PreparedNets(const PreparedNets &) = delete;
  PreparedNets &operator=(const PreparedNets &) = delete;
  ~PreparedNets() { if (r) net_free(r); if (s) net_free(s); }
  int prepare(const std::string &refiner_path, bool have_r, const std::string &scorer_path, bool have_s, int precision) {
    prec = precision;
    std::string err;
    if (!refiner_path.empty() && !have_r) {
      r = net_prepare(refiner_path.c_str(), false, precision, &err);
      FP_CHECK(r != nullptr, "[FoundationPose] Failed to load refiner weights: " + err);
    }
    if (!scorer_path.empty() && !have_s) {
      s = net_prepare(scorer_path.c_str(), true, precision, &err);
      FP_CHECK(s != nullptr, "[FoundationPose] Failed to load scorer weights: " + err);
    }
    return 0;
  }
  int adopt(fp_model *m) {
    std::string err;
    if (r && !m->refiner_p[prec]) {
      FP_CHECK(net_commit(r, &err) == 0, "[FoundationPose] Failed to load refiner weights: " + err);
      m->refiner_p[prec] = r; r = nullptr;
    }
    if (s && !m->scorer_p[prec]) {
      FP_CHECK(net_commit(s, &err) == 0, "[FoundationPose] Failed to load scorer weights: " + err);
      m->scorer_p[prec] = s; s = nullptr;
    }
    return 0;
  }
};

// networks of precision `prec` (loaded on first use) become the model's current ones
static int select_precision(fp_model *m, int prec) {
  FP_CHECK(prec == PREC_F16 || prec == PREC_BF16 || prec == PREC_FP8 || prec == PREC_INT8, "[FoundationPose] unknown precision");
  std::string err;
  if (!m->refiner_path.empty() && !m->refiner_p[prec]) {
    m->refiner_p[prec] = net_load(m->refiner_path.c_str(), false, prec, &err);
    FP_CHECK(m->refiner_p[prec] != nullptr, "[FoundationPose] Failed to load refiner weights: " + err);
  }
  if (!m->scorer_path.empty() && !m->scorer_p[prec]) {
    m->scorer_p[prec] = net_load(m->scorer_path.c_str(), true, prec, &err);
    FP_CHECK(m->scorer_p[prec] != nullptr, "[FoundationPose] Failed to load scorer weights: " + err);
  }
  if ((prec == PREC_FP8 || prec == PREC_INT8) && m->calibrated(prec)) {
    Net *nets[2] = {m->refiner_p[prec], m->scorer_p[prec]};
    const CalibRecord &r = m->calib[prec];
    for (int k = 0; k < 2; k++)
      if (nets[k] && !net_q8_ready(nets[k]) &&
          net_apply_q8(nets[k], r.amax[k].data(), r.bias_fix[k].empty() ? nullptr : r.bias_fix[k].data(),
                       r.tok_fix[k].empty() ? nullptr : r.tok_fix[k].data(), true, r.slots ? r.fmeans[k].data() : nullptr, r.slots))
        return 1;
    for (int k = 0; k < 2; k++)
      if (nets[k] && !r.out_fix[k].empty() && net_q8_set_out_fix(nets[k], r.out_fix[k].data())) return 1;
  }
  if (!m->ws_p[prec]) m->ws_p[prec] = nn_scratch_create(prec);
  m->prec = prec;
  m->refiner = m->refiner_p[prec];
  m->scorer = m->scorer_p[prec];
  m->ws = m->ws_p[prec];
  return 0;
}
// element type of the networks' input tensor in the current precision
static OutMode nn_mode(const fp_model *m) {
  const Net *n = m->refiner ? m->refiner : m->scorer;
  return n && net_input_dt(n) == DT_BF16 ? OUT_BF16X8 : OUT_F16X8;
}

// ---- pose fit ----
// buffers of the pose fit, allocated at the first use of the option (sized for the largest batch: 76 KB + 152 KB + 2 KB pinned)
static int ensure_fit(fp_model *m) {
  if (m->fit_acc && m->fit_rec && m->fit_io) return 0;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  if (!m->fit_acc) {
    if (dev_alloc(&m->fit_acc, (size_t)FP_MAX_BATCH * 4)) return 1;
    FP_HIP_OK(hipMemsetAsync(m->fit_acc, 0, (size_t)FP_MAX_BATCH * 4 * sizeof(unsigned long long), m->stream));   // once: the kernel leaves them zeroed
  }
  if (!m->fit_rec && dev_alloc(&m->fit_rec, (size_t)2 * FP_MAX_BATCH)) return 1;
  if (!m->fit_io) FP_HIP_OK(pinned_mapped_alloc(&m->fit_io, &m->fit_io_dev, 65 * sizeof(PoseFitRec), hipHostMallocCoherent));
  g_alloc_epoch++;
  return 0;
}
static float fit_tol_n(float tol_m, float diameter) { return tol_m / (diameter / 2); }   // formed once, in f32
static void fit_record(fp_pose_fit *o, const PoseFitRec &r, float tol_n, float diameter) {
  o->n_model = r.n_model; o->n_observed = r.n_observed; o->n_inlier = r.n_inlier; o->n_front = r.n_front; o->n_behind = r.n_behind;
  o->reserved = 0;
  o->sum_dz_q20 = r.sum_dz_q20;
  o->mean_dz_m = r.n_inlier ? (float)((double)r.sum_dz_q20 / 1048576.0 / (double)r.n_inlier * (double)(diameter / 2)) : 0.0f;
  o->tol_n = tol_n;
}
// the kernel over N hypotheses whose rendered images start at `a` and observed images at `b`, one image apart each
static int enqueue_pose_fit(fp_model *m, const __half *a, const __half *b, int N, const PoseFitTol &tol, PoseFitRec *out) {
  ProfScope ps(&m->prof, m->stream, "pose_fit", 0, (double)N * 2 * FP_CROP_HW * FP_CROP_HW * 16);
  launch_pose_fit(m->stream, a, FP_NN_IN_IMG_HALFS, b, FP_NN_IN_IMG_HALFS, N, tol, nn_mode(m), m->fit_acc, out);
  FP_HIP_OK(hipGetLastError());
  return 0;
}
static PoseFitTol fit_tol_uniform(float tol_n) {
  PoseFitTol t = {};
  t.v[0] = tol_n; t.uniform = 1;
  return t;
}

static void destroy_model_impl(fp_model *m);
fp_model *fp_create_on(int device, const fp_mesh *meshes, int n_meshes, const float K[9], const char *refiner_weights,
                       const char *scorer_weights, int max_h, int max_w) try {
  if (!meshes || n_meshes <= 0 || !K) { set_error("[FoundationPose] fp_create: invalid arguments"); return nullptr; }
  // host phase first, WITHOUT the lock [r5]: reading both weight files and building every kernel layout is most of a creation's time
  PreparedNets nets;
  if (nets.prepare(refiner_weights ? refiner_weights : "", false, scorer_weights ? scorer_weights : "", false, PREC_F16)) return nullptr;
  LifeExclusive life;   // device phase: not while another thread is inside a call (see SerialGuard)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("[FoundationPose] no HIP device available (this library has no CPU path)");
    return nullptr;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { set_error("[FoundationPose] hipGetDevice failed"); return nullptr; }   // -1: the caller's current device
  if (device >= ndev) { set_error("[FoundationPose] fp_create_on: no such device"); return nullptr; }
  DeviceScope on_device(device);
  std::unique_ptr<fp_model, void (*)(fp_model *)> m(new fp_model(), destroy_model_impl);  // a failed construction releases what it had allocated
  m->device = device;
  std::memcpy(m->K, K, sizeof(float) * 9);
  if (max_h > 0) m->max_h = max_h;
  if (max_w > 0) m->max_w = max_w;
  // non-blocking: no implicit synchronisation with the legacy null stream (other models' threads, the caller's framework)
  if (stream_acquire(&m->stream) != hipSuccess) { set_error("[FoundationPose] Failed to create stream"); return nullptr; }
  // the frame record's device block [FrameRef, padded to 64 bytes | packed window]: the window part and its pinned twin are allocated
  // on the first host-frame Track that needs them and grown on demand (ensure_window) [r5] -- a model that is only ever handed device
  // frames, or never tracks, pins no host memory
  if (hipMalloc((void **)&m->frame_dev, 64) != hipSuccess ||
      pinned_mapped_alloc(&m->frame_pinned, &m->frame_pinned_dev, 8 * 64, hipHostMallocMapped) != hipSuccess) {
    set_error("[FoundationPose] Failed to allocate the frame record");
    return nullptr;
  }
  for (int i = 0; i < n_meshes; i++) {
    const fp_mesh &src = meshes[i];
    if (!src.vertices || !src.normals || !src.texcoords || !src.faces || !src.texture || src.num_vertices <= 0 ||
        src.num_faces <= 0 || src.tex_height <= 0 || src.tex_width <= 0) {
      set_error("[FoundationPose Renderer] Failed to load textured mesh!!!");
      destroy_model_impl(m.release());
      return nullptr;
    }
    Target t;
    t.name = src.name ? src.name : "";
    DeviceMesh &d = t.mesh;
    d.V = src.num_vertices; d.F = src.num_faces; d.TH = src.tex_height; d.TW = src.tex_width;
    d.diameter = src.diameter;
    std::memcpy(d.center, src.center, sizeof(float) * 3);
    // LoadTexturedMesh (D6F/src/foundationpose_render.cpp:381-509): centre vertices, flip v
    std::vector<float> v((size_t)d.V * 3), uv((size_t)d.V * 2);
    for (int k = 0; k < d.V; k++) {
      for (int c = 0; c < 3; c++) v[(size_t)k * 3 + c] = src.vertices[(size_t)k * 3 + c] - src.center[c];
      uv[(size_t)k * 2] = src.texcoords[(size_t)k * 2];
      uv[(size_t)k * 2 + 1] = 1 - src.texcoords[(size_t)k * 2 + 1];
    }
    double norm2 = 0;
    for (int k = 0; k < d.V; k++)
      norm2 = std::max(norm2, (double)v[(size_t)k * 3] * v[(size_t)k * 3] + (double)v[(size_t)k * 3 + 1] * v[(size_t)k * 3 + 1] + (double)v[(size_t)k * 3 + 2] * v[(size_t)k * 3 + 2]);
    d.max_norm = (float)(std::sqrt(norm2) * (1.0 + 1e-6));   // (rounded up: fp_render_pose's screen bound must contain every vertex)
    std::vector<int32_t> f((size_t)d.F * 3);
    for (size_t k = 0; k < f.size(); k++) f[k] = (int32_t)src.faces[k];
    // A face whose centred corners are exactly collinear has no surface, but the rasterisers cull on the area of the SNAPPED corners:
    // under most poses three collinear points snap to a sliver up to 1/16 px wide, which can cover a sample and win a depth tie against
    // the surface it lies in.  Such a face is stored as (i0, i0, i0): a repeated index snaps to one point under every pose, so every
    // rasteriser of the library culls it, and the numbering of the other faces stays.  The differences of two
    // f32 and the products of two such differences are exact in double, so the cross product is zero exactly when the corners are collinear.
    for (int k = 0; k < d.F; k++) {
      int32_t *i = &f[(size_t)k * 3];
      if ((uint32_t)i[0] >= (uint32_t)d.V || (uint32_t)i[1] >= (uint32_t)d.V || (uint32_t)i[2] >= (uint32_t)d.V) continue;
      const float *p0 = &v[(size_t)i[0] * 3], *p1 = &v[(size_t)i[1] * 3], *p2 = &v[(size_t)i[2] * 3];
      const double a[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
      const double b[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
      if (a[1] * b[2] == a[2] * b[1] && a[2] * b[0] == a[0] * b[2] && a[0] * b[1] == a[1] * b[0]) i[1] = i[2] = i[0];
    }
    bool ok = !dev_alloc(&d.verts, v.size()) && !dev_alloc(&d.normals, v.size()) && !dev_alloc(&d.uvs, uv.size()) &&
              !dev_alloc(&d.faces, f.size()) && !dev_alloc(&d.tex, (size_t)d.TH * d.TW * 3);
    ok = ok && fp::memcpy_sync(d.verts, v.data(), v.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && fp::memcpy_sync(d.normals, src.normals, v.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && fp::memcpy_sync(d.uvs, uv.data(), uv.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && fp::memcpy_sync(d.faces, f.data(), f.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && fp::memcpy_sync(d.tex, src.texture, (size_t)d.TH * d.TW * 3, hipMemcpyHostToDevice) == hipSuccess;
    m->targets.push_back(t);
    m->max_faces = std::max(m->max_faces, (size_t)t.mesh.F);
    if (!ok) {
      set_error("[FoundationPose Renderer] Failed to prepare buffer!!!");
      destroy_model_impl(m.release());
      return nullptr;
    }
  }
  if (set_rotation_grid(m.get(), m->inplane_steps)) { destroy_model_impl(m.release()); return nullptr; }
  if (refiner_weights) m->refiner_path = refiner_weights;
  if (scorer_weights) m->scorer_path = scorer_weights;
  if (nets.adopt(m.get()) || select_precision(m.get(), PREC_F16)) { destroy_model_impl(m.release()); return nullptr; }
  if (hipMalloc((void **)&m->argmax_dev, sizeof(int)) != hipSuccess) { destroy_model_impl(m.release()); return nullptr; }
  return m.release();
} FP_CATCH_PTR

fp_model *fp_create(const fp_mesh *meshes, int n_meshes, const float K[9], const char *refiner_weights,
                    const char *scorer_weights, int max_h, int max_w) try {
  return fp_create_on(-1, meshes, n_meshes, K, refiner_weights, scorer_weights, max_h, max_w);
} FP_CATCH_PTR
int fp_device(const fp_model *m) { return m ? m->device : -1; }

static void destroy_model_impl(fp_model *m) {
  if (!m) return;
  DeviceScope on_device(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  invalidate_graphs(m);
  if (m->multi_io) (void)hipHostFree(m->multi_io);
  m->prof.reset();
  for (auto &t : m->targets) {
    dev_free(t.mesh.verts); dev_free(t.mesh.normals); dev_free(t.mesh.uvs); dev_free(t.mesh.faces); dev_free(t.mesh.tex);
    dev_free(t.mesh.vcol);
  }
  dev_free(m->rgb_own); dev_free(m->depth_own); dev_free(m->erode); dev_free(m->bilat); dev_free(m->xyz);
  dev_free(m->recs); dev_free(m->poses_dev); dev_free(m->clip); dev_free(m->attr); dev_free(m->tri_rows); dev_free(m->nn_in);
  dev_free(m->blob_a); dev_free(m->blob_b); dev_free(m->trans_dev); dev_free(m->rot_dev); dev_free(m->scores_dev);
  dev_free(m->feat_dev); dev_free(m->argmax_dev); dev_free(m->scores_all); dev_free(m->best_pose_dev);
  dev_free(m->gath_feat); dev_free(m->gath_poses); dev_free(m->shard_send); dev_free(m->shard_recv);
  if (m->result_pinned) (void)hipHostFree(m->result_pinned); dev_free(m->dbg_tri); dev_free(m->dbg_rast);
  if (m->poses_pinned) (void)hipHostFree(m->poses_pinned);
  if (m->track_io) (void)hipHostFree(m->track_io);
  if (m->frame_pinned) (void)hipHostFree(m->frame_pinned);
  if (m->win_stage) (void)hipHostFree(m->win_stage);
  if (m->host_stage) (void)hipHostFree(m->host_stage);
  if (m->host_stage_done) (void)hipEventDestroy(m->host_stage_done);
  if (m->frame_dev) (void)hipFree(m->frame_dev);
  dev_free(m->grid_dev); dev_free(m->samp_state); dev_free(m->samp_vals); dev_free(m->mask_dev);
  if (m->digests) (void)hipFree(m->digests);
  dev_free(m->fit_acc); dev_free(m->fit_rec);
  dev_free(m->st_snap); dev_free(m->st_cam); dev_free(m->st_poses); dev_free(m->st_items);
  dev_free(m->fr_flag); dev_free(m->fr_out);
  dev_free(m->sc_table); dev_free(m->sc_work); dev_free(m->sc_list);
  delete m->sc_table_host; m->sc_table_host = nullptr;
  dev_free(m->pe_mats); dev_free(m->pe_pairs); dev_free(m->pe_sums);
  dev_free(m->ps_recs); dev_free(m->icp_params); dev_free(m->icp_acc); dev_free(m->vsd_words); dev_free(m->vsd_plane);
  dev_free(m->col_acc);
  dev_free(m->sil_mask); dev_free(m->sil_g); dev_free(m->sil_d2); dev_free(m->sil_acc);
  dev_free(m->silref_sd); dev_free(m->silref_params); dev_free(m->silref_acc);
  if (m->fit_io) (void)hipHostFree(m->fit_io);
  for (int i = 0; i < N_PREC; i++) {
    if (m->refiner_p[i]) net_free(m->refiner_p[i]);
    if (m->scorer_p[i]) net_free(m->scorer_p[i]);
    if (m->ws_p[i]) nn_scratch_free(m->ws_p[i]);
  }
  if (m->stream) { (void)hipStreamSynchronize(m->stream); stream_release(m->stream); }
  delete m;
}
void fp_destroy(fp_model *m) {
  LifeExclusive life;   // not while another thread is inside a call (see SerialGuard)
  destroy_model_impl(m);
}

static_assert(FP_RENDER_SNAP_MAX == fp::FRAME_RENDER_SNAP_MAX && FP_RENDER_NEAR_M == fp::FRAME_RENDER_NEAR,
              "include/foundationpose_amd.h: the refusal constants of fp_render_pose are those of fp_internal.h");
static_assert(FP_MAX_BATCH == fp::MAX_BATCH && 42 * FP_MAX_INPLANE_STEPS <= FP_MAX_BATCH && 42 * (FP_MAX_INPLANE_STEPS + 1) > FP_MAX_BATCH,
              "include/foundationpose_amd.h: the batch limit is fp_nn.h MAX_BATCH");
int fp_set_inplane_steps(fp_model *m, int steps) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && steps >= 1, "[FoundationPose] fp_set_inplane_steps: invalid arguments");
  FP_CHECK(steps <= FP_MAX_INPLANE_STEPS, "[FoundationPose] fp_set_inplane_steps: " + std::to_string(steps) + " steps = " + std::to_string(42 * steps) +
           " hypotheses, above the batch limit FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH) + " (at most " + std::to_string(FP_MAX_INPLANE_STEPS) + " steps)");
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return set_rotation_grid(m, steps);
} FP_CATCH_INT
int fp_num_hypotheses(const fp_model *m) { return m ? m->n_hyp() : 0; }
void *fp_stream(fp_model *m) { return m ? (void *)m->stream : nullptr; }
int fp_synchronize(fp_model *m) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m, "null model");
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// asynchronous: the caller of this helper synchronises m->stream before the host frame can go away
// row0 / row1 (host frames): only rows [row0, row1) are needed by the caller (Track: the observed-crop window) -- the rest of the
// model's copy keeps whatever an earlier frame left there
// [r6] host -> device on a SERVING path without a copy command: the bytes are packed into the model's pinned, device-mapped block at
// `stage_off` and a kernel fetches them (staged_upload_kernel; dst must be 16-byte aligned).  The block is rewritten only after the fetches of
// the previous call have run (host_stage_done), so the asynchronous shard entry points may return before the GPU has read it; the caller's
// buffer is free on return.
static int ensure_host_stage(fp_model *m, size_t bytes) {
  if (m->host_stage_pending) {   // the last call's fetch kernels have read the block
    FP_HIP_OK(hipEventSynchronize(m->host_stage_done));
    m->host_stage_pending = false;
  }
  if (bytes <= m->host_stage_cap) return 0;
  const size_t cap = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  uint8_t *stage = nullptr, *stage_dev = nullptr;
  if (pinned_mapped_alloc(&stage, &stage_dev, cap, hipHostMallocMapped) != hipSuccess) { set_error("[FoundationPose] out of pinned, device-mapped host memory for the frame"); return 1; }
  if (m->host_stage) (void)hipHostFree(m->host_stage);
  m->host_stage = stage; m->host_stage_dev = stage_dev; m->host_stage_cap = cap;
  if (!m->host_stage_done) FP_HIP_OK(hipEventCreateWithFlags(&m->host_stage_done, hipEventDisableTiming));
  return 0;
}
static int stage_fetch(fp_model *m, void *dst_dev, const void *src_host, size_t bytes, size_t stage_off) {
  FP_CHECK(stage_off % 16 == 0 && stage_off + bytes <= m->host_stage_cap && ((uintptr_t)dst_dev & 15) == 0, "[FoundationPose] internal: misaligned staged upload");
  std::memcpy(m->host_stage + stage_off, src_host, bytes);
  const unsigned blocks = (unsigned)std::min<size_t>(1024, (bytes / 16 + 255) / 256 + 1);
  FP_GEOM_LOG("staged_upload");
  hipLaunchKernelGGL(fp::staged_upload_kernel, dim3(blocks), dim3(256), 0, m->stream, m->host_stage_dev + stage_off, (unsigned char *)dst_dev, bytes);
  FP_HIP_OK(hipGetLastError());
  return 0;
}
static int stage_fetch_done(fp_model *m) {
  FP_HIP_OK(hipEventRecord(m->host_stage_done, m->stream));
  m->host_stage_pending = true;
  return 0;
}
static size_t stage_mask_offset(size_t px) { return ((px * 3 + 63) & ~(size_t)63) + ((px * 4 + 63) & ~(size_t)63); }   // [rgb | depth | mask]

// room for a packed window of `total` bytes in the model's pinned block and its device twin (both hold the frame record in front)
static int ensure_window(fp_model *m, size_t total) {
  if (total <= m->win_cap) return 0;
  const size_t limit = (64 + (size_t)m->max_h * m->max_w * 7 / 2 + 256 + 15) & ~(size_t)15;   // a window that takes this path is at most half the frame wide
  size_t cap = std::min(limit, std::max<size_t>(total + total / 2, (size_t)256 << 10));
  cap = (cap + 15) & ~(size_t)15;   // whole 16-byte units for window_fetch_kernel
  if (total > cap) return 1;        // (larger than any window of this model's frame limits: the caller falls back to the 2-D copies)
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  uint8_t *stage = nullptr, *stage_dev = nullptr;
  FrameRef *block = nullptr;
  if (pinned_mapped_alloc(&stage, &stage_dev, cap, hipHostMallocCoherent) != hipSuccess) { set_error("[FoundationPose] out of pinned host memory for the Track window"); return 1; }
  if (hipMalloc((void **)&block, cap) != hipSuccess) {
    (void)hipHostFree(stage);
    set_error("[FoundationPose] out of device memory for the Track window");
    return 1;
  }
  if (m->win_stage) (void)hipHostFree(m->win_stage);
  if (m->frame_dev) (void)hipFree(m->frame_dev);
  m->win_stage = stage; m->win_stage_dev = stage_dev; m->frame_dev = block; m->win_cap = cap;
  m->frame_pub = FrameRef{};   // the new block holds no record yet
  g_alloc_epoch++;             // captured graphs read the frame through the old block's address
  return 0;
}

// the frame record of the model's current frame read whole: with the depth filter on the crops read `bilat`, which the caller fills
static FrameRef whole_frame_record(const fp_model *m) {
  FrameRef r{};   // no pitch, no window
  r.rgb = m->rgb; r.depth = m->depth;
  if (m->dfilt_on) { r.depth = m->bilat; r.raw = m->depth; r.ux1 = m->W; r.uy1 = m->H; }
  return r;
}
// makes `want` the record the kernels read, unless it is already
static int publish_record(fp_model *m, const FrameRef &want) {
  if (same_record(m->frame_pub, want)) return 0;
  // (a ring of pinned records: the asynchronous shard entry points return before the copy has run)
  const unsigned k = m->frame_pub_count++ & 7;
  FrameRef *slot = reinterpret_cast<FrameRef *>(m->frame_pinned + 64 * k);
  *slot = want;
  launch_window_fetch(m->stream, m->frame_pinned_dev + 64 * k, m->frame_dev, 64);   // [r6] 64 bytes by a kernel, not a copy command
  FP_HIP_OK(hipGetLastError());
  m->frame_pub = want;
  return 0;
}

// filt (depth filter on, Track): the rectangle of the frame the call's depth_filter_rect launch fills and the crops may read; the rows /
// columns uploaded hold every pixel within the filter's reach of it.  Null: the whole frame.
static int upload_frame_async(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, int row0, int row1, int col0, int col1,
                              const TrackWindow *filt) {
  Target *t = nullptr;
  if (check_frame_args(m, H, W, nullptr, &t)) return 1;
  FP_CHECK(rgb && depth, "[FoundationPose] Got INVALID rgb/depth ptr");
  size_t px = (size_t)H * W;
  if (px > m->frame_cap) {
    g_alloc_epoch++;
    dev_free(m->rgb_own); dev_free(m->depth_own); dev_free(m->erode); dev_free(m->bilat); dev_free(m->xyz);
    if (dev_alloc(&m->rgb_own, px * 3) || dev_alloc(&m->depth_own, px) || dev_alloc(&m->erode, px) ||
        dev_alloc(&m->bilat, px))
      return 1;
    m->frame_cap = px;
  }
  m->H = H; m->W = W;
  m->host_stage_fresh = false;
  if (memspace == FP_DEVICE) {
    m->rgb = (const uint8_t *)rgb;
    m->depth = (const float *)depth;
    m->frame_partial = false;
    row0 = 0; row1 = H; col0 = 0; col1 = W;
  } else {
    if (row1 < 0 || row1 > H) row1 = H;
    row0 = std::max(0, std::min(row0, row1));
    m->frame_partial = row0 > 0 || row1 < H;
    if (col1 < 0 || col1 > W) col1 = W;
    col0 = std::max(0, std::min(col0, col1));
    const size_t o = (size_t)row0 * W, n = (size_t)(row1 - row0) * W;
    const size_t cw = (size_t)(col1 - col0);
    ProfScope ps(&m->prof, m->stream, "h2d_frame", 0, (double)(row1 - row0) * cw * 7);
    if (n && cw && cw * 2 <= (size_t)W) {
      // the window is less than half the frame wide: only its rectangle is uploaded
      m->frame_partial = true;
      const size_t oc = o + col0, nr = (size_t)(row1 - row0);
      const size_t rgb_bytes = (nr * cw * 3 + 63) & ~(size_t)63, total = 64 + rgb_bytes + nr * cw * 4;
      if (ensure_window(m, total) == 0) {
        // [r4] The caller's frame is pageable: a 2-D copy from it is staged inside the runtime and holds the calling thread until it
        // is done (two of them: ~48 us of a 260 us Track).  The window is packed here into the model's own pinned block instead (a
        // few hundred short memcpys, ~0.1 MB) TOGETHER with the frame record that describes it, and a small kernel fetches the block
        // over PCIe (window_fetch_kernel: ~6 us before the graph behind it can start; a copy command of this size ~27 us, 2-D copies
        // from pinned memory 1.07 ms per Track: both retired, EXPERIMENTS.md); crop_body reads the packed window through the record's
        // pitch and virtual origins.  The caller's buffers are free again when this function returns.  The pinned block is reused by
        // the next call: a model's Track is waited for (fp_track_wait) before its next submission.
        uint8_t *dev_block = reinterpret_cast<uint8_t *>(m->frame_dev);
        uint8_t *sr = m->win_stage + 64;
        float *sd = reinterpret_cast<float *>(m->win_stage + 64 + rgb_bytes);
        const uint8_t *ur = (const uint8_t *)rgb + oc * 3;
        const float *ud = (const float *)depth + oc;
        for (size_t r = 0; r < nr; r++) {
          std::memcpy(sr + r * cw * 3, ur + r * (size_t)W * 3, cw * 3);
          std::memcpy(sd + r * cw, ud + r * (size_t)W, cw * 4);
        }
        FrameRef rec;
        const long long org = (long long)row0 * (long long)cw + col0;   // packed index of frame pixel (0, 0)
        // (virtual origins lie outside the block: formed as integers, only ever dereferenced inside the window)
        rec.rgb = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(dev_block) + 64 - (uintptr_t)(org * 3));
        rec.depth = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(dev_block) + 64 + rgb_bytes - (uintptr_t)(org * 4));
        rec.pitch = (int)cw;
        rec.wx0 = col0; rec.wx1 = col1; rec.wy0 = row0; rec.wy1 = row1;
        if (m->dfilt_on) {
          // the packed depth is the filter's input; its output goes to `bilat` under the same pitch and virtual origin, and the crops
          // read that inside the filtered rectangle alone
          rec.raw = rec.depth;
          rec.ux0 = col0; rec.ux1 = col1; rec.uy0 = row0; rec.uy1 = row1;
          rec.depth = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(m->bilat) - (uintptr_t)(org * 4));
          if (filt) { rec.wx0 = filt->col0; rec.wx1 = filt->col1; rec.wy0 = filt->row0; rec.wy1 = filt->row1; }
        }
        std::memcpy(m->win_stage, &rec, sizeof(rec));
        launch_window_fetch(m->stream, m->win_stage_dev, dev_block, total);
        FP_HIP_OK(hipGetLastError());
        m->frame_pub = rec;
        m->rgb = m->rgb_own; m->depth = m->depth_own;   // (hold nothing of this frame: frame_partial)
        return 0;
      }
      // the model cannot hold this window (ensure_window): two 2-D copies of the rectangle at the device frame's own pitch
      FP_HIP_OK(hipMemcpy2DAsync(m->rgb_own + oc * 3, (size_t)W * 3, (const uint8_t *)rgb + oc * 3, (size_t)W * 3, cw * 3, nr,
                                 hipMemcpyHostToDevice, m->stream));
      FP_HIP_OK(hipMemcpy2DAsync(m->depth_own + oc, (size_t)W * 4, (const float *)depth + oc, (size_t)W * 4, cw * 4, nr,
                                 hipMemcpyHostToDevice, m->stream));
    } else if (n) {
      // [r6] whole rows [row0', row1) through the pinned block + a fetch kernel (row0 rounded down so that both device offsets are
      // 16-byte aligned: row0' * W % 16 == 0)
      int ra = row0;
      while (ra > 0 && ((size_t)ra * W) % 16 != 0) ra--;
      const size_t oa = (size_t)ra * W, na = (size_t)(row1 - ra) * W;
      if (ensure_host_stage(m, stage_mask_offset(px) + px)) return 1;
      if (stage_fetch(m, m->rgb_own + oa * 3, (const uint8_t *)rgb + oa * 3, na * 3, 0)) return 1;
      if (stage_fetch(m, m->depth_own + oa, (const float *)depth + oa, na * 4, (px * 3 + 63) & ~(size_t)63)) return 1;
      if (stage_fetch_done(m)) return 1;
      m->host_stage_fresh = true;
    }
    m->rgb = m->rgb_own;
    m->depth = m->depth_own;
  }
  FrameRef want = whole_frame_record(m);
  if (m->dfilt_on) {
    // the unfiltered depth exists where this call put it (a device frame: everywhere)
    want.ux0 = col0; want.ux1 = col1; want.uy0 = row0; want.uy1 = row1;
    if (filt) { want.wx0 = filt->col0; want.wx1 = filt->col1; want.wy0 = filt->row0; want.wy1 = filt->row1; }
  }
  return publish_record(m, want);
}

// stage operators on the uploaded frame: with the depth filter on they read D' of the whole frame (the last call may have been a Track,
// which fills its window of `bilat` alone, or the option may have been switched since the upload)
static int run_depth_filters(fp_model *m);
static int stage_frame(fp_model *m) {
  if (m->dfilt_on && run_depth_filters(m)) return 1;
  return publish_record(m, whole_frame_record(m));
}

int fp_upload_frame(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W) try {
  SerialGuard serial(m ? m->device : -1);
  if (upload_frame_async(m, rgb, depth, memspace, H, W)) return 1;
  if (memspace == FP_HOST) FP_HIP_OK(hipStreamSynchronize(m->stream));  // the host frame may be released on return
  return 0;
} FP_CATCH_INT

int fp_get_xyz_map(fp_model *m, float *xyz_host) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && m->depth && xyz_host, "[FoundationPose] fp_get_xyz_map: no frame uploaded");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  size_t px = (size_t)m->H * m->W;
  if (!m->xyz && dev_alloc(&m->xyz, m->frame_cap * 3)) return 1;
  if (m->dfilt_on && run_depth_filters(m)) return 1;   // the map of D': what the networks see
  launch_depth_to_xyz(m->stream, m->dfilt_on ? m->bilat : m->depth, m->H, m->W, m->K, m->xyz);
  FP_HIP_OK(hipMemcpyAsync(xyz_host, m->xyz, px * 12, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

static int run_depth_filters(fp_model *m) {
  {
    ProfScope ps(&m->prof, m->stream, "erode_depth", 0, (double)m->H * m->W * 8);
    launch_erode(m->stream, m->depth, m->erode, m->H, m->W);
  }
  {
    ProfScope ps(&m->prof, m->stream, "bilateral_depth", 0, (double)m->H * m->W * 8);
    launch_bilateral(m->stream, m->erode, m->bilat, m->H, m->W);
  }
  return 0;
}

int fp_filter_depth(fp_model *m, float *eroded_out, float *bilateral_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && m->depth, "[FoundationPose] fp_filter_depth: no frame uploaded");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  size_t px = (size_t)m->H * m->W;
  run_depth_filters(m);
  if (eroded_out) FP_HIP_OK(hipMemcpyAsync(eroded_out, m->erode, px * 4, hipMemcpyDeviceToHost, m->stream));
  if (bilateral_out) FP_HIP_OK(hipMemcpyAsync(bilateral_out, m->bilat, px * 4, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// MakeRotationGrid result, host + device copies (device: the sampler kernel stamps the translation into it)
static int set_rotation_grid(fp_model *m, int steps) {
  m->inplane_steps = steps;
  m->grid_host = make_rotation_grid(40, steps);
  g_alloc_epoch++;
  dev_free(m->grid_dev);
  if (dev_alloc(&m->grid_dev, m->grid_host.size())) return 1;
  FP_HIP_OK(fp::memcpy_sync(m->grid_dev, m->grid_host.data(), m->grid_host.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// GetHypPoses (D6F/src/foundationpose_sampling.cpp:344-394), entirely on the device: erode + bilateral, then
// GuessTranslation (bounding box of the mask, exact median of the filtered depth under it) and the hypothesis poses
// [first, first+N) of the rotation grid written to m->poses_dev.  No read-back, no synchronisation: the status word
// (sampler_status) is fetched together with the results.
static int sample_hypotheses_async(fp_model *m, Target *t, const void *mask, int memspace, int first, int N) {
  FP_CHECK(m->depth != nullptr && mask != nullptr, "[FoudationPoseSampler] Got INVALID depth/mask ptr on device!!!");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  const size_t px = (size_t)m->H * m->W;
  if (ensure_capacity(m, N, t ? (size_t)t->mesh.V : 0)) return 1;
  if (px > m->samp_px_cap) {
    g_alloc_epoch++;
    dev_free(m->samp_vals); dev_free(m->mask_dev);
    m->samp_px_cap = 0;
    if (dev_alloc(&m->samp_vals, px) || dev_alloc(&m->mask_dev, px)) return 1;
    m->samp_px_cap = px;
  }
  if (!m->samp_state) {
    if (dev_alloc(&m->samp_state, 8)) return 1;
    const int init[8] = {0x7fffffff, -1, 0x7fffffff, -1, 0, 0, 3, 0};
    FP_HIP_OK(fp::memcpy_sync(m->samp_state, init, sizeof(init), hipMemcpyHostToDevice));
    g_alloc_epoch++;
  }
  run_depth_filters(m);
  const uint8_t *mask_d = (const uint8_t *)mask;
  if (memspace != FP_DEVICE) {  // the caller's host mask stays valid until the entry point returns (it synchronises)
    // [r6] through the pinned block (behind the frame's rgb | depth, which a host-frame call has just staged; a host mask over a DEVICE
    // frame finds the block free or waits for its last use)
    if (!m->host_stage_fresh && ensure_host_stage(m, stage_mask_offset(px) + px)) return 1;   // (fresh: this call's frame upload sized the block and waited for its last use)
    m->host_stage_fresh = false;
    if (stage_fetch(m, m->mask_dev, mask, px, stage_mask_offset(px))) return 1;
    if (stage_fetch_done(m)) return 1;
    mask_d = m->mask_dev;
  }
  ProfScope ps(&m->prof, m->stream, "sampler", 0, (double)px * 5);
  launch_sampler(m->stream, m->bilat, mask_d, m->H, m->W, FP_MIN_DEPTH, m->K, m->grid_dev, first, N, m->samp_state, m->samp_vals,
                 m->poses_dev);
  return 0;
}

// the sampler's status word as the reference's failure modes (foundationpose_sampling.cpp:269,278); null: the poses are valid.
// sampler_status fetches the word and synchronises.
static const char *sampler_verdict(int st) {
  return st == 0 ? nullptr : st == 1 ? "[FoundationposeSampling] Mask is all zero."
       : st == 2 ? "[FoundationposeSampling] No valid value in mask." : "[FoundationposeSampling] sampler did not run";
}
static int sampler_status(fp_model *m) {
  int st = 3;
  FP_HIP_OK(hipMemcpyAsync(&st, m->samp_state + 6, 4, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  const char *why = sampler_verdict(st);
  FP_CHECK(!why, why);
  return 0;
}

int fp_get_hyp_poses(fp_model *m, const void *mask, int memspace, float *poses_out, int *n_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses_out, "[FoundationPose] fp_get_hyp_poses: invalid arguments");
  const int n = m->n_hyp();
  if (sample_hypotheses_async(m, m->targets.empty() ? nullptr : &m->targets[0], mask, memspace, 0, n)) return 1;
  if (sampler_status(m)) return 1;
  FP_HIP_OK(hipMemcpyAsync(poses_out, m->poses_dev, (size_t)n * 64, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  if (n_out) *n_out = n;
  return 0;
} FP_CATCH_INT

static int upload_poses(fp_model *m, Target *t, const float *poses, int N) {
  if (ensure_capacity(m, N, (size_t)t->mesh.V)) return 1;
  if (N > m->poses_pinned_cap) {
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    if (m->poses_pinned) (void)hipHostFree(m->poses_pinned);
    m->poses_pinned = nullptr; m->poses_pinned_cap = 0;
    FP_HIP_OK(hipHostMalloc((void **)&m->poses_pinned, (size_t)std::max(N, 256) * 64, hipHostMallocDefault));
    m->poses_pinned_cap = std::max(N, 256);
  }
  // every entry point synchronises the stream before it returns or before it calls this again
  std::memcpy(m->poses_pinned, poses, (size_t)N * 64);
  FP_HIP_OK(hipMemcpyAsync(m->poses_dev, m->poses_pinned, (size_t)N * 64, hipMemcpyHostToDevice, m->stream));
  return 0;
}

int fp_render_and_transform(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio,
                            float *render_out, float *transf_out, int out_memspace) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && N > 0, "[FoundationposeRender] The transform matrix vector is empty");
  FP_CHECK(m->depth != nullptr, "[FoundationPose] fp_render_and_transform: no frame uploaded");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] unknown target_name");
  if (stage_frame(m) || upload_poses(m, t, poses, N)) return 1;
  const size_t bytes = (size_t)N * FP_CROP_HW * FP_CROP_HW * 6 * sizeof(float);
  float *a = render_out, *b = transf_out;
  if (out_memspace == FP_HOST) {
    if (ensure_blobs(m)) return 1;
    a = render_out ? m->blob_a : nullptr;
    b = transf_out ? m->blob_b : nullptr;
  }
  if (render_and_crop(m, t, N, crop_ratio, OUT_F32X6, a, b, nullptr, nullptr)) return 1;
  if (out_memspace == FP_HOST) {
    if (render_out) FP_HIP_OK(hipMemcpyAsync(render_out, a, bytes, hipMemcpyDeviceToHost, m->stream));
    if (transf_out) FP_HIP_OK(hipMemcpyAsync(transf_out, b, bytes, hipMemcpyDeviceToHost, m->stream));
  }
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

int fp_debug_rasterize(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio,
                       int32_t *tri_id, float *rast_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && N > 0, "[FoundationposeRender] The transform matrix vector is empty");
  FP_CHECK(m->H > 0, "[FoundationPose] fp_debug_rasterize: no frame uploaded (image size unknown)");
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] unknown target_name");
  if (upload_poses(m, t, poses, N)) return 1;
  if (ensure_blobs(m)) return 1;
  size_t px = (size_t)m->cap * FP_CROP_HW * FP_CROP_HW;
  if (!m->dbg_tri && dev_alloc(&m->dbg_tri, px)) return 1;
  if (!m->dbg_rast && dev_alloc(&m->dbg_rast, px * 4)) return 1;
  if (render_and_crop(m, t, N, crop_ratio, OUT_F32X6, m->blob_a, nullptr, m->dbg_tri, m->dbg_rast)) return 1;
  size_t n = (size_t)N * FP_CROP_HW * FP_CROP_HW;
  if (tri_id) FP_HIP_OK(hipMemcpyAsync(tri_id, m->dbg_tri, n * 4, hipMemcpyDeviceToHost, m->stream));
  if (rast_out) FP_HIP_OK(hipMemcpyAsync(rast_out, m->dbg_rast, n * 16, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// blob-mode network entry points: f32 NHWC [N,160,160,6] -> packed fp16 input
static int pack_blobs(fp_model *m, const float *render_input, const float *transf_input, int memspace, int N) {
  FP_CHECK(render_input && transf_input && N > 0, "[FoundationPose] null network input");
  FP_CHECK(N <= FP_MAX_BATCH, "[FoundationPose] network batch " + std::to_string(N) + " above the batch limit FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH));
  if (ensure_capacity(m, N, 0)) return 1;
  const size_t px = (size_t)N * FP_CROP_HW * FP_CROP_HW;
  const float *a = render_input, *b = transf_input;
  if (memspace == FP_HOST) {
    if (ensure_blobs(m)) return 1;
    FP_HIP_OK(hipMemcpyAsync(m->blob_a, render_input, px * 24, hipMemcpyHostToDevice, m->stream));
    FP_HIP_OK(hipMemcpyAsync(m->blob_b, transf_input, px * 24, hipMemcpyHostToDevice, m->stream));
    a = m->blob_a; b = m->blob_b;
  }
  launch_pack_f32x6(m->stream, a, m->nn_in, px, nn_mode(m));
  launch_pack_f32x6(m->stream, b, m->nn_in + (size_t)N * FP_NN_IN_IMG_HALFS, px, nn_mode(m));
  return 0;
}

int fp_refiner_infer(fp_model *m, const float *render_input, const float *transf_input, int memspace, int N,
                     float *trans_out, float *rot_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && m->refiner, "[FoundationPose] refiner weights not loaded");
  if (pack_blobs(m, render_input, transf_input, memspace, N)) return 1;
  if (refiner_forward(m->stream, &m->prof, m->refiner, m->ws, m->nn_in, N, m->trans_dev, m->rot_dev)) return 1;
  FP_HIP_OK(hipMemcpyAsync(trans_out, m->trans_dev, (size_t)N * 12, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipMemcpyAsync(rot_out, m->rot_dev, (size_t)N * 12, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

int fp_scorer_infer(fp_model *m, const float *render_input, const float *transf_input, int memspace, int N,
                    float *scores_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && m->scorer, "[FoundationPose] scorer weights not loaded");
  if (pack_blobs(m, render_input, transf_input, memspace, N)) return 1;
  if (scorer_features(m->stream, &m->prof, m->scorer, m->ws, m->nn_in, N, m->feat_dev)) return 1;
  if (scorer_head(m->stream, &m->prof, m->scorer, m->ws, m->feat_dev, N, m->scores_dev)) return 1;
  FP_HIP_OK(hipMemcpyAsync(scores_out, m->scores_dev, (size_t)N * 4, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

int fp_refine_post_process(fp_model *m, const char *target_name, const float *poses, const float *trans,
                           const float *rot, int N, float *poses_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && trans && rot && poses_out && N > 0, "[FoundationPose] fp_refine_post_process: invalid arguments");
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] unknown target_name");
  if (ensure_capacity(m, N, 0)) return 1;
  FP_HIP_OK(hipMemcpyAsync(m->poses_dev, poses, (size_t)N * 64, hipMemcpyHostToDevice, m->stream));
  FP_HIP_OK(hipMemcpyAsync(m->trans_dev, trans, (size_t)N * 12, hipMemcpyHostToDevice, m->stream));
  FP_HIP_OK(hipMemcpyAsync(m->rot_dev, rot, (size_t)N * 12, hipMemcpyHostToDevice, m->stream));
  launch_pose_update(m->stream, m->poses_dev, m->trans_dev, m->rot_dev, N, t->mesh.diameter);
  FP_HIP_OK(hipMemcpyAsync(poses_out, m->poses_dev, (size_t)N * 64, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

int fp_argmax(fp_model *m, const float *scores, int N, int *index_out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && scores && index_out && N > 0, "[FoundationPose] fp_argmax: invalid arguments");
  if (ensure_capacity(m, N, 0)) return 1;
  FP_HIP_OK(hipMemcpyAsync(m->scores_dev, scores, (size_t)N * 4, hipMemcpyHostToDevice, m->stream));
  launch_argmax(m->stream, m->scores_dev, N, m->argmax_dev);
  int idx = -1;
  FP_HIP_OK(hipMemcpyAsync(&idx, m->argmax_dev, 4, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  // the kernel flags non-finite scores with -2 (used by the sharded Register); the reference's getMaxScoreIndex always returns an
  // index in [0, N): here a NaN score is an error, never an out-of-range index
  FP_CHECK(idx >= 0 && idx < N, "[FoundationPose] fp_argmax: scores are not finite");
  *index_out = idx;
  return 0;
} FP_CATCH_INT

// one refine iteration over m->poses_dev[0..N): RefinePreProcess + SyncInfer + RefinePostProcess, all on device
// shared_b: all N poses have the same translation (fresh sampler output), so the observed crop -- which depends only on
// the translation (foundationpose_render.cpp:59, foundationpose_render.cu:78-80) -- is computed and encoded once.
// poses_in / result_out (Track): the poses are read from / the refined poses also written to host-pinned memory
// fit_out (Track with the pose fit on, last iteration): the fit of the poses this iteration STARTS from, behind render_and_crop
static int refine_iteration(fp_model *m, Target *t, int N, bool shared_b, const float *poses_in = nullptr, float *result_out = nullptr,
                            unsigned *done_flag = nullptr, PoseFitRec *fit_out = nullptr) {
  RoctxRange range("refine_iteration (render + crop @1.2, refine-net, pose update)");
  const size_t half = (size_t)N * FP_NN_IN_IMG_HALFS;
  if (render_and_crop(m, t, N, 1.2f /* refine_mode_crop_ratio_ foundationpose.cpp:87 */, nn_mode(m), m->nn_in,
                      m->nn_in + half, nullptr, nullptr, shared_b ? 1 : N, poses_in))
    return 1;
  if (fit_out && !shared_b && enqueue_pose_fit(m, m->nn_in, m->nn_in + half, N, fit_tol_uniform(fit_tol_n(m->fit_tol_m, t->mesh.diameter)), fit_out)) return 1;
  checkpoint(m, 0, m->recs, (size_t)N * sizeof(PoseRec));
  checkpoint(m, 1, m->clip, (size_t)N * t->mesh.V * 16);
  checkpoint(m, 2, m->attr, (size_t)N * t->mesh.V * 16);
  checkpoint(m, 3, m->nn_in, (size_t)N * FP_NN_IN_IMG_HALFS * 2);
  checkpoint(m, 4, m->nn_in + half, (size_t)(shared_b ? 1 : N) * FP_NN_IN_IMG_HALFS * 2);
  // N == 1 (Track): the head kernel applies RefinePostProcess itself (one launch less); profiling / digests keep the stages apart
  const PoseUpdateFuse fuse{m->poses_dev, t->mesh.diameter, poses_in, result_out, done_flag};
  bool fused = false;
  if (refiner_forward(m->stream, &m->prof, m->refiner, m->ws, m->nn_in, N, m->trans_dev, m->rot_dev, shared_b ? 1 : 0,
                      (N == 1 && !m->prof.on && !m->digests) ? &fuse : nullptr, &fused))
    return 1;
  checkpoint(m, 5, m->trans_dev, (size_t)N * 12);
  checkpoint(m, 6, m->rot_dev, (size_t)N * 12);
  if (!fused) {
    ProfScope ps(&m->prof, m->stream, "pose_update");
    launch_pose_update(m->stream, m->poses_dev, m->trans_dev, m->rot_dev, N, t->mesh.diameter, poses_in, result_out);
  }
  checkpoint(m, 7, m->poses_dev, (size_t)N * 64);
  return 0;
}

// ---- Register: the two halves every Register entry point is made of.  Plain functions: the entry points hold the guard and the
// exception barrier, and say through the options what is theirs to decide.
struct RegisterBeginOpts {
  bool defer_verdict;   // no synchronisation here: the finish that follows on this stream reports the sampler's verdict
  bool calibration;     // a calibration drives this call (the networks record statistics between their launches): not graphable
};
struct RegisterFinishOpts { bool sampler_word; };   // this finish also reports the sampler word of this model (its begin left the verdict to it)

// sampler + refine iterations + score trunk over hypotheses [shard_begin, shard_begin + shard_count) of the grid -> pooled score
// features / refined poses in the model's buffers.  A failure leaves no pending state, but may leave enqueued work running.
static int register_begin(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                          const char *target_name, int refine_itr, int shard_begin, int shard_count, const RegisterBeginOpts &opts,
                          float **feat_dev, float **poses_dev) {
  RoctxRange range("fp_register_shard_begin (sampler + refine + score trunk)");
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  m->reg_pending = {};
  Target *t = nullptr;
  if (check_frame_args(m, H, W, target_name ? target_name : "", &t)) return 1;
  FP_CHECK(m->refiner && m->scorer, "[FoundationPose] refiner/scorer weights not loaded");
  FP_CHECK(mask != nullptr, "[FoundationPose] Register needs a mask");
  const int n_all = m->n_hyp();
  FP_CHECK(shard_begin >= 0 && shard_count > 0 && shard_begin + shard_count <= n_all,
           "[FoundationPose] hypothesis shard out of range");
  FP_CHECK(shard_count <= FP_MAX_BATCH, "[FoundationPose] hypothesis shard of " + std::to_string(shard_count) +
           " above the batch limit FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH));
  m->fit_reg_n = 0;
  m->fit_reg_why = m->fit_on ? "the last Register failed" : "the last Register ran with the pose fit off (fp_set_pose_fit)";
  // the pose fit covers a Register whose hypotheses all live on this model: a smaller shard computes none
  const bool fit = m->fit_on && shard_begin == 0 && shard_count == n_all;
  if (m->fit_on && !fit) m->fit_reg_why = "the last Register was sharded: a shard smaller than the hypothesis grid computes no pose fit";
  if (fit && ensure_fit(m)) return 1;
  if (upload_frame_async(m, rgb, depth, memspace, H, W)) return 1;
  const int N = shard_count;
  if (sample_hypotheses_async(m, t, mask, memspace, shard_begin, N)) return 1;
  const size_t half = (size_t)N * FP_NN_IN_IMG_HALFS;
  if (run_graphed(m, m->rg, t, H, W, refine_itr, N, graphable(m, refine_itr) && !opts.calibration, [&]() {
        for (int it = 0; it < refine_itr; it++)
          if (refine_iteration(m, t, N, it == 0 && N > 1)) return 1;  // sampler output: one translation for all hypotheses
        {
          RoctxRange r2("render + crop @1.1 (score mode)");
          if (render_and_crop(m, t, N, 1.1f /* score_mode_crop_ratio_ foundationpose.cpp:88 */, nn_mode(m), m->nn_in,
                              m->nn_in + half, nullptr, nullptr))
            return 1;
          // the fit of the FINAL poses: only reads the score pass's input
          if (fit && enqueue_pose_fit(m, m->nn_in, m->nn_in + half, N, fit_tol_uniform(fit_tol_n(m->fit_tol_m, t->mesh.diameter)), m->fit_rec)) return 1;
        }
        RoctxRange r3("score-net trunk + self-attention");
        checkpoint(m, 8, m->clip, (size_t)N * t->mesh.V * 16);
        checkpoint(m, 9, m->attr, (size_t)N * t->mesh.V * 16);
        checkpoint(m, 10, m->nn_in, (size_t)N * FP_NN_IN_IMG_HALFS * 2);
        checkpoint(m, 11, m->nn_in + half, (size_t)N * FP_NN_IN_IMG_HALFS * 2);
        if (scorer_features(m->stream, &m->prof, m->scorer, m->ws, m->nn_in, N, m->feat_dev)) return 1;
        checkpoint(m, 12, m->feat_dev, (size_t)N * 512 * 4);
        return 0;
      }))
    return 1;
  if (feat_dev) *feat_dev = m->feat_dev;
  if (poses_dev) *poses_dev = m->poses_dev;
  if (fit) { m->reg_pending.fit_n = N; m->fit_reg_tol = fit_tol_n(m->fit_tol_m, t->mesh.diameter); m->fit_reg_diam = t->mesh.diameter; }
  if (opts.defer_verdict) return 0;
  // synchronises: the returned buffers are complete (and the GPU lock may be released); reports the sampler's verdict
  if (sampler_status(m)) {
    set_error(std::string("[FoundationPose] Failed to generate hyp poses!!! ") + g_last_error);
    return 1;
  }
  return 0;
}

// cross-hypothesis head + arg-max over N_total hypotheses (this model's or the gathered ones of every rank) and the call's ONE
// synchronisation
static int register_finish(fp_model *m, const float *all_feat_dev, const float *all_poses_dev, int N_total, float out_pose[16],
                           int *best_index, float *scores_host, const RegisterFinishOpts &opts) {
  FP_CHECK(m && m->scorer && all_feat_dev && all_poses_dev && N_total > 0 && out_pose,
           "[FoundationPose] fp_register_shard_finish: invalid arguments");
  RoctxRange range("fp_register_shard_finish (cross-hypothesis head + arg-max)");
  const RegisterPending pending = m->reg_pending;
  m->reg_pending = {};
  // (the records of a begin over all hypotheses belong to this finish when it ranks exactly those, from the model's own buffers)
  const bool fit = pending.fit_n > 0 && pending.fit_n == N_total && all_poses_dev == m->poses_dev && m->fit_io_dev;
  if (pending.fit_n > 0 && !fit) m->fit_reg_why = "the last Register was sharded: its finish ranked other hypotheses than its begin fitted";
  m->fit_reg_n = 0;
  float *scores = m->scores_dev;
  if (N_total > m->cap) {  // gathered hypotheses of all ranks: a persistent buffer, not a malloc/free per Register
    if (N_total > m->scores_all_cap) {
      dev_free(m->scores_all);
      m->scores_all_cap = 0;
      if (dev_alloc(&m->scores_all, (size_t)N_total)) return 1;
      m->scores_all_cap = N_total;
    }
    scores = m->scores_all;
  }
  if (!m->best_pose_dev && dev_alloc(&m->best_pose_dev, 16)) return 1;
  if (!m->result_pinned) FP_HIP_OK(pinned_mapped_alloc(&m->result_pinned, &m->result_pinned_dev, 64 * sizeof(int), hipHostMallocMapped));
  int rc = scorer_head(m->stream, &m->prof, m->scorer, m->ws, all_feat_dev, N_total, scores);
  if (!rc) checkpoint(m, 13, scores, (size_t)N_total * 4);
  if (!rc) {
    ProfScope ps(&m->prof, m->stream, "argmax");
    launch_argmax(m->stream, scores, N_total, m->argmax_dev, all_poses_dev, m->best_pose_dev);
  }
  // ONE synchronisation: winner index, the sampler's status word (opts.sampler_word) and the pose
  // [r6] written by a kernel into the pinned, device-mapped block: no device -> host copy command in front of the synchronisation
  int *res = m->result_pinned;
  res[0] = -3; res[1] = 3;   // (overwritten by the kernel; what a kernel that never ran would leave is an error, not a stale winner)
  if (!rc) {
    hipLaunchKernelGGL(fp::publish_result_kernel, dim3(1), dim3(64), 0, m->stream, m->argmax_dev, opts.sampler_word ? m->samp_state + 6 : nullptr, m->best_pose_dev, m->result_pinned_dev);
    if (hipGetLastError() != hipSuccess) rc = 1;
  }
  if (!rc && fit) {
    hipLaunchKernelGGL(fp::publish_fit_kernel, dim3(1), dim3(1), 0, m->stream, m->argmax_dev, m->fit_rec, N_total, m->fit_io_dev + 64);
    if (hipGetLastError() != hipSuccess) rc = 1;
  }
  if (!rc && scores_host &&
      hipMemcpyAsync(scores_host, scores, (size_t)N_total * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess)
    rc = 1;
  if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) rc = 1;
  if (!rc) {
    // the sampler's verdict first: on failure the caller's pose is left untouched, like the reference, which returns
    // false before it writes out_pose_in_mesh (foundationpose.cpp:196-201)
    if (const char *why = sampler_verdict(res[1])) { set_error(std::string("[FoundationPose] Failed to generate hyp poses!!! ") + why); rc = 1; }
    else if (res[0] == -2) { set_error("[FoundationPose] scores are not finite (a rank of a sharded Register reported a failed shard, or the weights are broken)"); rc = 1; }
  }
  if (!rc) {
    std::memcpy(out_pose, &res[2], 64);
    if (best_index) *best_index = res[0];
    if (fit) { m->fit_reg_n = N_total; m->fit_reg_index = res[0]; }
  }
  if (rc && g_last_error.empty()) set_error("[FoundationPose] fp_register_shard_finish failed");
  return rc;
}

// begin + finish back to back on one stream over the whole grid: a single synchronisation, at the end
static int register_whole(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                          const char *target_name, int refine_itr, float out_pose[16], bool calibration) {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  float *feat = nullptr, *poses = nullptr;
  if (register_begin(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, 0, m->n_hyp(), {/*defer_verdict*/ true, calibration}, &feat, &poses)) {
    (void)hipStreamSynchronize(m->stream);
    return 1;
  }
  return register_finish(m, feat, poses, m->n_hyp(), out_pose, nullptr, nullptr, {/*sampler_word*/ true});
}

int fp_register_shard_begin(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H,
                            int W, const char *target_name, int refine_itr, int shard_begin, int shard_count,
                            float **feat_dev, float **poses_dev) try {
  SerialGuard serial(m ? m->device : -1);
  return register_begin(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, shard_begin, shard_count, RegisterBeginOpts{}, feat_dev, poses_dev);
} FP_CATCH_INT

int fp_register_shard_finish(fp_model *m, const float *all_feat_dev, const float *all_poses_dev, int N_total,
                             float out_pose[16], int *best_index, float *scores_host) try {
  SerialGuard serial(m ? m->device : -1);
  return register_finish(m, all_feat_dev, all_poses_dev, N_total, out_pose, best_index, scores_host, RegisterFinishOpts{});
} FP_CATCH_INT

int fp_download(fp_model *m, void *dst_host, const void *src_dev, size_t bytes) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && dst_host && src_dev, "[FoundationPose] fp_download: invalid arguments");
  if (bytes) FP_HIP_OK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
} FP_CATCH_INT

// Sharded Register without host stalls: everything is enqueued on the model's stream, nothing is allocated or synchronised.
static int register_begin_packed(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                                 const char *target_name, int refine_itr, int shard_begin, int shard_count, float *packed_dev,
                                 int rows_per_rank) {
  FP_CHECK(m && packed_dev && rows_per_rank >= shard_count && shard_count >= 0, "[FoundationPose] fp_register_shard_begin_packed: invalid arguments");
  float *feat = nullptr, *poses = nullptr;
  int rc;
  if (shard_count > 0) {
    rc = register_begin(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, shard_begin, shard_count, {/*defer_verdict*/ true, /*calibration*/ false},
                        &feat, &poses);
  } else {
    // an empty shard still runs the (cheap) sampler, so that a bad mask fails on EVERY rank alike
    m->reg_pending = {};
    Target *t = nullptr;
    if (check_frame_args(m, H, W, target_name ? target_name : "", &t)) return 1;
    FP_CHECK(mask != nullptr, "[FoundationPose] Register needs a mask");
    rc = upload_frame_async(m, rgb, depth, memspace, H, W) || sample_hypotheses_async(m, t, mask, memspace, 0, 1);
  }
  if (rc) { (void)hipStreamSynchronize(m->stream); return 1; }
  m->reg_pending.sampler = true;
  const int n = rows_per_rank * 528;
  hipLaunchKernelGGL(pack_shard_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, feat, poses, shard_count, rows_per_rank, packed_dev, m->samp_state + 6);
  FP_HIP_OK(hipGetLastError());
  return 0;
}

static int register_finish_packed(fp_model *m, const float *gathered_dev, int n_total, float out_pose[16], int *best_index) {
  FP_CHECK(m && gathered_dev && n_total > 0 && out_pose, "[FoundationPose] fp_register_shard_finish_packed: invalid arguments");
  if (n_total > m->gath_cap) {
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    dev_free(m->gath_feat); dev_free(m->gath_poses);
    m->gath_cap = 0;
    if (dev_alloc(&m->gath_feat, (size_t)n_total * 512) || dev_alloc(&m->gath_poses, (size_t)n_total * 16)) return 1;
    m->gath_cap = n_total;
  }
  const int n = n_total * 528;
  hipLaunchKernelGGL(unpack_shards_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, gathered_dev, n_total, m->gath_feat, m->gath_poses);
  // the sampler's verdict of this rank's begin is fetched together with the result
  return register_finish(m, m->gath_feat, m->gath_poses, n_total, out_pose, best_index, nullptr, {/*sampler_word*/ m->reg_pending.sampler});
}

int fp_register_shard_begin_packed(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H,
                                   int W, const char *target_name, int refine_itr, int shard_begin, int shard_count,
                                   float *packed_dev, int rows_per_rank) try {
  SerialGuard serial(m ? m->device : -1);
  return register_begin_packed(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, shard_begin, shard_count, packed_dev, rows_per_rank);
} FP_CATCH_INT

int fp_register_shard_finish_packed(fp_model *m, const float *gathered_dev, int n_total, float out_pose[16], int *best_index) try {
  SerialGuard serial(m ? m->device : -1);
  return register_finish_packed(m, gathered_dev, n_total, out_pose, best_index);
} FP_CATCH_INT

// ---- native sharded Register: begin -> ONE ncclAllGather (RCCL over xGMI) on the model's stream -> finish.  No torch, no events
// across runtimes: the collective is ordered by the stream itself.  RCCL is bound at first use with dlopen / dlsym -- first an
// already loaded copy (a Python host has torch's bundled librccl in the process: a communicator made by torch.distributed belongs to
// THAT copy), otherwise librccl.so.1 of the ROCm installation -- so that the library itself has no link-time RCCL dependency and
// geometry-only / single-GPU users never load it.
namespace {
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
typedef const char *(*nccl_errstr_fn)(int);
typedef int (*nccl_count_fn)(void *, int *);
typedef int (*nccl_abort_fn)(void *);
struct RcclApi {
  nccl_abort_fn abort = nullptr;   // optional: lets a rank that cannot join the collective release the others
  nccl_allgather_fn all_gather = nullptr;
  nccl_errstr_fn err = nullptr;
  nccl_count_fn count = nullptr, user_rank = nullptr;
  std::string why;
};
const RcclApi &rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void *h = nullptr;
    // a copy that is already in the process, whatever its file name / soname (torch wheels ship `torch/lib/librccl.so`): the
    // communicator the caller hands over was made by THAT copy
    std::string loaded;
    dl_iterate_phdr([](struct dl_phdr_info *info, size_t, void *out) {
      if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) { *(std::string *)out = info->dlpi_name; return 1; }
      return 0;
    }, &loaded);
    if (!loaded.empty()) h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    for (const char *name : {"librccl.so.1", "librccl.so"}) if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      const char *why = dlerror();   // (one call: dlerror clears the message it returns)
      a.why = std::string("cannot load librccl: ") + (why ? why : "?");
      return a;
    }
    a.all_gather = (nccl_allgather_fn)dlsym(h, "ncclAllGather");
    a.err = (nccl_errstr_fn)dlsym(h, "ncclGetErrorString");
    a.count = (nccl_count_fn)dlsym(h, "ncclCommCount");
    a.user_rank = (nccl_count_fn)dlsym(h, "ncclCommUserRank");
    a.abort = (nccl_abort_fn)dlsym(h, "ncclCommAbort");
    if (!a.all_gather || !a.err || !a.count || !a.user_rank) { a.why = "librccl lacks ncclAllGather / ncclCommCount / ncclCommUserRank"; a.all_gather = nullptr; }
    return a;
  }();
  return api;
}
__global__ void poison_rows_kernel(float *p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = __int_as_float(0x7fc00000);
}
}  // namespace

int fp_register_sharded(fp_model *m, void *nccl_comm, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                        const char *target_name, int refine_itr, float out_pose[16], int *best_index) try {
  FP_CHECK(m && nccl_comm && out_pose, "[FoundationPose] fp_register_sharded: invalid arguments");
  const RcclApi &nccl = rccl_api();
  FP_CHECK(nccl.all_gather != nullptr, "[FoundationPose] fp_register_sharded: " + nccl.why);
  int world = 0, rank = -1, rc;
  if ((rc = nccl.count(nccl_comm, &world)) != 0 || (rc = nccl.user_rank(nccl_comm, &rank)) != 0 || world < 1 || rank < 0 || rank >= world) {
    set_error(std::string("[FoundationPose] fp_register_sharded: bad communicator: ") + (rc ? nccl.err(rc) : "rank / size out of range"));
    return 1;
  }
  struct NoSerial {   // (see g_no_serial; restored on every return path)
    bool prev = g_no_serial;
    explicit NoSerial(bool off) { if (off) g_no_serial = true; }
    ~NoSerial() { g_no_serial = prev; }
  } no_serial(world > 1);
  SerialGuard serial(m->device);
  const int n_total = m->n_hyp();
  const int per = (n_total + world - 1) / world;
  const int begin = std::min(rank * per, n_total), count = std::min(per, n_total - begin);
  // Everything that can fail on THIS rank alone happens behind a promise to the other ranks: they are already heading for the
  // collective.  A failure of the begin half joins it with NaN rows (every rank's finish reports them) and returns the error
  // afterwards; a rank that cannot even hold its exchange buffers cannot join -- it aborts the communicator (ncclCommAbort: the
  // others' collective returns an error instead of hanging) and says so.
  auto cannot_join = [&](const std::string &why) {
    const bool aborted = world > 1 && nccl.abort && nccl.abort(nccl_comm) == 0;
    set_error("[FoundationPose] fp_register_sharded: " + why + (world > 1 ? (aborted ? " -- the communicator was aborted so that the other ranks do not wait for this one (it must be re-created)"
                                                                                      : " -- this rank could not join the collective and ncclCommAbort is unavailable: the other ranks may wait") : ""));
    return 1;
  };
  // persistent exchange buffers (grown on demand; a Register never allocates in steady state)
  const size_t need_send = (size_t)per * 528, need_recv = (size_t)world * per * 528;
  if (need_send > m->shard_send_cap || need_recv > m->shard_recv_cap) {
    if (hipStreamSynchronize(m->stream) != hipSuccess) return cannot_join("the model's stream is in an error state");
    auto grow = [](float *&buf, size_t &cap, size_t need) {
      if (need <= cap) return true;
      dev_free(buf); cap = 0;
      if (hipMalloc((void **)&buf, need * sizeof(float)) != hipSuccess) { buf = nullptr; return false; }
      cap = need;
      return true;
    };
    if (!grow(m->shard_send, m->shard_send_cap, need_send) || !grow(m->shard_recv, m->shard_recv_cap, need_recv))
      return cannot_join("out of device memory for the exchange buffers");
  }
  const int rc_begin = register_begin_packed(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, begin, count, m->shard_send, per);
  std::string begin_error;
  if (rc_begin) {
    begin_error = g_last_error;
    hipLaunchKernelGGL(poison_rows_kernel, dim3((unsigned)((need_send + 255) / 256)), dim3(256), 0, m->stream, m->shard_send, need_send);
  }
  if (world > 1) {
    rc = nccl.all_gather(m->shard_send, m->shard_recv, need_send, 7 /* ncclFloat32 */, nccl_comm, m->stream);
    if (rc != 0) {
      (void)hipStreamSynchronize(m->stream);
      set_error(std::string("[FoundationPose] ncclAllGather failed: ") + nccl.err(rc) + (rc_begin ? " (after: " + begin_error + ")" : ""));
      return 1;
    }
  } else {
    FP_HIP_OK(hipMemcpyAsync(m->shard_recv, m->shard_send, need_send * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
  }
  if (rc_begin) {
    (void)hipStreamSynchronize(m->stream);
    set_error(begin_error);
    return 1;
  }
  return register_finish_packed(m, m->shard_recv, n_total, out_pose, best_index);
} FP_CATCH_INT

int fp_register_ex(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                   const char *target_name, int refine_itr, float out_pose[16]) try {
  SerialGuard serial(m ? m->device : -1);
  return register_whole(m, rgb, depth, mask, memspace, H, W, target_name, refine_itr, out_pose, false);
} FP_CATCH_INT

int fp_register(fp_model *m, const uint8_t *rgb, const float *depth, const uint8_t *mask, int H, int W,
                const char *target_name, int refine_itr, float out_pose[16]) try {
  return fp_register_ex(m, rgb, depth, mask, FP_HOST, H, W, target_name, refine_itr, out_pose);
} FP_CATCH_INT

// Track with the depth filter on: D' on the rectangle the frame record names, before anything reads it
static void enqueue_depth_filter(fp_model *m) {
  ProfScope ps(&m->prof, m->stream, "depth_filter_rect");
  launch_depth_filter_rect(m->stream, m->frame_dev, m->H, m->W);
}

// why a Track that is starting leaves no fit record, unless it succeeds with the option on (fp_last_track_fit reports it)
static const char *no_track_fit_because(const fp_model *m, int refine_itr) {
  return !m->fit_on ? "the last Track ran with the pose fit off (fp_set_pose_fit)"
       : refine_itr <= 0 ? "the last Track ran with refine_itr <= 0: nothing was rendered, so there is no record" : "the last Track failed";
}

// Track in two halves: everything is ENQUEUED by fp_track_submit (frame upload, the replayed graph); fp_track_wait synchronises the
// model's stream and hands the pose over.  One host thread can so keep several models (objects) in flight at once.
static int track_submit_impl(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, const float hyp_pose[16],
                             const char *target_name, int refine_itr) {
  RoctxRange range("fp_track_submit");
  Target *t = nullptr;
  if (check_frame_args(m, H, W, target_name ? target_name : "", &t)) return 1;
  FP_CHECK(m->refiner, "[FoundationPose] refiner weights not loaded");
  FP_CHECK(hyp_pose, "[FoundationPose] Track: null pose");
  FP_CHECK(!m->track_pending, "[FoundationPose] fp_track_submit: the previous submission has not been waited for");
  m->fit_track_n = 0;
  m->fit_track_why = no_track_fit_because(m, refine_itr);
  const bool fit = m->fit_on && refine_itr >= 1;
  if (fit && ensure_fit(m)) return 1;
  // a single refine iteration reads the frame only inside the observed-crop window of the hypothesis (ComputeCropWindowTF,
  // foundationpose_render.cpp:25-70, restated on the host in double with a margin): host frames upload just those rows
  // (plan_track_window; with the depth filter on, a device frame is read inside the same window, and a host frame uploads the
  // window grown by the filter's reach of 4 pixels: erode 2 + bilateral 2)
  int row0 = 0, row1 = -1, col0 = 0, col1 = -1;
  TrackWindow filt = {TRACK_WINDOW_WHOLE, 0, H, 0, W};
  if (refine_itr == 1 && (memspace != FP_DEVICE || m->dfilt_on)) {
    filt = plan_track_window(m->K, t->mesh.diameter, hyp_pose, H, W, 0);
    const TrackWindow up = m->dfilt_on ? plan_track_window(m->K, t->mesh.diameter, hyp_pose, H, W, 4) : filt;
    if (up.kind == TRACK_WINDOW_OUTSIDE) { row0 = 0; row1 = 0; }
    else if (up.kind != TRACK_WINDOW_WHOLE) {
      row0 = up.row0; row1 = up.row1;
      if (up.kind == TRACK_WINDOW_RECT) { col0 = up.col0; col1 = up.col1; }
    }
  }
  if (upload_frame_async(m, rgb, depth, memspace, H, W, row0, row1, col0, col1, m->dfilt_on && filt.kind != TRACK_WINDOW_WHOLE ? &filt : nullptr)) return 1;
  // (fine-grained: the done flag is read while the graph is still running)
  if (!m->track_io) FP_HIP_OK(pinned_mapped_alloc(&m->track_io, &m->track_io_dev, 48 * sizeof(float), hipHostMallocCoherent));
  m->track_flag_armed = false;
  if (refine_itr <= 0) {  // no refinement requested: the hypothesis is the answer (the reference's loop runs zero times)
    std::memcpy(m->track_io + 16, hyp_pose, 64);
    m->track_pending = true;
    return 0;
  }
  if (ensure_capacity(m, 1, (size_t)t->mesh.V)) return 1;
  // the hypothesis goes in and the refined pose comes out through host-pinned memory the kernels address directly: no copy
  // kernels around the graph (two of the ~50 launches of a Track)
  std::memcpy(m->track_io, hyp_pose, 64);
  // completion flag (own cache line of the pinned block): cleared here, raised by the last kernel after it stored the refined pose.
  // Armed only when that kernel is the fused head + pose-update kernel (not while profiling / taking digests: separate stages there)
  volatile unsigned *flag = reinterpret_cast<volatile unsigned *>(m->track_io + 32);
  *flag = 0u;
  const bool armed = !m->prof.on && !m->digests && refiner_fuses_pose(m->refiner);
  if (run_graphed(m, m->tg, t, H, W, refine_itr, 1, graphable(m, refine_itr), [&]() {
        if (m->dfilt_on) enqueue_depth_filter(m);   // the rectangle comes from the frame record: the captured launch serves every pose
        for (int it = 0; it < refine_itr; it++) {
          const bool last = it == refine_itr - 1;
          if (refine_iteration(m, t, 1, false, it == 0 ? m->track_io_dev : nullptr, last ? m->track_io_dev + 16 : nullptr,
                               last ? reinterpret_cast<unsigned *>(m->track_io_dev + 32) : nullptr, last && fit ? m->fit_io_dev : nullptr))
            return 1;
        }
        return 0;
      }))
    return 1;
  m->track_flag_armed = armed;
  m->track_pending = true;
  if (fit) { m->fit_track_n = 1; m->fit_track_tol[0] = fit_tol_n(m->fit_tol_m, t->mesh.diameter); m->fit_track_diam[0] = t->mesh.diameter; }
  return 0;
}

static int track_submit(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, const float hyp_pose[16],
                        const char *target_name, int refine_itr) {
  const int rc = track_submit_impl(m, rgb, depth, memspace, H, W, hyp_pose, target_name, refine_itr);
  // a failure after the upload was enqueued must not leave H2D copies of the caller's host frame in flight
  if (rc && m && m->stream) (void)hipStreamSynchronize(m->stream);
  return rc;
}

static int track_wait(fp_model *m, float out_pose[16]) {
  FP_CHECK(m && out_pose, "[FoundationPose] fp_track_wait: invalid arguments");
  FP_CHECK(m->track_pending, "[FoundationPose] fp_track_wait: nothing was submitted");
  m->track_pending = false;
  if (m->track_flag_armed) {
    // the last kernel of the Track raises a flag in host-pinned memory right after it stored the pose there: poll that instead of the
    // stream (later work on the model's stream is ordered behind the graph anyway).  Bounded: a fault, or a graph captured under
    // other settings, falls through to the stream wait, which also reports the error.
    m->track_flag_armed = false;
    volatile unsigned *flag = reinterpret_cast<volatile unsigned *>(m->track_io + 32);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    // (a raised flag IS the proof of success: the kernel that raises it is the last of the chain and a faulted stream never runs it;
    // spin briefly -- a Track takes ~0.2 ms -- then yield the core between looks)
    bool yielding = false;
    while (*flag == 0u) {
      if (yielding) std::this_thread::yield();
      else {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        asm volatile("yield");
#endif
      }
      if ((++spins & 1023u) == 0 || yielding) {
        const auto waited = std::chrono::steady_clock::now() - t0;
        if (waited > std::chrono::milliseconds(20)) break;
        yielding = waited > std::chrono::microseconds(500);
      }
    }
    if (*flag != 0u) {
      std::atomic_thread_fence(std::memory_order_acquire);
      std::memcpy(out_pose, m->track_io + 16, 64);
      return 0;
    }
  }
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  std::memcpy(out_pose, m->track_io + 16, 64);
  return 0;
}

int fp_track_submit(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, const float hyp_pose[16],
                    const char *target_name, int refine_itr) try {
  SerialGuard serial(m ? m->device : -1);
  return track_submit(m, rgb, depth, memspace, H, W, hyp_pose, target_name, refine_itr);
} FP_CATCH_INT

int fp_track_wait(fp_model *m, float out_pose[16]) try {
  SerialGuard serial(m ? m->device : -1);
  return track_wait(m, out_pose);
} FP_CATCH_INT

// Track of K objects of one frame in ONE batch: the geometry runs per object (its mesh), the refine-net once over all K crops.
// Track is launch-latency-bound at N = 1, so K objects cost little more than one (tools/bench_multi_track.py).
int fp_track_multi(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, int K, const float *hyp_poses,
                   const char *const *target_names, int refine_itr, float *out_poses) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  static_assert(64 <= FP_MAX_BATCH, "fp_track_multi: the object count is one network batch");
  FP_CHECK(K >= 1 && K <= 64 && hyp_poses && target_names && out_poses, "[FoundationPose] fp_track_multi: invalid arguments (1..64 objects)");
  FP_CHECK(m->refiner, "[FoundationPose] refiner weights not loaded");
  FP_CHECK(!m->track_pending, "[FoundationPose] fp_track_multi: a submitted Track has not been waited for");
  std::vector<Target *> targets(K);
  std::vector<std::pair<int, int>> groups;   // (first object, count) of every run of consecutive objects with one mesh
  size_t maxV = 0;
  for (int i = 0; i < K; i++) {
    Target *t = nullptr;
    if (check_frame_args(m, H, W, target_names[i] ? target_names[i] : "", &t)) return 1;
    targets[i] = t;
    maxV = std::max(maxV, (size_t)t->mesh.V);
    if (i > 0 && targets[i - 1] == t) groups.back().second++;
    else groups.emplace_back(i, 1);
  }
  m->fit_track_n = 0;
  m->fit_track_why = no_track_fit_because(m, refine_itr);
  const bool fit = m->fit_on && refine_itr >= 1;
  PoseFitTol fit_tol = {};   // per object: the meshes' diameters differ
  if (fit) {
    if (ensure_fit(m)) return 1;
    for (int i = 0; i < K; i++) fit_tol.v[i] = fit_tol_n(m->fit_tol_m, targets[i]->mesh.diameter);
  }
  if (upload_frame_async(m, rgb, depth, memspace, H, W)) return 1;
  if (refine_itr <= 0) {
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    std::memcpy(out_poses, hyp_poses, (size_t)K * 64);
    return 0;
  }
  if (ensure_capacity(m, K, maxV)) return 1;
  if (!m->multi_io) {   // once, for the largest object count
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    g_alloc_epoch++;   // graphs bake the pinned addresses
    FP_HIP_OK(pinned_mapped_alloc(&m->multi_io, &m->multi_io_dev, (size_t)2 * 64 * 16 * sizeof(float), hipHostMallocDefault));
  }
  std::memcpy(m->multi_io, hyp_poses, (size_t)K * 64);
  if (m->mg_sig != targets) { drop_graph(m->mg); m->mg.target = nullptr; m->mg_sig = targets; }
  float *pin_in = m->multi_io_dev, *pin_out = m->multi_io_dev + 64 * 16;
  const size_t IMG = FP_NN_IN_IMG_HALFS;
  if (run_graphed(m, m->mg, targets[0], H, W, refine_itr, K, graphable(m, refine_itr), [&]() {
        if (m->dfilt_on) enqueue_depth_filter(m);   // (the whole frame)
        for (int it = 0; it < refine_itr; it++) {
          for (const auto &[o, n] : groups)
            if (render_and_crop(m, targets[o], n, 1.2f, nn_mode(m), m->nn_in + (size_t)o * IMG, m->nn_in + (size_t)(K + o) * IMG, nullptr, nullptr, n,
                                (it == 0 ? pin_in : m->poses_dev) + (size_t)o * 16, m->recs + o))
              return 1;
          // one launch over all K objects: object o's crop is image K + o, its threshold its own mesh's
          if (fit && it == refine_itr - 1 && enqueue_pose_fit(m, m->nn_in, m->nn_in + (size_t)K * IMG, K, fit_tol, m->fit_io_dev)) return 1;
          if (refiner_forward(m->stream, &m->prof, m->refiner, m->ws, m->nn_in, K, m->trans_dev, m->rot_dev, 0)) return 1;
          for (const auto &[o, n] : groups)
            launch_pose_update(m->stream, m->poses_dev + (size_t)o * 16, m->trans_dev + (size_t)o * 3, m->rot_dev + (size_t)o * 3, n,
                               targets[o]->mesh.diameter, it == 0 ? pin_in + (size_t)o * 16 : nullptr,
                               it == refine_itr - 1 ? pin_out + (size_t)o * 16 : nullptr);
        }
        return 0;
      }))
    return 1;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  std::memcpy(out_poses, m->multi_io + 64 * 16, (size_t)K * 64);
  if (fit) {
    for (int i = 0; i < K; i++) { m->fit_track_tol[i] = fit_tol.v[i]; m->fit_track_diam[i] = targets[i]->mesh.diameter; }
    m->fit_track_n = K;
  }
  return 0;
} FP_CATCH_INT

int fp_track_ex(fp_model *m, const void *rgb, const void *depth, int memspace, int H, int W, const float hyp_pose[16],
                const char *target_name, int refine_itr, float out_pose[16]) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(out_pose, "[FoundationPose] Track: null pose");
  // an earlier fp_track_submit that is still in flight is the caller's to wait for: refuse without touching it
  FP_CHECK(!m || !m->track_pending, "[FoundationPose] Track: a submitted Track has not been waited for (fp_track_wait)");
  if (track_submit(m, rgb, depth, memspace, H, W, hyp_pose, target_name, refine_itr)) return 1;   // (synchronised; nothing is pending)
  return track_wait(m, out_pose);
} FP_CATCH_INT

int fp_track(fp_model *m, const uint8_t *rgb, const float *depth, int H, int W, const float hyp_pose[16],
             const char *target_name, int refine_itr, float out_pose[16]) try {
  return fp_track_ex(m, rgb, depth, FP_HOST, H, W, hyp_pose, target_name, refine_itr, out_pose);
} FP_CATCH_INT

// ---- pose fit: the option, the getters of the last call's records, the stage operator
int fp_set_pose_fit(fp_model *m, int on, float tol_m) try {
  LifeExclusive life;   // may destroy the captured graphs: not while another thread is inside a call
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(std::isfinite(tol_m) && tol_m > 0.0f, "[FoundationPose] fp_set_pose_fit: tol_m must be finite and > 0 (metres)");
  DeviceScope on_device(m->device);
  if ((on != 0) == m->fit_on && tol_m == m->fit_tol_m) return 0;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  m->fit_on = on != 0;
  m->fit_tol_m = tol_m;
  invalidate_graphs(m);   // the kernel and its threshold are part of the captured bodies
  return 0;
} FP_CATCH_INT
int fp_get_pose_fit(const fp_model *m, int *on, float *tol_m) try {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  if (on) *on = m->fit_on ? 1 : 0;
  if (tol_m) *tol_m = m->fit_tol_m;
  return 0;
} FP_CATCH_INT

// ---- depth filter
int fp_set_depth_filter(fp_model *m, int on) try {
  LifeExclusive life;   // destroys the captured graphs: not while another thread is inside a call
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  DeviceScope on_device(m->device);
  if ((on != 0) == m->dfilt_on) return 0;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  m->dfilt_on = on != 0;
  invalidate_graphs(m);   // the filter launch is part of the captured Track bodies
  return 0;
} FP_CATCH_INT
int fp_get_depth_filter(const fp_model *m) {
  if (!m) { set_error("[FoundationPose] null model"); return -1; }
  return m->dfilt_on ? 1 : 0;
}

// ---- vertex colours (DESIGN.md sections 3, 4.1): the target's colour source is its packed colour array when it has one
int fp_set_vertex_colors(fp_model *m, const char *target_name, const uint8_t *colors, int num_vertices) try {
  LifeExclusive life;   // destroys the captured graphs: not while another thread is inside a call
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] fp_set_vertex_colors: unknown target_name");
  FP_CHECK(!colors || num_vertices == t->mesh.V, "[FoundationPose] fp_set_vertex_colors: got " + std::to_string(num_vertices) +
                                                     " colours for a target of " + std::to_string(t->mesh.V) + " vertices");
  if (!colors && !t->mesh.vcol) return 0;
  DeviceScope on_device(m->device);
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  invalidate_graphs(m);   // the kernel of the colour source and the array's address are part of the captured bodies
  if (!colors) { dev_free(t->mesh.vcol); return 0; }
  std::vector<uint32_t> packed((size_t)t->mesh.V);
  for (size_t k = 0; k < packed.size(); k++)
    packed[k] = (uint32_t)colors[k * 3] | (uint32_t)colors[k * 3 + 1] << 8 | (uint32_t)colors[k * 3 + 2] << 16;
  uint32_t *dev = t->mesh.vcol;
  if (!dev && dev_alloc(&dev, packed.size())) return 1;
  if (fp::memcpy_sync(dev, packed.data(), packed.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    if (!t->mesh.vcol) dev_free(dev);   // (a fresh array: the target keeps its texture)
    FP_CHECK(false, "[FoundationPose] fp_set_vertex_colors: copying the colours to the device failed");
  }
  t->mesh.vcol = dev;
  return 0;
} FP_CATCH_INT
int fp_get_color_source(const fp_model *m, const char *target_name) try {
  Target *t = m ? const_cast<fp_model *>(m)->find(target_name ? target_name : "") : nullptr;
  if (!t) { set_error(m ? "[FoundationPose] fp_get_color_source: unknown target_name" : "[FoundationPose] null model"); return -1; }
  return t->mesh.vcol ? FP_COLOR_VERTEX : FP_COLOR_TEXTURE;
} FP_CATCH_INT

int fp_last_track_fit(fp_model *m, fp_pose_fit *out, int K) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && out, "[FoundationPose] fp_last_track_fit: invalid arguments");
  FP_CHECK(!m->track_pending, "[FoundationPose] fp_last_track_fit: the submitted Track has not been waited for (fp_track_wait)");
  FP_CHECK(m->fit_track_n > 0, "[FoundationPose] fp_last_track_fit: no record: " + m->fit_track_why);
  FP_CHECK(K >= m->fit_track_n, "[FoundationPose] fp_last_track_fit: the last Track left " + std::to_string(m->fit_track_n) + " records, room for " + std::to_string(K));
  for (int i = 0; i < m->fit_track_n; i++) fit_record(out + i, m->fit_io[i], m->fit_track_tol[i], m->fit_track_diam[i]);
  return 0;
} FP_CATCH_INT

int fp_last_register_fit(fp_model *m, fp_pose_fit *winner, fp_pose_fit *all, int N) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && (winner || all), "[FoundationPose] fp_last_register_fit: invalid arguments");
  FP_CHECK(m->fit_reg_n > 0, "[FoundationPose] fp_last_register_fit: no record: " + m->fit_reg_why);
  FP_CHECK(!all || N >= m->fit_reg_n, "[FoundationPose] fp_last_register_fit: the last Register left " + std::to_string(m->fit_reg_n) + " records, room for " + std::to_string(N));
  if (winner) fit_record(winner, m->fit_io[64], m->fit_reg_tol, m->fit_reg_diam);
  if (all) {   // diagnostic path: a device -> host copy on the model's stream
    std::vector<PoseFitRec> recs((size_t)m->fit_reg_n);
    FP_HIP_OK(hipMemcpyAsync(recs.data(), m->fit_rec, recs.size() * sizeof(PoseFitRec), hipMemcpyDeviceToHost, m->stream));
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    for (int i = 0; i < m->fit_reg_n; i++) fit_record(all + i, recs[(size_t)i], m->fit_reg_tol, m->fit_reg_diam);
  }
  return 0;
} FP_CATCH_INT

int fp_pose_fit_eval(fp_model *m, const char *target_name, const float *poses, int N, float crop_ratio, float tol_m, fp_pose_fit *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && out && N > 0, "[FoundationPose] fp_pose_fit_eval: invalid arguments");
  FP_CHECK(N <= FP_MAX_BATCH, "[FoundationPose] fp_pose_fit_eval: " + std::to_string(N) + " poses, above the batch limit FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH));
  FP_CHECK(std::isfinite(tol_m) && tol_m > 0.0f, "[FoundationPose] fp_pose_fit_eval: tol_m must be finite and > 0 (metres)");
  FP_CHECK(std::isfinite(crop_ratio) && crop_ratio > 0.0f, "[FoundationPose] fp_pose_fit_eval: crop_ratio must be finite and > 0");
  FP_CHECK(!m->track_pending, "[FoundationPose] fp_pose_fit_eval: a submitted Track has not been waited for (fp_track_wait)");
  FP_CHECK(m->depth != nullptr, "[FoundationPose] fp_pose_fit_eval: no frame uploaded");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] unknown target_name");
  if (ensure_fit(m) || stage_frame(m) || upload_poses(m, t, poses, N)) return 1;
  const size_t half = (size_t)N * FP_NN_IN_IMG_HALFS;
  if (render_and_crop(m, t, N, crop_ratio, nn_mode(m), m->nn_in, m->nn_in + half, nullptr, nullptr)) return 1;
  const float tol_n = fit_tol_n(tol_m, t->mesh.diameter);
  PoseFitRec *recs_dev = m->fit_rec + FP_MAX_BATCH;   // (Register's records stay readable)
  if (enqueue_pose_fit(m, m->nn_in, m->nn_in + half, N, fit_tol_uniform(tol_n), recs_dev)) return 1;
  std::vector<PoseFitRec> recs((size_t)N);
  FP_HIP_OK(hipMemcpyAsync(recs.data(), recs_dev, recs.size() * sizeof(PoseFitRec), hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  for (int i = 0; i < N; i++) fit_record(out + i, recs[(size_t)i], tol_n, t->mesh.diameter);
  return 0;
} FP_CATCH_INT

// ---- frame-resolution rendering of one pose, and the host steps the stage operators of sections 4.8 - 4.13 share
// the shared stage scratch (fp_model::st_*) for this many vertices (snapped / camera-space), poses and work items; 0: not needed
static int grow_stage(fp_model *m, size_t snap, size_t cam, size_t poses, size_t items) {
  hipStream_t s = m->stream;
  return grow_scratch(s, m->st_snap, m->st_snap_cap, snap) || grow_scratch(s, m->st_cam, m->st_cam_cap, cam) ||
         grow_scratch(s, m->st_poses, m->st_pose_cap, poses) || grow_scratch(s, m->st_items, m->st_item_cap, items);
}

// An output plane of a frame-resolution render: the caller's pointer (null: not wanted) and its bytes per pixel.
struct RenderPlane {
  void *user;
  size_t bpp;
};
static bool planes_wanted(const RenderPlane *pl, int n) {
  for (int i = 0; i < n; i++) if (pl[i].user) return true;
  return false;
}
static size_t fr_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// dev[i] = where the kernel writes plane i (null: not wanted): the caller's own memory for FP_DEVICE; for FP_HOST a 256-byte-aligned
// place in the model's staging block, the wanted planes one after the other in the order given.  (The offsets are those of THIS
// frame size: a smaller frame than the block was sized for uses its front.)
static int place_planes(fp_model *m, const RenderPlane *pl, int n, size_t px, int memspace, uint8_t **dev) {
  size_t total = 0;
  for (int i = 0; i < n; i++) if (pl[i].user) total += fr_align(px * pl[i].bpp);
  if (memspace == FP_HOST && grow_scratch(m->stream, m->fr_out, m->fr_out_bytes, total)) return 1;
  uint8_t *at = m->fr_out;
  for (int i = 0; i < n; i++) {
    dev[i] = memspace == FP_HOST && pl[i].user ? at : static_cast<uint8_t *>(pl[i].user);
    if (pl[i].user) at += fr_align(px * pl[i].bpp);
  }
  return 0;
}
static int download_planes(fp_model *m, const RenderPlane *pl, int n, size_t px, uint8_t *const *dev) {
  for (int i = 0; i < n; i++)
    if (pl[i].user) FP_HIP_OK(hipMemcpyAsync(pl[i].user, dev[i], px * pl[i].bpp, hipMemcpyDeviceToHost, m->stream));
  return 0;
}

// (Two more shared steps are templates and stand above, next to grow_scratch, outside extern "C": rigid_parts and launch_item_runs.)
// What the stage operators ask of their arguments and of the model, each check written once.  A call makes them in its own order,
// between its own argument checks: the order decides which error a call with several faults reports.  fn: the call's name.
static int batch_size_ok(const std::string &fn, int N) {
  FP_CHECK(N >= 1 && N <= FP_MAX_BATCH, "[FoundationPose] " + fn + ": " + std::to_string(N) + " poses (1..FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH) + ")");
  return 0;
}
static int no_pending_track(const fp_model *m, const std::string &fn) {
  FP_CHECK(!m->track_pending, "[FoundationPose] " + fn + ": a submitted Track has not been waited for (fp_track_wait)");
  return 0;
}
// The frame-resolution calls read fx, fy, cx, cy only (frame_pose below), so they ask for a plain pinhole matrix: a skew or a third row
// that Register and Track would honour must not be dropped silently.  K is row-major, as fp_create took it.
static int pinhole_camera_ok(const fp_model *m, const std::string &fn) {
  static const int zero[4] = {1, 3, 6, 7};
  for (int k : zero)
    FP_CHECK(m->K[k] == 0.0f, "[FoundationPose] " + fn + ": the model's K is not a plain pinhole matrix: K[" + std::to_string(k) + "] = " + std::to_string(m->K[k]) +
                 " must be 0 (this call reads fx, fy, cx, cy only; Register and Track take a general K)");
  FP_CHECK(m->K[8] == 1.0f, "[FoundationPose] " + fn + ": the model's K is not a plain pinhole matrix: K[8] = " + std::to_string(m->K[8]) +
               " must be 1 (this call reads fx, fy, cx, cy only; Register and Track take a general K)");
  for (int k : {0, 4})
    FP_CHECK(std::isfinite(m->K[k]) && m->K[k] > 0.0f, "[FoundationPose] " + fn + ": the model's K is not a plain pinhole matrix: K[" + std::to_string(k) + "] = " +
                 std::to_string(m->K[k]) + " (the focal length) must be finite and positive");
  for (int k : {2, 5})
    FP_CHECK(std::isfinite(m->K[k]), "[FoundationPose] " + fn + ": the model's K is not a plain pinhole matrix: K[" + std::to_string(k) + "] (the principal point) must be finite");
  return 0;
}
static int stage_target(fp_model *m, const std::string &fn, const char *target_name, Target **t) {   // no pending Track, a pinhole K, then the target
  if (no_pending_track(m, fn) || pinhole_camera_ok(m, fn)) return 1;
  *t = m->find(target_name ? target_name : "");
  FP_CHECK(*t != nullptr, "[FoundationPose] unknown target_name");
  return 0;
}
static int frame_ready(const fp_model *m, const std::string &fn, bool with_rgb) {   // a whole frame is on the device
  FP_CHECK(m->depth != nullptr && (!with_rgb || m->rgb != nullptr) && m->H > 0, "[FoundationPose] " + fn + ": no frame uploaded");
  FP_CHECK(!m->frame_partial, "[FoundationPose] the last call (Track from a host frame) uploaded only its crop window: call fp_upload_frame first");
  return 0;
}
static bool matrix_finite(const float *p) {
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(p[k])) return false;
  return true;
}
static int matrices_finite_ok(const std::string &fn, const char *name, const float *mats, int n) {   // the n matrices of the argument `name`
  for (int i = 0; i < n; i++)
    FP_CHECK(matrix_finite(mats + (size_t)i * 16), "[FoundationPose] " + fn + ": a non-finite entry in " + name + "[" + std::to_string(i) + "]");
  return 0;
}
// what the two renderers ask of their arguments and of the model's frame, after their own argument checks
static int render_preconditions(const fp_model *m, const std::string &fn, int memspace, bool any_output, float tol_m) {
  FP_CHECK(memspace == FP_HOST || memspace == FP_DEVICE, "[FoundationPose] " + fn + ": memspace must be FP_HOST or FP_DEVICE");
  FP_CHECK(any_output, "[FoundationPose] " + fn + ": no output requested");
  FP_CHECK(std::isfinite(tol_m) && tol_m >= 0.0f, "[FoundationPose] " + fn + ": tol_m must be finite and >= 0 (metres)");
  return no_pending_track(m, fn) || pinhole_camera_ok(m, fn) || frame_ready(m, fn, true);
}
static FramePose frame_pose(const fp_model *m, const float pose[16]) {   // pose: column-major 4 x 4
  FramePose P;
  rigid_parts(pose, P.r, P.t);
  P.fx = m->K[0]; P.cx = m->K[2]; P.fy = m->K[4]; P.cy = m->K[5];
  return P;
}
// The (pose, tile) work of fp_pose_vsd and fp_refine_depth.  Tiles of a bound:
static bool bound_empty(const FrameTileBound &b) { return b.tx0 > b.tx1 || b.ty0 > b.ty1; }
static long long bound_tiles(const FrameTileBound &b) { return bound_empty(b) ? 0 : (long long)(b.tx1 - b.tx0 + 1) * (b.ty1 - b.ty0 + 1); }
static FrameTileBound bound_union(const FrameTileBound &a, const FrameTileBound &b) {
  if (bound_empty(a)) return b;
  if (bound_empty(b)) return a;
  return {std::min(a.tx0, b.tx0), std::min(a.ty0, b.ty0), std::max(a.tx1, b.tx1), std::max(a.ty1, b.ty1)};
}
// poses per chunk: as many as keep bytes_per_pose of vertex scratch each below the budget, one at least, N at most; forced > 0 (the
// test build's fpt_*_set_chunk) overrides the budget
static int stage_chunk(size_t bytes_per_pose, size_t budget, int N, int forced) {
  if (forced > 0) return std::min(forced, N);
  return (int)std::min<size_t>(std::max<size_t>(budget / bytes_per_pose, 1), (size_t)N);
}
// one item {local_pose, tile} per tile of the bound, in a grid of ntx tiles per row
static void append_tile_items(std::vector<int2> &items, int local_pose, const FrameTileBound &b, int ntx) {
  if (bound_empty(b)) return;
  for (int ty = b.ty0; ty <= b.ty1; ty++)
    for (int tx = b.tx0; tx <= b.tx1; tx++) items.push_back(make_int2(local_pose, ty * ntx + tx));
}
// the vertex pass's refusal word: a pose that needs a clipper, or leaves the exact integer range, gives an error, not a picture
static int pose_refused(int flag, const std::string &prefix) {
  FP_CHECK(!(flag & FRAME_RENDER_FLAG_NEAR), prefix + "a vertex lies nearer than FP_RENDER_NEAR_M (0.01 m) to the camera plane, or behind it (there is no clipper)");
  FP_CHECK(!(flag & FRAME_RENDER_FLAG_RANGE), prefix + "a vertex projects beyond FP_RENDER_SNAP_MAX sixteenths of a pixel (the exact range of the edge functions)");
  return 0;
}

int fp_render_pose(fp_model *m, const char *target_name, const float pose[16], float tol_m, const fp_frame_render *out, int memspace) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && pose && out, "[FoundationPose] fp_render_pose: invalid arguments");
  const RenderPlane pl[5] = {{out->model_depth, 4}, {out->tri_id, 4}, {out->overlay, 3}, {out->model_mask, 1}, {out->visible_mask, 1}};
  if (render_preconditions(m, "fp_render_pose", memspace, planes_wanted(pl, 5), tol_m)) return 1;
  Target *t = m->find(target_name ? target_name : "");
  FP_CHECK(t != nullptr, "[FoundationPose] unknown target_name");
  const DeviceMesh &mesh = t->mesh;
  const int H = m->H, W = m->W;
  const size_t px = (size_t)H * W;
  hipStream_t s = m->stream;
  if (grow_stage(m, (size_t)mesh.V, (size_t)mesh.V, 0, 0)) return 1;
  if (!m->fr_flag && dev_alloc(&m->fr_flag, 1)) return 1;
  const FramePose P = frame_pose(m, pose);
  // (a) vertex pass + the refusal word
  FP_HIP_OK(hipMemsetAsync(m->fr_flag, 0, sizeof(int), s));
  {
    ProfScope ps(&m->prof, s, "frame_vertex", 0, (double)mesh.V * (12.0 + 32.0));
    launch_frame_vertex(s, mesh, P, m->st_snap, m->st_cam, m->fr_flag);
    FP_HIP_OK(hipGetLastError());
  }
  int flag = 0;
  FP_HIP_OK(hipMemcpyAsync(&flag, m->fr_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  if (pose_refused(flag, "[FoundationPose] fp_render_pose: pose refused: ")) return 1;
  // (b) raster + resolve, straight into the caller's device memory or into the model's staging block
  uint8_t *dev[5];
  if (place_planes(m, pl, 5, px, memspace, dev)) return 1;
  const FrameRenderOut o = {reinterpret_cast<float *>(dev[0]), dev[3], dev[4], reinterpret_cast<int32_t *>(dev[1]), dev[2]};
  const FrameTileBound bound = frame_tile_bound(P, (double)mesh.max_norm, H, W);
  {
    const double wr = (o.depth ? 4.0 : 0.0) + (o.tri ? 4.0 : 0.0) + (o.overlay ? 3.0 : 0.0) + (o.mask ? 1.0 : 0.0) + (o.vis ? 1.0 : 0.0);
    const double rd = (o.overlay ? 3.0 : 0.0) + (o.vis || o.overlay ? 4.0 : 0.0);
    ProfScope ps(&m->prof, s, "frame_raster", 0, (double)px * (wr + rd));
    launch_frame_raster(s, mesh, m->st_snap, m->st_cam, m->rgb, m->depth, H, W, bound, tol_m, o);
    FP_HIP_OK(hipGetLastError());
  }
  if (memspace == FP_HOST && download_planes(m, pl, 5, px, dev)) return 1;
  FP_HIP_OK(hipStreamSynchronize(s));
  return 0;
} FP_CATCH_INT

// ---- all tracked objects of a frame at frame resolution
static_assert(FP_SCENE_MAX_OBJECTS == fp::SCENE_MAX_OBJECTS, "include/foundationpose_amd.h: the object limit of fp_render_scene is that of fp_internal.h");
static_assert(sizeof(fp_scene_object) == 32, "fp_scene_object: eight 32-bit words");
int fp_render_scene(fp_model *m, int K, const char *const *target_names, const float *poses, float tol_m, const fp_scene_render *out,
                    fp_scene_object *objects, int memspace) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(K >= 1 && K <= FP_SCENE_MAX_OBJECTS, "[FoundationPose] fp_render_scene: " + std::to_string(K) + " objects (1..FP_SCENE_MAX_OBJECTS = 64)");
  FP_CHECK(target_names && poses, "[FoundationPose] fp_render_scene: invalid arguments");
  static const fp_scene_render none = {};
  const fp_scene_render &want = out ? *out : none;
  const RenderPlane pl[6] = {{want.cover_bits, 8}, {want.model_depth, 4}, {want.tri_id, 4}, {want.overlay, 3}, {want.instance_id, 1}, {want.visible_mask, 1}};
  if (render_preconditions(m, "fp_render_scene", memspace, planes_wanted(pl, 6) || objects, tol_m)) return 1;
  if (!m->sc_table_host) m->sc_table_host = new SceneTable();
  SceneTable &tb = *m->sc_table_host;
  unsigned long long faces = 0, verts = 0;
  for (int o = 0; o < K; o++) {
    Target *t = m->find(target_names[o] ? target_names[o] : "");
    FP_CHECK(t != nullptr, "[FoundationPose] fp_render_scene: unknown target_name of object " + std::to_string(o));
    tb.pose[o] = frame_pose(m, poses + (size_t)o * 16);
    tb.verts[o] = t->mesh.verts;
    tb.faces[o] = t->mesh.faces;
    tb.vert_start[o] = (int)verts;
    tb.face_start[o] = (unsigned)faces;
    verts += (unsigned long long)t->mesh.V;
    faces += (unsigned long long)t->mesh.F;
    FP_CHECK(faces < 0xffffffffull, "[FoundationPose] fp_render_scene: the objects' face counts must sum to less than 2^32 - 1");
    FP_CHECK(verts <= 0x7fffffffull, "[FoundationPose] fp_render_scene: the objects' vertex counts must sum to at most 2^31 - 1");
  }
  for (int o = K; o <= SCENE_MAX_OBJECTS; o++) { tb.vert_start[o] = (int)verts; tb.face_start[o] = (unsigned)faces; }
  tb.K = K;
  const int H = m->H, W = m->W;
  const size_t px = (size_t)H * W;
  const int ntiles = scene_tiles_x(W) * scene_tiles_y(H);
  hipStream_t s = m->stream;
  if (!m->sc_table && dev_alloc(&m->sc_table, 1)) return 1;
  if (grow_stage(m, (size_t)verts, (size_t)verts, 0, 0) || grow_scratch(s, m->sc_work, m->sc_work_cap, scene_work_words(H, W))) return 1;
  int *flags = m->sc_work + SCENE_WORK_FLAGS, *counters = m->sc_work + SCENE_WORK_COUNTERS;
  unsigned long long *total_dev = reinterpret_cast<unsigned long long *>(m->sc_work + SCENE_WORK_TOTAL);
  unsigned *count = reinterpret_cast<unsigned *>(m->sc_work + SCENE_WORK_COUNT), *offset = count + ntiles, *cursor = offset + ntiles + 1;
  FP_HIP_OK(hipMemcpyAsync(m->sc_table, &tb, sizeof(SceneTable), hipMemcpyHostToDevice, s));
  FP_HIP_OK(hipMemsetAsync(m->sc_work, 0, ((size_t)SCENE_WORK_COUNT + ntiles) * sizeof(int), s));   // flags, total, counters, tile counts
  // (a) vertex pass, (b) binning: count + scan.  Then the call's one early read-back: the refusal words and the size of the lists.
  {
    ProfScope ps(&m->prof, s, "scene_vertex", 0, (double)verts * (12.0 + 32.0));
    launch_scene_vertex(s, m->sc_table, (int)verts, m->st_snap, m->st_cam, flags);
    FP_HIP_OK(hipGetLastError());
  }
  {
    ProfScope ps(&m->prof, s, "scene_bin", 0, (double)faces * (12.0 + 48.0));
    launch_scene_bin_count(s, m->sc_table, (unsigned)faces, m->st_snap, H, W, count, offset, cursor, total_dev);
    FP_HIP_OK(hipGetLastError());
  }
  int early[SCENE_WORK_TOTAL + 2] = {0};
  FP_HIP_OK(hipMemcpyAsync(early, m->sc_work, sizeof(early), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  for (int o = 0; o < K; o++)
    if (pose_refused(early[o], "[FoundationPose] fp_render_scene: pose refused: object " + std::to_string(o) + ": ")) return 1;
  unsigned long long entries = 0;
  std::memcpy(&entries, early + SCENE_WORK_TOTAL, sizeof(entries));
  FP_CHECK(entries <= (unsigned long long)SCENE_MAX_ENTRIES, "[FoundationPose] fp_render_scene: " + std::to_string(entries) +
               " (tile, triangle) pairs, above the limit of 2^31 - 1");
  if ((size_t)entries > m->sc_list_cap &&   // (half as much again, so that a scene that grows a little does not allocate every frame)
      grow_scratch(s, m->sc_list, m->sc_list_cap, (size_t)std::min<unsigned long long>(entries + entries / 2, (unsigned long long)SCENE_MAX_ENTRIES)))
    return 1;
  // (c) fill the lists, raster + resolve straight into the caller's device memory or into the model's staging block
  uint8_t *dev[6];
  if (place_planes(m, pl, 6, px, memspace, dev)) return 1;
  const SceneRenderOut o = {reinterpret_cast<float *>(dev[1]), dev[4], dev[5], reinterpret_cast<int32_t *>(dev[2]), reinterpret_cast<unsigned long long *>(dev[0]),
                            dev[3], objects ? counters : nullptr};
  {
    ProfScope ps(&m->prof, s, "scene_bin", 0, (double)faces * (12.0 + 48.0) + (double)entries * 4.0);
    launch_scene_bin_fill(s, m->sc_table, (unsigned)faces, m->st_snap, H, W, cursor, m->sc_list);
    FP_HIP_OK(hipGetLastError());
  }
  {
    const double wr = (o.depth ? 4.0 : 0.0) + (o.tri ? 4.0 : 0.0) + (o.cover ? 8.0 : 0.0) + (o.overlay ? 3.0 : 0.0) + (o.inst ? 1.0 : 0.0) + (o.vis ? 1.0 : 0.0);
    const double rd = (o.overlay ? 3.0 : 0.0) + (o.vis || o.overlay || o.counters ? 4.0 : 0.0);
    ProfScope ps(&m->prof, s, "scene_raster", 0, (double)px * (wr + rd) + (double)entries * 4.0);
    launch_scene_raster(s, m->sc_table, m->st_snap, m->st_cam, offset, m->sc_list, m->rgb, m->depth, H, W, tol_m, o);
    FP_HIP_OK(hipGetLastError());
  }
  if (memspace == FP_HOST && download_planes(m, pl, 6, px, dev)) return 1;
  int sums[SCENE_MAX_OBJECTS * 3] = {0};
  if (objects) FP_HIP_OK(hipMemcpyAsync(sums, counters, (size_t)K * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  if (objects) {
    for (int i = 0; i < K; i++) {
      fp_scene_object &r = objects[i];
      r = fp_scene_object{};
      r.n_covered = sums[i * 3]; r.n_front = sums[i * 3 + 1]; r.n_visible = sums[i * 3 + 2];
      r.n_hidden = r.n_covered - r.n_front;
      r.n_occluded = r.n_front - r.n_visible;
    }
  }
  return 0;
} FP_CATCH_INT

// ---- pose errors: ADD, ADD-S, MSSD, MSPD with object symmetries
namespace {
struct Rigid {   // host side, double: linear part ROW-major, then t
  double r[9], t[3];
};
Rigid rigid_from_colmajor(const float *p) {
  Rigid x;
  rigid_parts(p, x.r, x.t);
  return x;
}
Rigid rigid_mul(const Rigid &a, const Rigid &b) {   // a b
  Rigid x;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) x.r[r * 3 + c] = (a.r[r * 3] * b.r[c] + a.r[r * 3 + 1] * b.r[3 + c]) + a.r[r * 3 + 2] * b.r[6 + c];
    x.t[r] = ((a.r[r * 3] * b.t[0] + a.r[r * 3 + 1] * b.t[1]) + a.r[r * 3 + 2] * b.t[2]) + a.t[r];
  }
  return x;
}
Rigid rigid_inv_mul(const Rigid &a, const Rigid &b) {   // a^-1 b for a rigid a: (Ra^T Rb, Ra^T (tb - ta))
  Rigid x;
  const double d[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) x.r[r * 3 + c] = (a.r[r] * b.r[c] + a.r[3 + r] * b.r[3 + c]) + a.r[6 + r] * b.r[6 + c];
    x.t[r] = (a.r[r] * d[0] + a.r[3 + r] * d[1]) + a.r[6 + r] * d[2];
  }
  return x;
}
void rigid_to_f32(const Rigid &x, float *o) {
  for (int k = 0; k < 9; k++) o[k] = (float)x.r[k];
  for (int k = 0; k < 3; k++) o[9 + k] = (float)x.t[k];
}
// every entry finite, no translation component beyond +-1000 m
bool pose_error_matrix_ok(const float *p) {
  return matrix_finite(p) && std::fabs(p[12]) <= 1000.0f && std::fabs(p[13]) <= 1000.0f && std::fabs(p[14]) <= 1000.0f;
}
// the symmetries of a call in the CENTRED mesh's frame, the identity first: x' = R_s (x + c) + t_s - c, host, double (fp_pose_errors and
// fp_resolve_symmetry).  symmetries: S column-major 4 x 4 matrices of the mesh frame.
std::vector<Rigid> conjugated_symmetries(const DeviceMesh &mesh, const float *symmetries, int S) {
  std::vector<Rigid> sym((size_t)S + 1);
  sym[0] = Rigid{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  const double c[3] = {(double)mesh.center[0], (double)mesh.center[1], (double)mesh.center[2]};
  for (int s = 0; s < S; s++) {
    Rigid x = rigid_from_colmajor(symmetries + (size_t)s * 16);
    for (int r = 0; r < 3; r++) x.t[r] = (((x.r[r * 3] * c[0] + x.r[r * 3 + 1] * c[1]) + x.r[r * 3 + 2] * c[2]) + x.t[r]) - c[r];
    sym[(size_t)s + 1] = x;
  }
  return sym;
}
long long pose_error_vs(int V, long long step) { return ((long long)V + step - 1) / step; }
bool pose_error_adds_fits(int N, int V, long long step) {
  const unsigned __int128 vs = (unsigned __int128)pose_error_vs(V, step);
  return (unsigned __int128)N * vs * vs <= (unsigned __int128)FP_POSE_ERROR_MAX_PAIRS;
}
}  // namespace
static_assert(sizeof(fp_pose_error) == 56, "fp_pose_error: six floats, two 32-bit words, two 64-bit sums, two 32-bit words");
static_assert(FP_POSE_ERROR_MAX_PAIRS / 640 >= 1, "the launch shares of fp_pose_errors are whole numbers");
int fp_pose_errors(fp_model *m, const char *target_name, const float *est_poses, int N, const float *gt_poses, int n_gt,
                   const float *symmetries, int S, int vertex_step, int flags, fp_pose_error *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && est_poses && gt_poses && out, "[FoundationPose] fp_pose_errors: invalid arguments");
  if (batch_size_ok("fp_pose_errors", N)) return 1;
  FP_CHECK(n_gt == 1 || n_gt == N, "[FoundationPose] fp_pose_errors: n_gt must be 1 or N");
  FP_CHECK(S >= 0 && S <= FP_MAX_SYMMETRIES, "[FoundationPose] fp_pose_errors: " + std::to_string(S) + " symmetries (0..FP_MAX_SYMMETRIES = " + std::to_string(FP_MAX_SYMMETRIES) + ")");
  FP_CHECK(S == 0 || symmetries, "[FoundationPose] fp_pose_errors: invalid arguments (S > 0 without symmetries)");
  FP_CHECK(vertex_step >= 1, "[FoundationPose] fp_pose_errors: vertex_step must be >= 1");
  FP_CHECK(!(flags & ~FP_POSE_ERROR_ADDS), "[FoundationPose] fp_pose_errors: unknown flag bits");
  Target *t = nullptr;
  if (stage_target(m, "fp_pose_errors", target_name, &t)) return 1;
  const char *bad = "a non-finite entry or a translation beyond +-1000 m in ";
  for (int i = 0; i < N; i++)
    FP_CHECK(pose_error_matrix_ok(est_poses + (size_t)i * 16), std::string("[FoundationPose] fp_pose_errors: ") + bad + "est_poses[" + std::to_string(i) + "]");
  for (int i = 0; i < n_gt; i++)
    FP_CHECK(pose_error_matrix_ok(gt_poses + (size_t)i * 16), std::string("[FoundationPose] fp_pose_errors: ") + bad + "gt_poses[" + std::to_string(i) + "]");
  for (int i = 0; i < S; i++)
    FP_CHECK(pose_error_matrix_ok(symmetries + (size_t)i * 16), std::string("[FoundationPose] fp_pose_errors: ") + bad + "symmetries[" + std::to_string(i) + "]");
  const DeviceMesh &mesh = t->mesh;
  const bool adds = (flags & FP_POSE_ERROR_ADDS) != 0;
  const int S1 = S + 1;
  const int Vs = (int)pose_error_vs(mesh.V, vertex_step);
  if (adds && !pose_error_adds_fits(N, mesh.V, vertex_step)) {
    long long lo = vertex_step, hi = mesh.V;   // (hi: one vertex, N pairs, always fits)
    while (lo < hi) {
      const long long mid = lo + (hi - lo) / 2;
      if (pose_error_adds_fits(N, mesh.V, mid)) hi = mid;
      else lo = mid + 1;
    }
    FP_CHECK(false, "[FoundationPose] fp_pose_errors: ADD-S over " + std::to_string(N) + " poses x " + std::to_string(Vs) + "^2 point pairs is above FP_POSE_ERROR_MAX_PAIRS = " +
                        std::to_string((long long)FP_POSE_ERROR_MAX_PAIRS) + "; the smallest vertex_step that fits is " + std::to_string(lo));
  }
  const long long n_pairs = (long long)N * S1;
  FP_CHECK(n_pairs * Vs <= FP_POSE_ERROR_MAX_PAIRS / 64, "[FoundationPose] fp_pose_errors: " + std::to_string(N) + " poses x " + std::to_string(S1) + " symmetries x " +
               std::to_string(Vs) + " vertices is above FP_POSE_ERROR_MAX_PAIRS / 64 = " + std::to_string((long long)FP_POSE_ERROR_MAX_PAIRS / 64) + " transformed vertex pairs: raise vertex_step");
  // host, double: the conjugated symmetries x' = R_s (x + c) + t_s - c (identity first), the composites G S_s and D = E^-1 G
  const std::vector<Rigid> sym = conjugated_symmetries(mesh, symmetries, S);
  const size_t mat_floats = ((size_t)2 * N + (size_t)n_pairs) * 12;
  m->pe_mats_host.resize(mat_floats);
  float *est_h = m->pe_mats_host.data(), *rel_h = est_h + (size_t)N * 12, *comp_h = rel_h + (size_t)N * 12;
  for (int i = 0; i < N; i++) {
    const Rigid E = rigid_from_colmajor(est_poses + (size_t)i * 16), G = rigid_from_colmajor(gt_poses + (size_t)(n_gt == 1 ? 0 : i) * 16);
    rigid_to_f32(E, est_h + (size_t)i * 12);
    rigid_to_f32(rigid_inv_mul(E, G), rel_h + (size_t)i * 12);
    for (int s = 0; s < S1; s++) rigid_to_f32(rigid_mul(G, sym[(size_t)s]), comp_h + ((size_t)i * S1 + s) * 12);
  }
  hipStream_t st = m->stream;
  if (grow_scratch(st, m->pe_mats, m->pe_mat_cap, mat_floats) || grow_scratch(st, m->pe_pairs, m->pe_pair_cap, (size_t)n_pairs)) return 1;
  if (!m->pe_sums && dev_alloc(&m->pe_sums, (size_t)FP_MAX_BATCH)) return 1;
  const float *est_d = m->pe_mats, *rel_d = est_d + (size_t)N * 12, *comp_d = rel_d + (size_t)N * 12;
  FP_HIP_OK(hipMemcpyAsync(m->pe_mats, est_h, mat_floats * sizeof(float), hipMemcpyHostToDevice, st));
  {
    // no launch above a tenth of the cap: whole pairs (one workgroup each) per launch
    const long long per_launch = std::min<long long>(std::max<long long>(FP_POSE_ERROR_MAX_PAIRS / 640 / Vs, 1), 1 << 30);
    ProfScope ps(&m->prof, st, "pose_error_pairs", 0, (double)n_pairs * ((double)Vs * 12.0 + 72.0));
    for (long long p0 = 0; p0 < n_pairs; p0 += per_launch) {
      launch_pose_error_pairs(st, mesh.verts, Vs, vertex_step, m->K[0], m->K[4], m->K[2], m->K[5], est_d, comp_d, S1, p0,
                              (int)std::min(per_launch, n_pairs - p0), m->pe_pairs);
      FP_HIP_OK(hipGetLastError());
    }
  }
  if (adds) {
    FP_HIP_OK(hipMemsetAsync(m->pe_sums, 0, (size_t)N * sizeof(unsigned long long), st));
    const int per_launch = (int)std::min<long long>(std::max<long long>(FP_POSE_ERROR_MAX_PAIRS / 10 / ((long long)Vs * Vs), 1), N);
    ProfScope ps(&m->prof, st, "pose_error_nn", (double)N * Vs * Vs * 8.0, (double)N * Vs * 12.0);
    for (int p0 = 0; p0 < N; p0 += per_launch) {
      launch_pose_error_nn(st, mesh.verts, Vs, vertex_step, rel_d, p0, std::min(per_launch, N - p0), m->pe_sums);
      FP_HIP_OK(hipGetLastError());
    }
  }
  m->pe_pairs_host.resize((size_t)n_pairs);
  std::vector<unsigned long long> sums((size_t)N, 0);
  FP_HIP_OK(hipMemcpyAsync(m->pe_pairs_host.data(), m->pe_pairs, (size_t)n_pairs * sizeof(PoseErrPair), hipMemcpyDeviceToHost, st));
  if (adds) FP_HIP_OK(hipMemcpyAsync(sums.data(), m->pe_sums, (size_t)N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  FP_HIP_OK(hipStreamSynchronize(st));
  // the min over the symmetries (lowest index on ties) and the host-derived fields
  const auto as_float = [](unsigned bits) { float f; std::memcpy(&f, &bits, sizeof(f)); return f; };
  for (int i = 0; i < N; i++) {
    const PoseErrPair *pr = m->pe_pairs_host.data() + (size_t)i * S1;
    fp_pose_error r = {};
    int best = 0, best_px = 0, near = 0;
    for (int s = 0; s < S1; s++) {
      if (as_float(pr[s].max_d_bits) < as_float(pr[best].max_d_bits)) best = s;
      if (as_float(pr[s].max_px_bits) < as_float(pr[best_px].max_px_bits)) best_px = s;
      near |= pr[s].near;
    }
    r.add_sum_q20 = pr[0].sum_q20;
    r.add_m = (float)((double)pr[0].sum_q20 / 1048576.0 / (double)Vs);
    r.adds_sum_q20 = adds ? (int64_t)sums[(size_t)i] : -1;
    r.adds_m = adds ? (float)((double)sums[(size_t)i] / 1048576.0 / (double)Vs) : std::nanf("");
    r.mssd_m = as_float(pr[best].max_d_bits);
    r.best_sym = best;
    r.mspd_px = near ? INFINITY : as_float(pr[best_px].max_px_bits);
    r.best_sym_mspd = near ? -1 : best_px;
    const Rigid E = rigid_from_colmajor(est_poses + (size_t)i * 16);
    const Rigid GS = rigid_mul(rigid_from_colmajor(gt_poses + (size_t)(n_gt == 1 ? 0 : i) * 16), sym[(size_t)best]);
    const Rigid D = rigid_inv_mul(E, GS);
    // angle of E^T (G S): atan2 of the skew part's length and the trace term -- exactly 0 for equal matrices, accurate for small angles
    const double sx = (D.r[7] - D.r[5]) / 2, sy = (D.r[2] - D.r[6]) / 2, sz = (D.r[3] - D.r[1]) / 2;
    r.rot_deg = (float)(std::atan2(std::sqrt((sx * sx + sy * sy) + sz * sz), ((D.r[0] + D.r[4] + D.r[8]) - 1.0) / 2) * (180.0 / 3.14159265358979323846));
    const double dx = E.t[0] - GS.t[0], dy = E.t[1] - GS.t[1], dz = E.t[2] - GS.t[2];
    r.trans_m = (float)std::sqrt((dx * dx + dy * dy) + dz * dz);
    r.n_vertices = Vs;
    out[i] = r;
  }
  return 0;
} FP_CATCH_INT

// ---- visible surface discrepancy
static_assert(sizeof(fp_pose_vsd_t) == 160, "fp_pose_vsd: six counts, 16 counts, 16 floats, two 32-bit words");
static_assert(FP_VSD_MAX_TAUS == fp::VSD_MAX_TAUS && 6 + FP_VSD_MAX_TAUS <= fp::VSD_WORDS, "include/foundationpose_amd.h: the thresholds of fp_pose_vsd are those of fp_internal.h");
static_assert(FP_VSD_EST_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR && FP_VSD_EST_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE &&
              FP_VSD_GT_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR << 2 && FP_VSD_GT_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE << 2,
              "include/foundationpose_amd.h: the status bits of fp_pose_vsd are the refusal bits of the vertex rule");
int fp_pose_vsd(fp_model *m, const char *target_name, const float *est_poses, int N, const float *gt_poses, int n_gt, float delta_m,
                const float *taus, int T, int flags, fp_pose_vsd_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && est_poses && gt_poses && taus && out, "[FoundationPose] fp_pose_vsd: invalid arguments");
  if (batch_size_ok("fp_pose_vsd", N)) return 1;
  FP_CHECK(n_gt == 1 || n_gt == N, "[FoundationPose] fp_pose_vsd: n_gt must be 1 or N");
  FP_CHECK(T >= 1 && T <= FP_VSD_MAX_TAUS, "[FoundationPose] fp_pose_vsd: " + std::to_string(T) + " thresholds (1..FP_VSD_MAX_TAUS = " + std::to_string(FP_VSD_MAX_TAUS) + ")");
  FP_CHECK(std::isfinite(delta_m) && delta_m >= 0.0f, "[FoundationPose] fp_pose_vsd: delta_m must be finite and >= 0 (metres)");
  for (int t = 0; t < T; t++)
    FP_CHECK(std::isfinite(taus[t]) && taus[t] >= 0.0f, "[FoundationPose] fp_pose_vsd: taus[" + std::to_string(t) + "] must be finite and >= 0");
  FP_CHECK(!(flags & ~FP_VSD_NORMALIZED), "[FoundationPose] fp_pose_vsd: unknown flag bits");
  Target *t = nullptr;
  if (stage_target(m, "fp_pose_vsd", target_name, &t) || matrices_finite_ok("fp_pose_vsd", "est_poses", est_poses, N) ||
      matrices_finite_ok("fp_pose_vsd", "gt_poses", gt_poses, n_gt) || frame_ready(m, "fp_pose_vsd", false))
    return 1;
  const DeviceMesh &mesh = t->mesh;
  const int H = m->H, W = m->W, V = mesh.V;
  const int ntx = scene_tiles_x(W);
  const bool paired = n_gt == N && N > 1;   // (N == 1: the one truth goes through the plane like any n_gt == 1 call; same pixels)
  // host: the poses in the kernels' form, every pose's tiles, the work they stand for
  m->st_poses_host.resize((size_t)N + n_gt);
  FramePose *est_h = m->st_poses_host.data(), *gt_h = est_h + N;
  for (int i = 0; i < N; i++) est_h[i] = frame_pose(m, est_poses + (size_t)i * 16);
  for (int i = 0; i < n_gt; i++) gt_h[i] = frame_pose(m, gt_poses + (size_t)i * 16);
  std::vector<FrameTileBound> bounds((size_t)N);
  const FrameTileBound truth_bound = frame_tile_bound(gt_h[0], (double)mesh.max_norm, H, W);
  const long long walk = (long long)std::max(mesh.F, 1) * (paired ? 2 : 1);   // faces an item walks
  long long work = paired ? 0 : bound_tiles(truth_bound) * std::max(mesh.F, 1);
  for (int i = 0; i < N; i++) {
    const FrameTileBound g = paired ? frame_tile_bound(gt_h[i], (double)mesh.max_norm, H, W) : truth_bound;
    bounds[(size_t)i] = bound_union(frame_tile_bound(est_h[i], (double)mesh.max_norm, H, W), g);
    work += bound_tiles(bounds[(size_t)i]) * walk;
  }
  FP_CHECK(work <= FP_VSD_MAX_WORK, "[FoundationPose] fp_pose_vsd: " + std::to_string(N) + " poses of " + std::to_string(mesh.F) + " faces walk " + std::to_string(work) +
               " faces over their 32 x 32 px tiles, above FP_VSD_MAX_WORK = " + std::to_string((long long)FP_VSD_MAX_WORK) + ": pass fewer poses per call");
  VsdParams P;
  P.fx = m->K[0]; P.cx = m->K[2]; P.fy = m->K[4]; P.cy = m->K[5];
  P.delta = delta_m;
  P.T = T;
  for (int k = 0; k < VSD_MAX_TAUS; k++) P.thr[k] = k >= T ? 0.0f : (flags & FP_VSD_NORMALIZED) ? taus[k] * mesh.diameter : taus[k];
  // chunks of poses: the snapped vertices of a chunk (and of its truths) stay below VSD_SCRATCH_BYTES, one pose at least
  const int chunk = stage_chunk((size_t)std::max(V, 1) * sizeof(int4) * (paired ? 2 : 1), VSD_SCRATCH_BYTES, N, g_vsd_chunk);
  hipStream_t s = m->stream;
  const size_t n_words = (size_t)N * VSD_WORDS + N + n_gt;
  if (grow_stage(m, (size_t)V * ((size_t)chunk * (paired ? 2 : 1) + (paired ? 0 : 1)), 0, (size_t)N + n_gt, 0) ||
      grow_scratch(s, m->vsd_words, m->vsd_word_cap, n_words) || (!paired && grow_scratch(s, m->vsd_plane, m->vsd_plane_cap, (size_t)H * W)))
    return 1;
  int *counters = m->vsd_words, *flags_est = counters + (size_t)N * VSD_WORDS, *flags_gt = flags_est + N;
  const FramePose *est_d = m->st_poses, *gt_d = est_d + N;
  FP_HIP_OK(hipMemcpyAsync(m->st_poses, est_h, ((size_t)N + n_gt) * sizeof(FramePose), hipMemcpyHostToDevice, s));
  FP_HIP_OK(hipMemsetAsync(m->vsd_words, 0, n_words * sizeof(int), s));   // counters and refusal words together
  std::vector<int> words(n_words, 0);
  const int *flag_e = words.data() + (size_t)N * VSD_WORDS, *flag_g = flag_e + N;
  for (int p0 = 0; p0 < N; p0 += chunk) {
    const int c = std::min(chunk, N - p0);
    const int c_gt = paired ? c : p0 == 0 ? 1 : 0;   // the chunk's own truths, or the one truth with the first chunk
    int4 *snap_e = m->st_snap, *snap_g = snap_e + (size_t)c * V;
    {
      ProfScope ps(&m->prof, s, "vsd_vertex", 0, (double)(c + c_gt) * V * (12.0 + 16.0));
      launch_pose_vertices(s, "vsd_vertex", mesh, est_d + p0, c, paired ? gt_d + p0 : gt_d, c_gt, snap_e, nullptr, flags_est + p0, paired ? flags_gt + p0 : flags_gt);
      FP_HIP_OK(hipGetLastError());
    }
    // the refusal words of this chunk decide its work list (everything the stream held before is finished after this)
    FP_HIP_OK(hipMemcpyAsync(words.data() + (size_t)N * VSD_WORDS, flags_est, ((size_t)N + n_gt) * sizeof(int), hipMemcpyDeviceToHost, s));
    FP_HIP_OK(hipStreamSynchronize(s));
    if (!paired && p0 == 0) {
      if (pose_refused(flag_g[0], "[FoundationPose] fp_pose_vsd: ground truth refused: ")) return 1;
      // the one truth, once: fp_render_pose's own raster kernel writes its model depth over the whole frame
      ProfScope ps(&m->prof, s, "vsd_tile", 0, (double)H * W * 4.0);
      launch_frame_raster(s, mesh, snap_g, nullptr, nullptr, m->depth, H, W, truth_bound, 0.0f, FrameRenderOut{m->vsd_plane, nullptr, nullptr, nullptr, nullptr});
      FP_HIP_OK(hipGetLastError());
    }
    std::vector<int2> &items = m->st_items_host;
    items.clear();
    for (int l = 0; l < c; l++)
      if (!flag_e[p0 + l] && !(paired && flag_g[p0 + l])) append_tile_items(items, l, bounds[(size_t)(p0 + l)], ntx);
    if (items.empty()) continue;
    if (grow_stage(m, 0, 0, 0, items.size())) return 1;
    FP_HIP_OK(hipMemcpyAsync(m->st_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    ProfScope ps(&m->prof, s, "vsd_tile", 0, (double)items.size() * (double)walk * 60.0);
    if (launch_item_runs(0, items.size(), FP_VSD_MAX_WORK, walk, [&](size_t first, int cnt) {
          launch_vsd_tiles(s, mesh, snap_e, paired ? snap_g : nullptr, m->vsd_plane, m->st_items + first, cnt, m->depth, H, W, P, p0, counters);
          FP_HIP_OK(hipGetLastError());
          return 0;
        }))
      return 1;
  }
  FP_HIP_OK(hipMemcpyAsync(words.data(), counters, (size_t)N * VSD_WORDS * sizeof(int), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  std::vector<fp_pose_vsd_t> recs((size_t)N);
  for (int i = 0; i < N; i++) {
    fp_pose_vsd_t r = {};
    r.status = flag_e[i] | (paired ? flag_g[i] << 2 : 0);
    const int *w = words.data() + (size_t)i * VSD_WORDS;
    if (!r.status) {
      r.n_model_est = w[0]; r.n_model_gt = w[1]; r.n_visib_est = w[2]; r.n_visib_gt = w[3]; r.n_inter = w[4]; r.n_union = w[5];
      for (int k = 0; k < T; k++) r.n_fail[k] = w[6 + k];
    }
    for (int k = 0; k < FP_VSD_MAX_TAUS; k++)
      r.vsd[k] = k >= T ? std::nanf("") : r.n_union == 0 ? 1.0f : (float)(((double)r.n_fail[k] + (double)r.n_union - (double)r.n_inter) / (double)r.n_union);
    recs[(size_t)i] = r;
  }
  std::memcpy(out, recs.data(), recs.size() * sizeof(fp_pose_vsd_t));
  return 0;
} FP_CATCH_INT

// ---- depth refinement
namespace {
// cyclic Jacobi eigen-decomposition of the symmetric n x n matrix a (row-major, n <= 6; destroyed): eigenvalues w, eigenvectors the
// COLUMNS of v.  A rotation is skipped where the off-diagonal entry is exactly 0, so a block of zero rows and columns keeps its axes.
void jacobi_eigen(int n, double *a, double *w, double *v) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) v[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0, diag = 0;
    for (int i = 0; i < n; i++) {
      diag += a[i * n + i] * a[i * n + i];
      for (int j = i + 1; j < n; j++) off += a[i * n + j] * a[i * n + j];
    }
    if (off <= 1e-32 * diag) break;
    for (int p = 0; p < n; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * akq; a[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * aqk; a[q * n + k] = s * apk + c * aqk;
        }
        a[p * n + q] = a[q * n + p] = 0.0;
        for (int k = 0; k < n; k++) {
          const double vkp = v[k * n + p], vkq = v[k * n + q];
          v[k * n + p] = c * vkp - s * vkq; v[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < n; i++) w[i] = a[i * n + i];
}
// A xi = b from a record's integer sums, xi = (omega, upsilon / rad); only eigen-directions with lambda >= FP_ICP_RANK_EPS * lambda_max move
struct IcpSolve {
  double xi[6];
  int rank;
  double cond;
};
// (quantum: what one unit of a sum stands for, 2^32 for fp_refine_depth's records and 2^24 for fp_refine_silhouette's)
IcpSolve icp_solve(const int64_t *sums, double quantum, bool translation_only) {
  double A[36], b[6];
  int j = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) A[r * 6 + c] = A[c * 6 + r] = (double)sums[j++] / quantum;
  for (int r = 0; r < 6; r++) b[r] = (double)sums[21 + r] / quantum;
  const int n = translation_only ? 3 : 6, o = 6 - n;
  double a[36], w[6], v[36];
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) a[r * n + c] = A[(o + r) * 6 + (o + c)];
  jacobi_eigen(n, a, w, v);
  IcpSolve S = {};
  double lmax = w[0], lmin = w[0];
  for (int k = 1; k < n; k++) { lmax = std::max(lmax, w[k]); lmin = std::min(lmin, w[k]); }
  if (!(lmax > 0.0)) return S;
  S.cond = lmin / lmax;
  for (int k = 0; k < n; k++) {
    if (!(w[k] >= FP_ICP_RANK_EPS * lmax)) continue;
    double dot = 0;
    for (int r = 0; r < n; r++) dot += v[r * n + k] * b[o + r];
    for (int r = 0; r < n; r++) S.xi[o + r] += dot / w[k] * v[r * n + k];
    S.rank++;
  }
  return S;
}
// R <- exp(omega) R (Rodrigues), t <- t + upsilon; R row-major
void icp_apply(double *R, double *t, const double *omega, const double *upsilon) {
  const double x = omega[0], y = omega[1], z = omega[2];
  const double th2 = x * x + y * y + z * z, th = std::sqrt(th2);
  const double A = th < 1e-6 ? 1.0 - th2 / 6.0 : std::sin(th) / th, B = th < 1e-6 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
  const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  double E[9], out[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double k2 = 0;
      for (int k = 0; k < 3; k++) k2 += K[r * 3 + k] * K[k * 3 + c];
      E[r * 3 + c] = (r == c ? 1.0 : 0.0) + A * K[r * 3 + c] + B * k2;
    }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out[r * 3 + c] = (E[r * 3] * R[c] + E[r * 3 + 1] * R[3 + c]) + E[r * 3 + 2] * R[6 + c];
  if (th2 > 0.0)   // (exp(0) R is R itself, the sign of a zero entry included)
    for (int k = 0; k < 9; k++) R[k] = out[k];
  for (int k = 0; k < 3; k++)
    if (upsilon[k] != 0.0) t[k] += upsilon[k];
}
struct IcpState {
  double R[9], t[3], R_prev[9], t_prev[3];
  FramePose P, P_prev;   // the f32 form the device sees
  int state;             // 0 active, 1 one more evaluation (the record of a converged pose), 2 stopped
  fp_depth_refine_t rec;
};
void icp_round(IcpState &s) {
  for (int k = 0; k < 9; k++) s.P.r[k] = (float)s.R[k];
  for (int k = 0; k < 3; k++) s.P.t[k] = (float)s.t[k];
}
}  // namespace
static_assert(sizeof(fp_depth_refine_t) == 280, "fp_refine_depth: ten 32-bit words, four floats, 28 64-bit sums");
static_assert(FP_ICP_MIN_COS == fp::ICP_MIN_COS && fp::ICP_SUMS == 28 && fp::ICP_COUNTS == 6, "include/foundationpose_amd.h: the constants of fp_refine_depth are those of fp_internal.h");
static_assert(FP_ICP_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR << 2 && FP_ICP_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE << 2,
              "include/foundationpose_amd.h: the refusal bits of fp_refine_depth are the refusal bits of the vertex rule");
int fp_refine_depth(fp_model *m, const char *target_name, const float *poses, int N, int iterations, float max_dist_m, int flags, float *out_poses,
                    fp_depth_refine_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && out_poses && out, "[FoundationPose] fp_refine_depth: invalid arguments");
  if (batch_size_ok("fp_refine_depth", N)) return 1;
  FP_CHECK(iterations >= 0 && iterations <= FP_ICP_MAX_ITERATIONS,
           "[FoundationPose] fp_refine_depth: " + std::to_string(iterations) + " iterations (0..FP_ICP_MAX_ITERATIONS = " + std::to_string(FP_ICP_MAX_ITERATIONS) + ")");
  FP_CHECK(!(flags & ~FP_ICP_TRANSLATION_ONLY), "[FoundationPose] fp_refine_depth: unknown flag bits");
  Target *t = nullptr;
  if (stage_target(m, "fp_refine_depth", target_name, &t)) return 1;
  const DeviceMesh &mesh = t->mesh;
  FP_CHECK(std::isfinite(max_dist_m) && max_dist_m > 0.0f && max_dist_m <= mesh.diameter,
           "[FoundationPose] fp_refine_depth: max_dist_m must be finite, > 0 and at most the target's diameter (metres)");
  if (matrices_finite_ok("fp_refine_depth", "poses", poses, N) || frame_ready(m, "fp_refine_depth", false)) return 1;
  const int H = m->H, W = m->W, V = mesh.V;
  FP_CHECK((long long)H * W < (1ll << 26), "[FoundationPose] fp_refine_depth: a frame of 2^26 pixels or more (the 64-bit sums could overflow)");
  const int ntx = scene_tiles_x(W);
  const long long F = std::max(mesh.F, 1);
  std::vector<IcpState> st((size_t)N);
  long long work = 0;
  for (int i = 0; i < N; i++) {
    IcpState &s = st[(size_t)i];
    s.P = frame_pose(m, poses + (size_t)i * 16);
    for (int k = 0; k < 9; k++) s.R[k] = s.P.r[k];
    for (int k = 0; k < 3; k++) s.t[k] = s.P.t[k];
    s.state = 0;
    s.rec = fp_depth_refine_t{};
    work += bound_tiles(frame_tile_bound(s.P, (double)mesh.max_norm, H, W)) * F * (iterations + 1);
  }
  FP_CHECK(work <= FP_ICP_MAX_WORK, "[FoundationPose] fp_refine_depth: " + std::to_string(N) + " poses of " + std::to_string(mesh.F) + " faces walk " + std::to_string(work) +
               " faces over their 32 x 32 px tiles in " + std::to_string(iterations + 1) + " evaluations, above FP_ICP_MAX_WORK = " +
               std::to_string((long long)FP_ICP_MAX_WORK) + ": pass fewer poses or iterations per call");
  const float rad = mesh.diameter * 0.5f;
  // chunks of poses: the snapped and camera-space vertices of a chunk stay below ICP_SCRATCH_BYTES, one pose at least
  const int chunk = stage_chunk((size_t)std::max(V, 1) * (sizeof(int4) + sizeof(float4)), ICP_SCRATCH_BYTES, N, g_icp_chunk);
  hipStream_t s = m->stream;
  if (grow_stage(m, (size_t)V * chunk, (size_t)V * chunk, (size_t)N, 0) || grow_scratch(s, m->icp_params, m->icp_param_cap, (size_t)N) ||
      grow_scratch(s, m->icp_acc, m->icp_acc_cap, (size_t)N * ICP_WORDS + ((size_t)N + 1) / 2))
    return 1;
  std::vector<int> active;
  for (int pass = 0; pass <= iterations; pass++) {
    active.clear();
    for (int i = 0; i < N; i++)
      if (st[(size_t)i].state != 2) active.push_back(i);
    if (active.empty()) break;
    // ---- one evaluation of the active poses: vertex pass and tile kernel per chunk, one read-back, one synchronisation
    const int n = (int)active.size();
    const size_t acc_words = (size_t)n * ICP_WORDS + ((size_t)n + 1) / 2;
    m->st_poses_host.resize((size_t)n);
    m->icp_params_host.resize((size_t)n);
    m->icp_acc_host.assign(acc_words, 0ull);
    std::vector<int2> &items = m->st_items_host;
    items.clear();
    std::vector<size_t> chunk_end;   // items.size() after each chunk
    for (int a = 0; a < n; a++) {
      const IcpState &p = st[(size_t)active[(size_t)a]];
      m->st_poses_host[(size_t)a] = p.P;
      IcpParams q = {};
      q.fx = p.P.fx; q.fy = p.P.fy; q.cx = p.P.cx; q.cy = p.P.cy;
      q.max_dist = max_dist_m; q.rad = rad;
      for (int k = 0; k < 3; k++) q.t[k] = p.P.t[k];
      m->icp_params_host[(size_t)a] = q;
      append_tile_items(items, a % chunk, frame_tile_bound(p.P, (double)mesh.max_norm, H, W), ntx);
      if ((a + 1) % chunk == 0 || a + 1 == n) chunk_end.push_back(items.size());
    }
    if (grow_stage(m, 0, 0, 0, items.size())) return 1;
    unsigned long long *acc = m->icp_acc;
    int *flag_d = reinterpret_cast<int *>(acc + (size_t)n * ICP_WORDS);
    FP_HIP_OK(hipMemcpyAsync(m->st_poses, m->st_poses_host.data(), (size_t)n * sizeof(FramePose), hipMemcpyHostToDevice, s));
    FP_HIP_OK(hipMemcpyAsync(m->icp_params, m->icp_params_host.data(), (size_t)n * sizeof(IcpParams), hipMemcpyHostToDevice, s));
    if (!items.empty()) FP_HIP_OK(hipMemcpyAsync(m->st_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    FP_HIP_OK(hipMemsetAsync(acc, 0, acc_words * sizeof(unsigned long long), s));   // accumulators and refusal words together
    size_t first = 0;
    for (size_t c = 0; c < chunk_end.size(); c++) {
      const int a0 = (int)c * chunk, cn = std::min(chunk, n - a0);
      {
        ProfScope ps(&m->prof, s, "icp_vertex", 0, (double)cn * V * (12.0 + 32.0));
        launch_pose_vertices(s, "icp_vertex", mesh, m->st_poses + a0, cn, nullptr, 0, m->st_snap, m->st_cam, flag_d + a0, nullptr);
        FP_HIP_OK(hipGetLastError());
      }
      if (chunk_end[c] > first) {
        ProfScope ps(&m->prof, s, "icp_tile", 0, (double)(chunk_end[c] - first) * (double)F * 60.0);
        if (launch_item_runs(first, chunk_end[c], FP_ICP_MAX_WORK, F, [&](size_t at, int cnt) {
              launch_icp_tiles(s, mesh, m->st_snap, m->st_cam, m->st_items + at, cnt, m->depth, H, W, m->icp_params, flag_d, a0, acc);
              FP_HIP_OK(hipGetLastError());
              return 0;
            }))
          return 1;
        first = chunk_end[c];
      }
    }
    FP_HIP_OK(hipMemcpyAsync(m->icp_acc_host.data(), acc, acc_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    FP_HIP_OK(hipStreamSynchronize(s));
    const int *flag_h = reinterpret_cast<const int *>(m->icp_acc_host.data() + (size_t)n * ICP_WORDS);
    // ---- per pose: the record of this evaluation, then the update (or the reason to stop)
    for (int a = 0; a < n; a++) {
      IcpState &p = st[(size_t)active[(size_t)a]];
      fp_depth_refine_t &r = p.rec;
      if (flag_h[a]) {   // fp_render_pose would refuse: the input stays as it is, an updated pose goes back to what it was (and to that record)
        r.status |= flag_h[a] << 2;
        if (pass > 0) {
          std::memcpy(p.R, p.R_prev, sizeof(p.R)); std::memcpy(p.t, p.t_prev, sizeof(p.t));
          p.P = p.P_prev;
          r.iterations--;
        }
        p.state = 2;
        continue;
      }
      const unsigned long long *w = m->icp_acc_host.data() + (size_t)a * ICP_WORDS;
      for (int k = 0; k < ICP_SUMS; k++) r.sums_q32[k] = (int64_t)w[k];
      r.n_model = (int32_t)w[28]; r.n_valid = (int32_t)w[29]; r.n_used = (int32_t)w[30];
      r.n_front = (int32_t)w[31]; r.n_behind = (int32_t)w[32]; r.n_grazing = (int32_t)w[33];
      r.rms_m = r.n_used ? (float)(std::sqrt((double)r.sums_q32[27] / 4294967296.0 / (double)r.n_used) * (double)rad) : 0.0f;
      if (p.state == 1 || pass == iterations) { p.state = 2; continue; }
      if (r.n_used < FP_ICP_MIN_PIXELS) { r.status |= FP_ICP_TOO_FEW; p.state = 2; continue; }
      const IcpSolve S = icp_solve(r.sums_q32, 4294967296.0, (flags & FP_ICP_TRANSLATION_ONLY) != 0);
      const double ups[3] = {S.xi[3] * (double)rad, S.xi[4] * (double)rad, S.xi[5] * (double)rad};
      const double rot = std::sqrt(S.xi[0] * S.xi[0] + S.xi[1] * S.xi[1] + S.xi[2] * S.xi[2]);
      const double trans = std::sqrt(ups[0] * ups[0] + ups[1] * ups[1] + ups[2] * ups[2]);
      r.rank = S.rank; r.cond = (float)S.cond; r.last_rot_rad = (float)rot; r.last_trans_m = (float)trans;
      std::memcpy(p.R_prev, p.R, sizeof(p.R)); std::memcpy(p.t_prev, p.t, sizeof(p.t));
      p.P_prev = p.P;
      icp_apply(p.R, p.t, S.xi, ups);
      icp_round(p);
      r.iterations++;
      if (rot < (double)FP_ICP_EPS_ROT_RAD && trans < (double)FP_ICP_EPS_TRANS_M) {
        r.status |= FP_ICP_CONVERGED;
        p.state = std::memcmp(&p.P, &p.P_prev, sizeof(FramePose)) == 0 ? 2 : 1;   // the same f32 pose: the record is already that of the returned pose
      }
    }
  }
  for (int i = 0; i < N; i++) {
    const IcpState &p = st[(size_t)i];
    const float *in = poses + (size_t)i * 16;
    float *o = out_poses + (size_t)i * 16;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o[c * 4 + r] = p.P.r[r * 3 + c];
      o[12 + r] = p.P.t[r];
    }
    o[3] = in[3]; o[7] = in[7]; o[11] = in[11]; o[15] = in[15];
    out[i] = p.rec;
  }
  return 0;
} FP_CATCH_INT

// ---- depth search and the Register built on it
static_assert(sizeof(fp_pose_search_t) == sizeof(SearchRec) && sizeof(fp_pose_search_t) == 40, "fp_pose_search: a record is ten 32-bit words, the kernel's layout");
static_assert(FP_SEARCH_MAX_POINTS == fp::SEARCH_MAX_POINTS && FP_SEARCH_MAX_STEPS == fp::SEARCH_MAX_STEPS && FP_SEARCH_REFUSED_NEAR == fp::SEARCH_STATUS_REFUSED_NEAR,
              "include/foundationpose_amd.h: the constants of fp_pose_search are those of fp_internal.h");
static_assert(sizeof(fp_depth_register_t) == 336, "fp_register_depth: four 32-bit words, a search record, a refine record");
int fp_pose_search(fp_model *m, const char *target_name, const float *poses, int N, int n_steps, float step_m, float tol_m, int vertex_step,
                   fp_pose_search_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && out, "[FoundationPose] fp_pose_search: invalid arguments");
  if (batch_size_ok("fp_pose_search", N)) return 1;
  FP_CHECK(n_steps >= 1 && n_steps <= FP_SEARCH_MAX_STEPS,
           "[FoundationPose] fp_pose_search: " + std::to_string(n_steps) + " steps (1..FP_SEARCH_MAX_STEPS = " + std::to_string(FP_SEARCH_MAX_STEPS) + ")");
  FP_CHECK(std::isfinite(step_m) && step_m >= 0.0f, "[FoundationPose] fp_pose_search: step_m must be finite and >= 0 (metres)");
  FP_CHECK(std::isfinite(tol_m) && tol_m > 0.0f, "[FoundationPose] fp_pose_search: tol_m must be finite and > 0 (metres)");
  Target *t = nullptr;
  if (stage_target(m, "fp_pose_search", target_name, &t)) return 1;
  const DeviceMesh &mesh = t->mesh;
  const int V = mesh.V;
  const int fits = std::max((V + FP_SEARCH_MAX_POINTS - 1) / FP_SEARCH_MAX_POINTS, 1);   // the smallest step with P <= the cap
  FP_CHECK(vertex_step >= 1, "[FoundationPose] fp_pose_search: vertex_step must be >= 1");
  FP_CHECK(vertex_step >= fits, "[FoundationPose] fp_pose_search: vertex_step " + std::to_string(vertex_step) + " takes " +
               std::to_string((V + (long long)vertex_step - 1) / vertex_step) + " of the target's " + std::to_string(V) + " vertices, above FP_SEARCH_MAX_POINTS = " +
               std::to_string(FP_SEARCH_MAX_POINTS) + ": the smallest vertex_step that fits is " + std::to_string(fits));
  for (int i = 0; i < N; i++) {
    FP_CHECK(matrix_finite(poses + (size_t)i * 16), "[FoundationPose] fp_pose_search: a non-finite entry in poses[" + std::to_string(i) + "]");
    FP_CHECK(poses[(size_t)i * 16 + 14] >= FP_RENDER_NEAR_M, "[FoundationPose] fp_pose_search: poses[" + std::to_string(i) +
                 "] has its origin nearer than FP_RENDER_NEAR_M (0.01 m) to the camera plane, or behind it");
  }
  if (frame_ready(m, "fp_pose_search", false)) return 1;
  SearchParams S = {};
  S.H = m->H; S.W = m->W;
  S.P = (int)((V + (long long)vertex_step - 1) / vertex_step); S.vertex_step = vertex_step;
  S.n_steps = n_steps; S.step_m = step_m; S.tol_m = tol_m;
  hipStream_t s = m->stream;
  if (grow_stage(m, 0, 0, (size_t)N, 0) || grow_scratch(s, m->ps_recs, m->ps_rec_cap, (size_t)N)) return 1;
  m->st_poses_host.resize((size_t)N);
  m->ps_recs_host.resize((size_t)N);
  for (int i = 0; i < N; i++) m->st_poses_host[(size_t)i] = frame_pose(m, poses + (size_t)i * 16);
  FP_HIP_OK(hipMemcpyAsync(m->st_poses, m->st_poses_host.data(), (size_t)N * sizeof(FramePose), hipMemcpyHostToDevice, s));
  {
    ProfScope ps(&m->prof, s, "pose_search", 0, (double)N * S.P * (24.0 + 4.0 * n_steps));
    launch_pose_search(s, mesh, m->st_poses, N, m->depth, S, m->ps_recs);
    FP_HIP_OK(hipGetLastError());
  }
  FP_HIP_OK(hipMemcpyAsync(m->ps_recs_host.data(), m->ps_recs, (size_t)N * sizeof(SearchRec), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  std::memcpy(out, m->ps_recs_host.data(), (size_t)N * sizeof(SearchRec));
  return 0;
} FP_CATCH_INT

int fp_register_depth(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W, const char *target_name,
                      int top_k, float tol_m, int icp_iterations, float out_pose[16], fp_depth_register_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  RoctxRange range("fp_register_depth (sampler + depth search + ICP)");
  FP_CHECK(m && out_pose, "[FoundationPose] fp_register_depth: invalid arguments");
  FP_CHECK(top_k >= 0 && top_k <= FP_REGISTER_DEPTH_MAX_TOP_K,
           "[FoundationPose] fp_register_depth: top_k " + std::to_string(top_k) + " (0 = 16, at most " + std::to_string(FP_REGISTER_DEPTH_MAX_TOP_K) + ")");
  FP_CHECK(std::isfinite(tol_m) && tol_m >= 0.0f, "[FoundationPose] fp_register_depth: tol_m must be finite and >= 0 (metres; 0 = 0.005)");
  FP_CHECK(icp_iterations >= 0 && icp_iterations <= FP_ICP_MAX_ITERATIONS,
           "[FoundationPose] fp_register_depth: " + std::to_string(icp_iterations) + " iterations (0 = 15, at most FP_ICP_MAX_ITERATIONS = " + std::to_string(FP_ICP_MAX_ITERATIONS) + ")");
  if (no_pending_track(m, "fp_register_depth") || pinhole_camera_ok(m, "fp_register_depth")) return 1;
  if (top_k == 0) top_k = 16;
  if (tol_m == 0.0f) tol_m = 0.005f;
  if (icp_iterations == 0) icp_iterations = 15;
  Target *t = nullptr;
  if (check_frame_args(m, H, W, target_name ? target_name : "", &t)) return 1;
  FP_CHECK(mask != nullptr, "[FoundationPose] fp_register_depth needs a mask");
  // 1. the frame and the sampler's poses, as fp_upload_frame + fp_get_hyp_poses leave them
  const int N = m->n_hyp();
  if (upload_frame_async(m, rgb, depth, memspace, H, W)) return 1;
  if (sample_hypotheses_async(m, t, mask, memspace, 0, N)) { (void)hipStreamSynchronize(m->stream); return 1; }
  if (sampler_status(m)) return 1;
  std::vector<float> hyp((size_t)N * 16);
  FP_HIP_OK(hipMemcpyAsync(hyp.data(), m->poses_dev, (size_t)N * 64, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  // 2. the search
  const float diameter = t->mesh.diameter;
  const int n_steps = 9;
  const float step_m = diameter / 16.0f;
  const int vertex_step = std::max((t->mesh.V + 1023) / 1024, 1);
  std::vector<fp_pose_search_t> found((size_t)N);
  if (fp_pose_search(m, target_name, hyp.data(), N, n_steps, step_m, tol_m, vertex_step, found.data())) return 1;
  // 3. the candidates: by score, ties to the lower index; each at its best step
  std::vector<int> order;
  for (int i = 0; i < N; i++)
    if (found[(size_t)i].status == 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return found[(size_t)a].score > found[(size_t)b].score; });
  if ((int)order.size() > top_k) order.resize((size_t)top_k);
  FP_CHECK(!order.empty(), "[FoundationPose] fp_register_depth: no candidate: the search refused every hypothesis (the object would lie nearer than FP_RENDER_NEAR_M)");
  const int n_cand = (int)order.size();
  std::vector<float> cand((size_t)n_cand * 16), refined((size_t)n_cand * 16);
  for (int c = 0; c < n_cand; c++) {
    const float *src = hyp.data() + (size_t)order[(size_t)c] * 16;
    float *dst = cand.data() + (size_t)c * 16;
    std::memcpy(dst, src, 64);
    const float s_k = (float)found[(size_t)order[(size_t)c]].best_step * step_m;
    const float tx = src[12], ty = src[13], tz = src[14];
    dst[12] = tx + s_k * (tx / tz); dst[13] = ty + s_k * (ty / tz); dst[14] = tz + s_k;
  }
  // 4. the ICP
  const float gate = std::min(4.0f * tol_m, diameter);
  std::vector<fp_depth_refine_t> recs((size_t)n_cand);
  if (fp_refine_depth(m, target_name, cand.data(), n_cand, icp_iterations, gate, 0, refined.data(), recs.data())) return 1;
  // 5. the winner
  int win = -1;
  for (int c = 0; c < n_cand; c++) {
    const fp_depth_refine_t &r = recs[(size_t)c];
    if (r.status & (FP_ICP_REFUSED_NEAR | FP_ICP_REFUSED_RANGE | FP_ICP_TOO_FEW)) continue;
    if (win < 0) { win = c; continue; }
    const fp_depth_refine_t &w = recs[(size_t)win];
    const int key = r.n_used - r.n_behind, wkey = w.n_used - w.n_behind;
    if (key > wkey || (key == wkey && (r.sums_q32[27] < w.sums_q32[27] || (r.sums_q32[27] == w.sums_q32[27] && order[(size_t)c] < order[(size_t)win])))) win = c;
  }
  FP_CHECK(win >= 0, "[FoundationPose] fp_register_depth: no candidate is left: fp_refine_depth refused every one of the " + std::to_string(n_cand) +
               " candidates or found too few pixels of the object in the depth");
  std::memcpy(out_pose, refined.data() + (size_t)win * 16, 64);
  if (out) {
    out->hypothesis = order[(size_t)win];
    out->n_hypotheses = N; out->n_candidates = n_cand;
    out->rank_key = recs[(size_t)win].n_used - recs[(size_t)win].n_behind;
    out->search = found[(size_t)order[(size_t)win]];
    out->refine = recs[(size_t)win];
  }
  return 0;
} FP_CATCH_INT

// ---- colour agreement and symmetry resolution
static_assert(sizeof(fp_pose_color_t) == 152, "fp_pose_color: six 32-bit words, 15 64-bit sums, two floats");
static_assert(fp::COLOR_SUMS == 15 && fp::COLOR_COUNTS == 4, "include/foundationpose_amd.h: the sums of fp_pose_color are those of fp_internal.h");
static_assert(FP_COLOR_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR && FP_COLOR_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE,
              "include/foundationpose_amd.h: the refusal bits of fp_pose_color are the refusal bits of the vertex rule");
int fp_pose_color(fp_model *m, const char *target_name, const float *poses, int N, float tol_m, fp_pose_color_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && poses && out, "[FoundationPose] fp_pose_color: invalid arguments");
  if (batch_size_ok("fp_pose_color", N)) return 1;
  FP_CHECK(std::isfinite(tol_m) && tol_m >= 0.0f, "[FoundationPose] fp_pose_color: tol_m must be finite and >= 0 (metres)");
  Target *t = nullptr;
  if (stage_target(m, "fp_pose_color", target_name, &t) || matrices_finite_ok("fp_pose_color", "poses", poses, N) || frame_ready(m, "fp_pose_color", true))
    return 1;
  const DeviceMesh &mesh = t->mesh;
  const int H = m->H, W = m->W, V = mesh.V;
  FP_CHECK((long long)H * W < (1ll << 26), "[FoundationPose] fp_pose_color: a frame of 2^26 pixels or more (the sums are sized for fewer)");
  FP_CHECK(mesh.vcol || (mesh.tex && mesh.uvs && mesh.TH > 0 && mesh.TW > 0), "[FoundationPose] fp_pose_color: the target has neither a texture nor vertex colours");
  const int ntx = scene_tiles_x(W);
  const long long F = std::max(mesh.F, 1);
  // host: the poses in the kernels' form, every pose's tiles, the work they stand for (one evaluation, as fp_refine_depth counts it)
  m->st_poses_host.resize((size_t)N);
  std::vector<FrameTileBound> bounds((size_t)N);
  long long work = 0;
  for (int i = 0; i < N; i++) {
    m->st_poses_host[(size_t)i] = frame_pose(m, poses + (size_t)i * 16);
    bounds[(size_t)i] = frame_tile_bound(m->st_poses_host[(size_t)i], (double)mesh.max_norm, H, W);
    work += bound_tiles(bounds[(size_t)i]) * F;
  }
  FP_CHECK(work <= FP_COLOR_MAX_WORK, "[FoundationPose] fp_pose_color: " + std::to_string(N) + " poses of " + std::to_string(mesh.F) + " faces walk " + std::to_string(work) +
               " faces over their 32 x 32 px tiles, above FP_COLOR_MAX_WORK = " + std::to_string((long long)FP_COLOR_MAX_WORK) + ": pass fewer poses per call");
  // chunks of poses: the snapped vertices of a chunk stay below COLOR_SCRATCH_BYTES, one pose at least
  const int chunk = stage_chunk((size_t)std::max(V, 1) * sizeof(int4), COLOR_SCRATCH_BYTES, N, g_color_chunk);
  std::vector<int2> &items = m->st_items_host;
  items.clear();
  std::vector<size_t> chunk_end;   // items.size() after each chunk
  for (int i = 0; i < N; i++) {
    append_tile_items(items, i % chunk, bounds[(size_t)i], ntx);
    if ((i + 1) % chunk == 0 || i + 1 == N) chunk_end.push_back(items.size());
  }
  hipStream_t s = m->stream;
  const size_t acc_words = (size_t)N * COLOR_WORDS + ((size_t)N + 1) / 2;
  if (grow_stage(m, (size_t)V * chunk, 0, (size_t)N, items.size()) || grow_scratch(s, m->col_acc, m->col_acc_cap, acc_words)) return 1;
  unsigned long long *acc = m->col_acc;
  int *flag_d = reinterpret_cast<int *>(acc + (size_t)N * COLOR_WORDS);
  m->col_acc_host.assign(acc_words, 0ull);
  FP_HIP_OK(hipMemcpyAsync(m->st_poses, m->st_poses_host.data(), (size_t)N * sizeof(FramePose), hipMemcpyHostToDevice, s));
  if (!items.empty()) FP_HIP_OK(hipMemcpyAsync(m->st_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, s));
  FP_HIP_OK(hipMemsetAsync(acc, 0, acc_words * sizeof(unsigned long long), s));   // accumulators and refusal words together
  size_t first = 0;
  for (size_t c = 0; c < chunk_end.size(); c++) {
    const int p0 = (int)c * chunk, cn = std::min(chunk, N - p0);
    {
      ProfScope ps(&m->prof, s, "color_vertex", 0, (double)cn * V * (12.0 + 16.0));
      launch_pose_vertices(s, "color_vertex", mesh, m->st_poses + p0, cn, nullptr, 0, m->st_snap, nullptr, flag_d + p0, nullptr);
      FP_HIP_OK(hipGetLastError());
    }
    if (chunk_end[c] > first) {
      ProfScope ps(&m->prof, s, "color_tile", 0, (double)(chunk_end[c] - first) * (double)F * 60.0);
      if (launch_item_runs(first, chunk_end[c], FP_COLOR_MAX_WORK, F, [&](size_t at, int cnt) {
            launch_color_tiles(s, mesh, m->st_snap, m->st_items + at, cnt, m->rgb, m->depth, H, W, tol_m, flag_d, p0, acc);
            FP_HIP_OK(hipGetLastError());
            return 0;
          }))
        return 1;
      first = chunk_end[c];
    }
  }
  FP_HIP_OK(hipMemcpyAsync(m->col_acc_host.data(), acc, acc_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  const int *flag_h = reinterpret_cast<const int *>(m->col_acc_host.data() + (size_t)N * COLOR_WORDS);
  std::vector<fp_pose_color_t> recs((size_t)N);
  for (int i = 0; i < N; i++) {
    fp_pose_color_t r = {};
    r.status = flag_h[i];
    if (!r.status) {
      const unsigned long long *w = m->col_acc_host.data() + (size_t)i * COLOR_WORDS;
      for (int ch = 0; ch < 3; ch++) {
        r.sum_m[ch] = (int64_t)w[ch]; r.sum_o[ch] = (int64_t)w[3 + ch]; r.sum_mm[ch] = (int64_t)w[6 + ch];
        r.sum_oo[ch] = (int64_t)w[9 + ch]; r.sum_mo[ch] = (int64_t)w[12 + ch];
      }
      r.n_model = (int32_t)w[15]; r.n_visible = (int32_t)w[16]; r.n_compared = (int32_t)w[17]; r.n_nocolor = (int32_t)w[18];
      if (r.n_compared < FP_COLOR_MIN_PIXELS) r.status |= FP_COLOR_TOO_FEW;
      else {
        const double n = (double)r.n_compared;
        double cov = 0, var_m = 0, var_o = 0;
        for (int ch = 0; ch < 3; ch++) {
          const double sm = (double)r.sum_m[ch], so = (double)r.sum_o[ch];
          cov += (double)r.sum_mo[ch] - sm * so / n;
          var_m += (double)r.sum_mm[ch] - sm * sm / n;
          var_o += (double)r.sum_oo[ch] - so * so / n;
        }
        if (!(var_m > 0.0) || !(var_o > 0.0)) r.status |= FP_COLOR_FLAT;
        else r.zncc = (float)(cov / std::sqrt(var_m * var_o));
      }
    }
    recs[(size_t)i] = r;
  }
  std::memcpy(out, recs.data(), recs.size() * sizeof(fp_pose_color_t));
  return 0;
} FP_CATCH_INT

int fp_resolve_symmetry(fp_model *m, const char *target_name, const float pose[16], const float *symmetries, int S, float tol_m, float out_pose[16],
                        int *best_sym, fp_pose_color_t *records) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && pose && out_pose, "[FoundationPose] fp_resolve_symmetry: invalid arguments");
  FP_CHECK(S >= 0 && S <= FP_MAX_SYMMETRIES, "[FoundationPose] fp_resolve_symmetry: " + std::to_string(S) + " symmetries (0..FP_MAX_SYMMETRIES = " + std::to_string(FP_MAX_SYMMETRIES) + ")");
  FP_CHECK(S == 0 || symmetries, "[FoundationPose] fp_resolve_symmetry: invalid arguments (S > 0 without symmetries)");
  Target *t = nullptr;
  if (stage_target(m, "fp_resolve_symmetry", target_name, &t)) return 1;
  FP_CHECK(matrix_finite(pose), "[FoundationPose] fp_resolve_symmetry: a non-finite entry in pose");
  for (int i = 0; i < S; i++)
    FP_CHECK(pose_error_matrix_ok(symmetries + (size_t)i * 16),
             "[FoundationPose] fp_resolve_symmetry: a non-finite entry or a translation beyond +-1000 m in symmetries[" + std::to_string(i) + "]");
  // 1. the equivalents: host, double, rounded once; E_0 is the pose itself
  const std::vector<Rigid> sym = conjugated_symmetries(t->mesh, symmetries, S);
  const Rigid P = rigid_from_colmajor(pose);
  std::vector<float> eq(((size_t)S + 1) * 16);
  std::memcpy(eq.data(), pose, 64);
  for (int s = 1; s <= S; s++) {
    const Rigid E = rigid_mul(P, sym[(size_t)s]);
    float *o = eq.data() + (size_t)s * 16;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o[c * 4 + r] = (float)E.r[r * 3 + c];
      o[12 + r] = (float)E.t[r];
    }
    o[3] = pose[3]; o[7] = pose[7]; o[11] = pose[11]; o[15] = pose[15];
  }
  // 2. their records
  std::vector<fp_pose_color_t> recs((size_t)S + 1);
  if (fp_pose_color(m, target_name, eq.data(), S + 1, tol_m, recs.data())) return 1;
  // 3. the winner
  int win = -1;
  for (int s = 0; s <= S; s++)
    if (recs[(size_t)s].status == 0 && (win < 0 || recs[(size_t)s].zncc > recs[(size_t)win].zncc)) win = s;
  FP_CHECK(win >= 0, "[FoundationPose] fp_resolve_symmetry: no usable record: every one of the " + std::to_string(S + 1) +
               " equivalents is refused, shows fewer than FP_COLOR_MIN_PIXELS pixels or has no colour variance (an untextured model?)");
  std::memcpy(out_pose, eq.data() + (size_t)win * 16, 64);
  if (best_sym) *best_sym = win;
  if (records) std::memcpy(records, recs.data(), recs.size() * sizeof(fp_pose_color_t));
  return 0;
} FP_CATCH_INT

// ---- silhouette agreement
static_assert(sizeof(fp_pose_silhouette_t) == 64, "fp_pose_silhouette: eight 32-bit words, two 64-bit sums, four floats");
static_assert(FP_SIL_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR && FP_SIL_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE,
              "include/foundationpose_amd.h: the refusal bits of fp_pose_silhouette are the refusal bits of the vertex rule");
static_assert((long long)FP_SIL_MAX_TRUNC_PX * FP_SIL_MAX_TRUNC_PX < FP_SIL_D2_NONE && 2ll * (FP_SIL_MAX_DIM - 1) * (FP_SIL_MAX_DIM - 1) < FP_SIL_D2_NONE,
              "fp_pose_silhouette: a clip and every squared distance of a frame stay below FP_SIL_D2_NONE");
// what both calls ask of the mask and of the frame, after their own pointer checks
static int silhouette_frame_ok(const fp_model *m, const std::string &fn, int memspace) {
  FP_CHECK(memspace == FP_HOST || memspace == FP_DEVICE, "[FoundationPose] " + fn + ": memspace must be FP_HOST or FP_DEVICE");
  if (frame_ready(m, fn, false)) return 1;
  FP_CHECK(m->H <= FP_SIL_MAX_DIM && m->W <= FP_SIL_MAX_DIM, "[FoundationPose] " + fn + ": a frame of " + std::to_string(m->W) + " x " + std::to_string(m->H) +
               " pixels, above FP_SIL_MAX_DIM = " + std::to_string(FP_SIL_MAX_DIM) + " in a dimension");
  return 0;
}
// The distance transform of the call's mask on the model's stream: a host mask goes up by one stream-ordered copy, a device mask is read
// where it is; *mask_d is the mask the kernels read, m->sil_d2 [2, H, W] the two maps.  tot {n_mask, T} and any [2] are device words the
// caller has zeroed on the stream.
static int silhouette_maps(fp_model *m, const void *mask, int memspace, long long t2, unsigned long long *tot, int *any, const uint8_t **mask_d) {
  hipStream_t s = m->stream;
  const int H = m->H, W = m->W;
  const size_t px = (size_t)H * W;
  if (grow_scratch(s, m->sil_g, m->sil_g_cap, 2 * px) || grow_scratch(s, m->sil_d2, m->sil_d2_cap, 2 * px)) return 1;
  if (memspace == FP_HOST) {
    if (grow_scratch(s, m->sil_mask, m->sil_mask_cap, px)) return 1;
    FP_HIP_OK(hipMemcpyAsync(m->sil_mask, mask, px, hipMemcpyHostToDevice, s));
    *mask_d = m->sil_mask;
  } else {
    *mask_d = static_cast<const uint8_t *>(mask);
  }
  {
    ProfScope ps(&m->prof, s, "mask_edt_cols", 0, (double)px * (2.0 + 4.0 * 3.0));
    launch_mask_edt_cols(s, *mask_d, H, W, m->sil_g, any);
    FP_HIP_OK(hipGetLastError());
  }
  {
    ProfScope ps(&m->prof, s, "mask_edt_rows", 0, (double)px * (4.0 + 8.0));
    launch_mask_edt_rows(s, m->sil_g, any, H, W, m->sil_d2, t2, tot);
    FP_HIP_OK(hipGetLastError());
  }
  return 0;
}

int fp_mask_distance(fp_model *m, const void *mask, int memspace, uint32_t *d2_to_mask, uint32_t *d2_to_bg) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && mask && (d2_to_mask || d2_to_bg), "[FoundationPose] fp_mask_distance: invalid arguments");
  if (pinhole_camera_ok(m, "fp_mask_distance") || silhouette_frame_ok(m, "fp_mask_distance", memspace)) return 1;
  hipStream_t s = m->stream;
  const size_t px = (size_t)m->H * m->W;
  if (grow_scratch(s, m->sil_acc, m->sil_acc_cap, (size_t)3)) return 1;
  FP_HIP_OK(hipMemsetAsync(m->sil_acc, 0, 3 * sizeof(unsigned long long), s));
  const uint8_t *mask_d = nullptr;
  if (silhouette_maps(m, mask, memspace, 0, m->sil_acc, reinterpret_cast<int *>(m->sil_acc + 2), &mask_d)) return 1;
  if (d2_to_mask) FP_HIP_OK(hipMemcpyAsync(d2_to_mask, m->sil_d2, px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (d2_to_bg) FP_HIP_OK(hipMemcpyAsync(d2_to_bg, m->sil_d2 + px, px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  return 0;
} FP_CATCH_INT

int fp_pose_silhouette(fp_model *m, const char *target_name, const void *mask, int memspace, const float *poses, int N, float tol_m, int trunc_px,
                       int flags, fp_pose_silhouette_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && mask && poses && out, "[FoundationPose] fp_pose_silhouette: invalid arguments");
  if (batch_size_ok("fp_pose_silhouette", N)) return 1;
  FP_CHECK(std::isfinite(tol_m) && tol_m >= 0.0f, "[FoundationPose] fp_pose_silhouette: tol_m must be finite and >= 0 (metres)");
  FP_CHECK(trunc_px >= 0 && trunc_px <= FP_SIL_MAX_TRUNC_PX, "[FoundationPose] fp_pose_silhouette: trunc_px " + std::to_string(trunc_px) +
               " (0..FP_SIL_MAX_TRUNC_PX = " + std::to_string(FP_SIL_MAX_TRUNC_PX) + ")");
  FP_CHECK((flags & ~FP_SIL_AMODAL) == 0, "[FoundationPose] fp_pose_silhouette: unknown flag bits in " + std::to_string(flags));
  Target *t = nullptr;
  if (stage_target(m, "fp_pose_silhouette", target_name, &t) || matrices_finite_ok("fp_pose_silhouette", "poses", poses, N) ||
      silhouette_frame_ok(m, "fp_pose_silhouette", memspace))
    return 1;
  const DeviceMesh &mesh = t->mesh;
  const int H = m->H, W = m->W, V = mesh.V;
  const bool amodal = (flags & FP_SIL_AMODAL) != 0;
  const long long t2 = (long long)trunc_px * trunc_px;
  const int ntx = scene_tiles_x(W);
  const long long F = std::max(mesh.F, 1);
  // host: the poses in the kernels' form, every pose's tiles, the work they stand for (as fp_pose_color counts it)
  m->st_poses_host.resize((size_t)N);
  std::vector<FrameTileBound> bounds((size_t)N);
  long long work = 0;
  for (int i = 0; i < N; i++) {
    m->st_poses_host[(size_t)i] = frame_pose(m, poses + (size_t)i * 16);
    bounds[(size_t)i] = frame_tile_bound(m->st_poses_host[(size_t)i], (double)mesh.max_norm, H, W);
    work += bound_tiles(bounds[(size_t)i]) * F;
  }
  FP_CHECK(work <= FP_SIL_MAX_WORK, "[FoundationPose] fp_pose_silhouette: " + std::to_string(N) + " poses of " + std::to_string(mesh.F) + " faces walk " +
               std::to_string(work) + " faces over their 32 x 32 px tiles, above FP_SIL_MAX_WORK = " + std::to_string((long long)FP_SIL_MAX_WORK) +
               ": pass fewer poses per call");
  // chunks of poses: the snapped vertices of a chunk stay below SIL_SCRATCH_BYTES, one pose at least
  const int chunk = stage_chunk((size_t)std::max(V, 1) * sizeof(int4), SIL_SCRATCH_BYTES, N, g_sil_chunk);
  std::vector<int2> &items = m->st_items_host;
  items.clear();
  std::vector<size_t> chunk_end;   // items.size() after each chunk
  for (int i = 0; i < N; i++) {
    append_tile_items(items, i % chunk, bounds[(size_t)i], ntx);
    if ((i + 1) % chunk == 0 || i + 1 == N) chunk_end.push_back(items.size());
  }
  hipStream_t s = m->stream;
  const size_t acc_words = (size_t)2 + (size_t)N * SIL_WORDS + ((size_t)N + 3) / 2;
  if (grow_stage(m, (size_t)V * chunk, 0, (size_t)N, items.size()) || grow_scratch(s, m->sil_acc, m->sil_acc_cap, acc_words)) return 1;
  unsigned long long *tot = m->sil_acc, *acc = tot + 2;
  int *any_d = reinterpret_cast<int *>(acc + (size_t)N * SIL_WORDS), *flag_d = any_d + 2;
  m->sil_acc_host.assign(acc_words, 0ull);
  FP_HIP_OK(hipMemcpyAsync(m->st_poses, m->st_poses_host.data(), (size_t)N * sizeof(FramePose), hipMemcpyHostToDevice, s));
  if (!items.empty()) FP_HIP_OK(hipMemcpyAsync(m->st_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, s));
  FP_HIP_OK(hipMemsetAsync(tot, 0, acc_words * sizeof(unsigned long long), s));   // totals, accumulators, seed and refusal words together
  const uint8_t *mask_d = nullptr;
  if (silhouette_maps(m, mask, memspace, t2, tot, any_d, &mask_d)) return 1;
  size_t first = 0;
  for (size_t c = 0; c < chunk_end.size(); c++) {
    const int p0 = (int)c * chunk, cn = std::min(chunk, N - p0);
    {
      ProfScope ps(&m->prof, s, "silhouette_vertex", 0, (double)cn * V * (12.0 + 16.0));
      launch_pose_vertices(s, "silhouette_vertex", mesh, m->st_poses + p0, cn, nullptr, 0, m->st_snap, nullptr, flag_d + p0, nullptr);
      FP_HIP_OK(hipGetLastError());
    }
    if (chunk_end[c] > first) {
      ProfScope ps(&m->prof, s, "silhouette_tile", 0, (double)(chunk_end[c] - first) * (double)F * 60.0);
      if (launch_item_runs(first, chunk_end[c], FP_SIL_MAX_WORK, F, [&](size_t at, int cnt) {
            launch_silhouette_tiles(s, mesh, m->st_snap, m->st_items + at, cnt, m->depth, mask_d, m->sil_d2, H, W, tol_m, t2, amodal, flag_d, p0, acc);
            FP_HIP_OK(hipGetLastError());
            return 0;
          }))
        return 1;
      first = chunk_end[c];
    }
  }
  FP_HIP_OK(hipMemcpyAsync(m->sil_acc_host.data(), tot, acc_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  const unsigned long long *tot_h = m->sil_acc_host.data();
  const int *flag_h = reinterpret_cast<const int *>(tot_h + 2 + (size_t)N * SIL_WORDS) + 2;
  const int64_t n_mask = (int64_t)tot_h[0], T = (int64_t)tot_h[1];
  std::vector<fp_pose_silhouette_t> recs((size_t)N);
  for (int i = 0; i < N; i++) {
    fp_pose_silhouette_t r = {};
    r.status = flag_h[i];
    if (!r.status) {
      const unsigned long long *w = tot_h + 2 + (size_t)i * SIL_WORDS;
      r.n_model = (int32_t)w[0]; r.n_visible = (int32_t)w[1]; r.n_inter = (int32_t)w[2]; r.n_spill = (int32_t)w[3];
      r.n_mask = (int32_t)n_mask;
      r.n_miss = (int32_t)(n_mask - (int64_t)w[2]);
      r.sum_spill_d2 = (int64_t)w[4];
      r.sum_miss_d2 = T - (int64_t)w[5];
      const int64_t uni = n_mask + r.n_spill;
      if (uni == 0) r.status |= FP_SIL_EMPTY;
      else r.iou = (float)((double)r.n_inter / (double)uni);
      if (r.n_spill) r.rms_spill_px = (float)std::sqrt((double)r.sum_spill_d2 / (double)r.n_spill);
      if (r.n_miss) r.rms_miss_px = (float)std::sqrt((double)r.sum_miss_d2 / (double)r.n_miss);
    }
    recs[(size_t)i] = r;
  }
  std::memcpy(out, recs.data(), recs.size() * sizeof(fp_pose_silhouette_t));
  return 0;
} FP_CATCH_INT

// ---- silhouette refinement
namespace {
struct SilrefState {
  double R[9], t[3], R_prev[9], t_prev[3];
  FramePose P, P_prev;   // the f32 form the device sees
  int state;             // 0 active, 1 one more evaluation (the record of a converged pose), 2 stopped
  fp_silhouette_refine_t rec;
};
// the per-pose constants of section 4.16 in f32, each operation separately rounded (this file is compiled without contraction)
SilrefParams silref_params_of(const FramePose &P, float rad) {
  SilrefParams q = {};
  q.fx = P.fx; q.fy = P.fy; q.cx = P.cx; q.cy = P.cy;
  q.rad = rad;
  for (int k = 0; k < 3; k++) q.t[k] = P.t[k];
  const float fr = P.fx * rad, gr = P.fy * rad;
  q.s = fr / P.t[2];
  q.kx = fr / q.s; q.ky = gr / q.s;
  return q;
}
}  // namespace
static_assert(sizeof(fp_silhouette_refine_t) == 288, "fp_refine_silhouette: ten 32-bit words, six floats, 28 64-bit sums");
static_assert(FP_SILREF_MAX_TERM == fp::SILREF_MAX_TERM && fp::SILREF_SUMS == 28 && fp::SILREF_COUNTS == 7,
              "include/foundationpose_amd.h: the constants of fp_refine_silhouette are those of fp_internal.h");
static_assert(FP_SILREF_REFUSED_NEAR == FRAME_RENDER_FLAG_NEAR << 2 && FP_SILREF_REFUSED_RANGE == FRAME_RENDER_FLAG_RANGE << 2 &&
                  FP_SILREF_CONVERGED == FP_ICP_CONVERGED && FP_SILREF_TOO_FEW == FP_ICP_TOO_FEW,
              "include/foundationpose_amd.h: the status bits of fp_refine_silhouette are fp_refine_depth's");
int fp_refine_silhouette(fp_model *m, const char *target_name, const void *mask, int memspace, const float *poses, int N, int iterations, int gate_px,
                         float tol_m, int flags, float *out_poses, fp_silhouette_refine_t *out) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m && mask && poses && out_poses && out, "[FoundationPose] fp_refine_silhouette: invalid arguments");
  if (batch_size_ok("fp_refine_silhouette", N)) return 1;
  FP_CHECK(iterations >= 0 && iterations <= FP_SILREF_MAX_ITERATIONS, "[FoundationPose] fp_refine_silhouette: " + std::to_string(iterations) +
               " iterations (0..FP_SILREF_MAX_ITERATIONS = " + std::to_string(FP_SILREF_MAX_ITERATIONS) + ")");
  FP_CHECK(std::isfinite(tol_m) && tol_m >= 0.0f, "[FoundationPose] fp_refine_silhouette: tol_m must be finite and >= 0 (metres)");
  FP_CHECK(gate_px >= 0 && gate_px <= FP_SIL_MAX_TRUNC_PX, "[FoundationPose] fp_refine_silhouette: gate_px " + std::to_string(gate_px) +
               " (0..FP_SIL_MAX_TRUNC_PX = " + std::to_string(FP_SIL_MAX_TRUNC_PX) + ")");
  FP_CHECK((flags & ~(FP_SILREF_TRANSLATION_ONLY | FP_SILREF_OCCLUSION)) == 0, "[FoundationPose] fp_refine_silhouette: unknown flag bits in " + std::to_string(flags));
  Target *t = nullptr;
  if (stage_target(m, "fp_refine_silhouette", target_name, &t) || matrices_finite_ok("fp_refine_silhouette", "poses", poses, N) ||
      silhouette_frame_ok(m, "fp_refine_silhouette", memspace))
    return 1;
  const DeviceMesh &mesh = t->mesh;
  const int H = m->H, W = m->W, V = mesh.V;
  const bool occlusion = (flags & FP_SILREF_OCCLUSION) != 0;
  const int gate2 = gate_px * gate_px;
  const int ntx = scene_tiles_x(W);
  const long long F = std::max(mesh.F, 1);
  std::vector<SilrefState> st((size_t)N);
  long long work = 0;
  for (int i = 0; i < N; i++) {
    SilrefState &s = st[(size_t)i];
    s.P = frame_pose(m, poses + (size_t)i * 16);
    for (int k = 0; k < 9; k++) s.R[k] = s.P.r[k];
    for (int k = 0; k < 3; k++) s.t[k] = s.P.t[k];
    s.state = 0;
    s.rec = fp_silhouette_refine_t{};
    work += bound_tiles(frame_tile_bound(s.P, (double)mesh.max_norm, H, W)) * F * (iterations + 1);
  }
  FP_CHECK(work <= FP_SILREF_MAX_WORK, "[FoundationPose] fp_refine_silhouette: " + std::to_string(N) + " poses of " + std::to_string(mesh.F) + " faces walk " +
               std::to_string(work) + " faces over their 32 x 32 px tiles in " + std::to_string(iterations + 1) + " evaluations, above FP_SILREF_MAX_WORK = " +
               std::to_string((long long)FP_SILREF_MAX_WORK) + ": pass fewer poses or iterations per call");
  const float rad = mesh.diameter * 0.5f;
  // chunks of poses: the snapped vertices of a chunk stay below SIL_SCRATCH_BYTES, one pose at least
  const int chunk = stage_chunk((size_t)std::max(V, 1) * sizeof(int4), SIL_SCRATCH_BYTES, N, g_silref_chunk);
  hipStream_t s = m->stream;
  // the accumulator block: {n_mask, T} | the two seed words | per pass the accumulators [n, SILREF_WORDS] and the refusal words [n]
  constexpr size_t HEAD = 3;
  if (grow_stage(m, (size_t)V * chunk, 0, (size_t)N, 0) || grow_scratch(s, m->silref_params, m->silref_param_cap, (size_t)N) ||
      grow_scratch(s, m->silref_acc, m->silref_acc_cap, HEAD + (size_t)N * SILREF_WORDS + ((size_t)N + 1) / 2) ||
      grow_scratch(s, m->silref_sd, m->silref_sd_cap, (size_t)H * W))
    return 1;
  // ---- once per call: the distance transform of the mask and the signed map.  Whether the mask has both sides comes back with the
  // first evaluation's read-back (the seed words), so the call keeps to one synchronisation per evaluation.
  FP_HIP_OK(hipMemsetAsync(m->silref_acc, 0, HEAD * sizeof(unsigned long long), s));
  const uint8_t *mask_d = nullptr;
  if (silhouette_maps(m, mask, memspace, 0, m->silref_acc, reinterpret_cast<int *>(m->silref_acc + 2), &mask_d)) return 1;
  {
    ProfScope ps(&m->prof, s, "mask_signed_d2", 0, (double)H * W * (1.0 + 8.0 + 4.0));
    launch_mask_signed_d2(s, mask_d, m->sil_d2, H, W, m->silref_sd);
    FP_HIP_OK(hipGetLastError());
  }
  std::vector<int> active;
  for (int pass = 0; pass <= iterations; pass++) {
    active.clear();
    for (int i = 0; i < N; i++)
      if (st[(size_t)i].state != 2) active.push_back(i);
    if (active.empty()) break;
    // ---- one evaluation of the active poses: vertex pass and tile kernel per chunk, one read-back, one synchronisation
    const int n = (int)active.size();
    const size_t acc_words = HEAD + (size_t)n * SILREF_WORDS + ((size_t)n + 1) / 2;
    m->st_poses_host.resize((size_t)n);
    m->silref_params_host.resize((size_t)n);
    m->silref_acc_host.assign(acc_words, 0ull);
    std::vector<int2> &items = m->st_items_host;
    items.clear();
    std::vector<size_t> chunk_end;   // items.size() after each chunk
    for (int a = 0; a < n; a++) {
      const SilrefState &p = st[(size_t)active[(size_t)a]];
      m->st_poses_host[(size_t)a] = p.P;
      m->silref_params_host[(size_t)a] = silref_params_of(p.P, rad);
      // (a pose whose origin is nearer than the near constant has no scale: refused below, its tiles are not walked)
      if (p.P.t[2] >= FRAME_RENDER_NEAR) append_tile_items(items, a % chunk, frame_tile_bound(p.P, (double)mesh.max_norm, H, W), ntx);
      if ((a + 1) % chunk == 0 || a + 1 == n) chunk_end.push_back(items.size());
    }
    if (grow_stage(m, 0, 0, 0, items.size())) return 1;
    unsigned long long *acc = m->silref_acc + HEAD;
    int *flag_d = reinterpret_cast<int *>(acc + (size_t)n * SILREF_WORDS);
    FP_HIP_OK(hipMemcpyAsync(m->st_poses, m->st_poses_host.data(), (size_t)n * sizeof(FramePose), hipMemcpyHostToDevice, s));
    FP_HIP_OK(hipMemcpyAsync(m->silref_params, m->silref_params_host.data(), (size_t)n * sizeof(SilrefParams), hipMemcpyHostToDevice, s));
    if (!items.empty()) FP_HIP_OK(hipMemcpyAsync(m->st_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    FP_HIP_OK(hipMemsetAsync(acc, 0, (acc_words - HEAD) * sizeof(unsigned long long), s));   // accumulators and refusal words together
    size_t first = 0;
    for (size_t c = 0; c < chunk_end.size(); c++) {
      const int a0 = (int)c * chunk, cn = std::min(chunk, n - a0);
      {
        ProfScope ps(&m->prof, s, "silref_vertex", 0, (double)cn * V * (12.0 + 16.0));
        launch_pose_vertices(s, "silref_vertex", mesh, m->st_poses + a0, cn, nullptr, 0, m->st_snap, nullptr, flag_d + a0, nullptr);
        FP_HIP_OK(hipGetLastError());
      }
      if (chunk_end[c] > first) {
        ProfScope ps(&m->prof, s, "silref_tile", 0, (double)(chunk_end[c] - first) * (double)F * 60.0);
        if (launch_item_runs(first, chunk_end[c], FP_SILREF_MAX_WORK, F, [&](size_t at, int cnt) {
              launch_silref_tiles(s, mesh, m->st_snap, m->st_items + at, cnt, m->depth, m->silref_sd, H, W, gate2, tol_m, occlusion, m->silref_params, flag_d,
                                  a0, acc);
              FP_HIP_OK(hipGetLastError());
              return 0;
            }))
          return 1;
        first = chunk_end[c];
      }
    }
    FP_HIP_OK(hipMemcpyAsync(m->silref_acc_host.data(), m->silref_acc, acc_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    FP_HIP_OK(hipStreamSynchronize(s));
    if (pass == 0) {
      const int *any_h = reinterpret_cast<const int *>(m->silref_acc_host.data() + 2);
      FP_CHECK(any_h[0] != 0, "[FoundationPose] fp_refine_silhouette: the mask is empty (no pixel has a byte > 0): it has no outline");
      FP_CHECK(any_h[1] != 0, "[FoundationPose] fp_refine_silhouette: the mask covers the whole frame: it has no outline");
    }
    const unsigned long long *acc_h = m->silref_acc_host.data() + HEAD;
    const int *flag_h = reinterpret_cast<const int *>(acc_h + (size_t)n * SILREF_WORDS);
    // ---- per pose: the record of this evaluation, then the update (or the reason to stop)
    for (int a = 0; a < n; a++) {
      SilrefState &p = st[(size_t)active[(size_t)a]];
      fp_silhouette_refine_t &r = p.rec;
      const int refused = flag_h[a] | (p.P.t[2] >= FRAME_RENDER_NEAR ? 0 : FRAME_RENDER_FLAG_NEAR);
      if (refused) {   // fp_render_pose would refuse: the input stays as it is, an updated pose goes back to what it was (and to that record)
        r.status |= refused << 2;
        if (pass > 0) {
          std::memcpy(p.R, p.R_prev, sizeof(p.R)); std::memcpy(p.t, p.t_prev, sizeof(p.t));
          p.P = p.P_prev;
          r.iterations--;
        }
        p.state = 2;
        continue;
      }
      const unsigned long long *w = acc_h + (size_t)a * SILREF_WORDS;
      const SilrefParams &q = m->silref_params_host[(size_t)a];
      for (int k = 0; k < SILREF_SUMS; k++) r.sums_q24[k] = (int64_t)w[k];
      r.n_model = (int32_t)w[28]; r.n_contour = (int32_t)w[29]; r.n_used = (int32_t)w[30]; r.n_occluded = (int32_t)w[31];
      r.n_far = (int32_t)w[32]; r.n_flat = (int32_t)w[33]; r.n_steep = (int32_t)w[34];
      r.scale_px = q.s;
      r.rms_px = r.n_used ? (float)(std::sqrt((double)r.sums_q24[27] / 16777216.0 / (double)r.n_used) * (double)q.s) : 0.0f;
      if (p.state == 1 || pass == iterations) { p.state = 2; continue; }
      if (r.n_used < FP_SILREF_MIN_PIXELS) { r.status |= FP_SILREF_TOO_FEW; p.state = 2; continue; }
      IcpSolve S = icp_solve(r.sums_q24, 16777216.0, (flags & FP_SILREF_TRANSLATION_ONLY) != 0);
      const double rot = std::sqrt(S.xi[0] * S.xi[0] + S.xi[1] * S.xi[1] + S.xi[2] * S.xi[2]);
      const double radii = std::sqrt(S.xi[3] * S.xi[3] + S.xi[4] * S.xi[4] + S.xi[5] * S.xi[5]);
      const double trans = radii * (double)rad;
      // the step cap: the whole twist is scaled, so its direction stays the solve's
      double scale = 1.0;
      if (rot > FP_SILREF_MAX_STEP_RAD) scale = std::min(scale, FP_SILREF_MAX_STEP_RAD / rot);
      if (radii > FP_SILREF_MAX_STEP_RADII) scale = std::min(scale, FP_SILREF_MAX_STEP_RADII / radii);
      if (scale < 1.0)
        for (int k = 0; k < 6; k++) S.xi[k] *= scale;
      const double ups[3] = {S.xi[3] * (double)rad, S.xi[4] * (double)rad, S.xi[5] * (double)rad};
      r.rank = S.rank; r.cond = (float)S.cond; r.last_rot_rad = (float)(rot * scale); r.last_trans_m = (float)(trans * scale);
      std::memcpy(p.R_prev, p.R, sizeof(p.R)); std::memcpy(p.t_prev, p.t, sizeof(p.t));
      p.P_prev = p.P;
      icp_apply(p.R, p.t, S.xi, ups);
      for (int k = 0; k < 9; k++) p.P.r[k] = (float)p.R[k];
      for (int k = 0; k < 3; k++) p.P.t[k] = (float)p.t[k];
      r.iterations++;
      if (rot < (double)FP_SILREF_EPS_ROT_RAD && trans < (double)FP_SILREF_EPS_TRANS_M) {
        r.status |= FP_SILREF_CONVERGED;
        p.state = std::memcmp(&p.P, &p.P_prev, sizeof(FramePose)) == 0 ? 2 : 1;   // the same f32 pose: the record is already that of the returned pose
      }
    }
  }
  for (int i = 0; i < N; i++) {
    const SilrefState &p = st[(size_t)i];
    const float *in = poses + (size_t)i * 16;
    float *o = out_poses + (size_t)i * 16;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o[c * 4 + r] = p.P.r[r * 3 + c];
      o[12 + r] = p.P.t[r];
    }
    o[3] = in[3]; o[7] = in[7]; o[11] = in[11]; o[15] = in[15];
    out[i] = p.rec;
  }
  return 0;
} FP_CATCH_INT

int fp_set_precision(fp_model *m, int precision) try {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(precision == PREC_F16 || precision == PREC_BF16 || precision == PREC_FP8 || precision == PREC_INT8, "[FoundationPose] unknown precision");
  // (checked BEFORE anything is prepared: an uncalibrated 8-bit precision must not cost 0.3-1 s of host work, an exclusive section and
  // two resident networks just to be refused.  m->calibrated only changes under the exclusive lock, which a racing calibration of the
  // same model would be a caller error anyway: models are not re-entrant)
  FP_CHECK(!(precision == PREC_FP8 || precision == PREC_INT8) || m->calibrated(precision),
           "[FoundationPose] an 8-bit precision needs its calibration: call fp_calibrate for it (or fp_set_calibration_blob with its record) first");
  PreparedNets nets;   // (host phase of a first selection outside the lock)
  if (nets.prepare(m->refiner_path, m->refiner_p[precision] != nullptr, m->scorer_path, m->scorer_p[precision] != nullptr, precision)) return 1;
  LifeExclusive life;   // may load the networks of a precision: as exclusive as fp_create
  DeviceScope on_device(m->device);
  if (nets.adopt(m)) return 1;
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return select_precision(m, precision);
} FP_CATCH_INT
int fp_get_precision(const fp_model *m) { return m ? m->prec : -1; }

int fp_set_float_model(fp_model *m, int fmad) try {
  LifeExclusive life;   // destroys the captured graphs: not while another thread is inside a call
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  DeviceScope on_device(m->device);
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  m->fmad = fmad != 0;
  invalidate_graphs(m);
  return 0;
} FP_CATCH_INT
int fp_get_float_model(const fp_model *m) { return m ? (m->fmad ? 1 : 0) : -1; }

// Post-training static quantisation for the 8-bit precisions (FP_PREC_FP8 / FP_PREC_INT8) over K >= 1 calibration frames
// (fp_calibrate_begin / fp_calibrate_add_frame / fp_calibrate_finish; fp_calibrate = the three with one frame):
//   1. one Register per frame in f16 records, per channel of the 15 trunk activations of both networks, |max| and the mean OVER ALL
//      FRAMES (the statistics buffers accumulate across the Registers of a pass: integer atomics, so the result does not depend on order);
//   2. the 8-bit networks are quantised with per-channel activation scales folded into their weights (net_apply_q8);
//   3. bias correction (Nagel et al., "Data-free quantization through weight equalization and bias correction", 2019 -- here with
//      data): layer by layer, in trunk order, a pass of the 8-bit model over the frames measures the per-channel mean of the layer's
//      output and the difference to the f16 mean goes into its bias (two sweeps over the 13 layers);
//   4. what is left of the mean shift of the TOKEN tensor goes into the positional table;
//   5. what is left at the OUTPUTS (means over hypotheses and frames) goes into the output layers' biases.
// Why several frames [r5]: the common-mode part of the correction (steps 4, 5) measured on ONE frame is partly that frame's own
// (round 4: 0.6-0.7 mm of common-mode shift on other frames, 82-90 % of the refined poses within 1 mm / 1 deg); solved over frames of
// the deployment's scene family it is the family's mean and carries over to frames the calibration never saw.
// The record of the precision is replaced only when every step succeeded; a failure restores the previous record (or leaves the
// precision uncalibrated).  The pose is discarded; the model's precision is unchanged.  ~30 Registers per frame, once per deployment.
static constexpr int kCalibSlots = 16;   // frame-mean slots a record carries (more frames share slots: frame f -> slot f % 16)
// (re-)quantises the LOADED networks of `precision` from a record (weights and corrections)
static int apply_record(fp_model *m, int precision, const CalibRecord &r) {
  Net *loaded[2] = {m->refiner_p[precision], m->scorer_p[precision]};
  for (int k = 0; k < 2; k++)
    if (loaded[k] && (net_apply_q8(loaded[k], r.amax[k].data(), r.bias_fix[k].data(), r.tok_fix[k].data(), true, r.slots ? r.fmeans[k].data() : nullptr, r.slots) ||
                      net_q8_set_out_fix(loaded[k], r.out_fix[k].data()))) return 1;
  return 0;
}

// after a failed apply_record: the previous record goes back onto the precision's loaded networks, or the precision is left
// uncalibrated (fp_set_precision refuses it until a calibration succeeds)
static void restore_record(fp_model *m, int precision, const CalibRecord &before) {
  if (before.valid() && apply_record(m, precision, before) == 0) return;
  m->calib[precision] = {};
  for (Net *n : {m->refiner_p[precision], m->scorer_p[precision]}) if (n) net_q8_unready(n);
}

static int calibrate_impl(fp_model *m, const std::vector<CalibFrame> &frames, int precision) {   // (calibrate_locked checked m and precision)
  FP_CHECK(!frames.empty(), "[FoundationPose] fp_calibrate_finish: no calibration frame was added");
  FP_CHECK(m->refiner_p[precision] && m->scorer_p[precision] && m->refiner_p[PREC_F16] && m->scorer_p[PREC_F16], "[FoundationPose] fp_calibrate: networks not loaded");
  const int prev = m->prec;
  if (select_precision(m, PREC_F16)) return 1;
  float pose[16];
  constexpr size_t NS = (size_t)15 * 512;
  const double inv_frames = 1.0 / (double)frames.size();
  // means over the hypotheses of what the networks hand to the pose update / the cross-hypothesis head (still in the model's buffers
  // after a Register): refiner trans | rot, scorer pooled features; accumulated over the frames of a pass
  auto add_output_means = [&](std::vector<double> (&acc)[2]) -> int {
    const int N = m->n_hyp();
    std::vector<float> t((size_t)N * 3), r((size_t)N * 3), f((size_t)N * 512);
    FP_HIP_OK(hipMemcpyAsync(t.data(), m->trans_dev, t.size() * 4, hipMemcpyDeviceToHost, m->stream));
    FP_HIP_OK(hipMemcpyAsync(r.data(), m->rot_dev, r.size() * 4, hipMemcpyDeviceToHost, m->stream));
    FP_HIP_OK(hipMemcpyAsync(f.data(), m->feat_dev, f.size() * 4, hipMemcpyDeviceToHost, m->stream));
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    for (int c = 0; c < 3; c++) {
      double a = 0, b = 0;
      for (int i = 0; i < N; i++) { a += t[(size_t)i * 3 + c]; b += r[(size_t)i * 3 + c]; }
      acc[0][c] += a / N * inv_frames; acc[0][3 + c] += b / N * inv_frames;
    }
    for (int c = 0; c < 512; c++) {
      double a = 0;
      for (int i = 0; i < N; i++) a += f[(size_t)i * 512 + c];
      acc[1][c] += a / N * inv_frames;
    }
    return 0;
  };
  // one pass over the frames: statistics of both networks (mode / only_act: net_calib_begin), optionally the output means
  auto pass = [&](int mode, int only_act, std::vector<float> *amax, std::vector<float> (&mean)[2], std::vector<float> *out_mean) -> int {
    Net *nets[2] = {m->refiner, m->scorer};
    for (Net *n : nets) net_calib_begin(n, m->stream, mode, only_act);
    std::vector<double> acc[2] = {std::vector<double>(8, 0.0), std::vector<double>(512, 0.0)};
    int rc = 0;
    for (const CalibFrame &f : frames) {
      rc = register_whole(m, f.rgb.data(), f.depth.data(), f.mask.data(), FP_HOST, f.H, f.W, f.target.c_str(), 1, pose, true);
      if (!rc && out_mean) rc = add_output_means(acc);
      if (rc) break;
    }
    for (int k = 0; k < 2; k++) {
      mean[k].assign(NS, 0.f);
      if (amax) amax[k].assign(NS, 0.f);
      rc |= net_calib_end(nets[k], m->stream, amax ? amax[k].data() : nullptr, mean[k].data());
      if (out_mean) out_mean[k].assign(acc[k].begin(), acc[k].end());
    }
    return rc;
  };
  std::vector<float> f16_mean[2], f16_out_mean[2];
  CalibRecord rec;
  {   // 1. f16 statistics, frame by frame: |max| over all frames, the mean over all frames, and every frame's own channel means (slots)
    rec.slots = (int)std::min<size_t>(frames.size(), kCalibSlots);
    std::vector<double> acc_out[2] = {std::vector<double>(8, 0.0), std::vector<double>(512, 0.0)};
    std::vector<double> mean_acc[2] = {std::vector<double>(NS, 0.0), std::vector<double>(NS, 0.0)};
    std::vector<int> per_slot(rec.slots, 0);
    for (int k = 0; k < 2; k++) { rec.amax[k].assign(NS, 0.f); rec.fmeans[k].assign((size_t)rec.slots * NS, 0.f); }
    Net *nets[2] = {m->refiner, m->scorer};
    for (size_t f = 0; f < frames.size(); f++) {
      for (Net *n : nets) net_calib_begin(n, m->stream, 1, -1);
      int rc = register_whole(m, frames[f].rgb.data(), frames[f].depth.data(), frames[f].mask.data(), FP_HOST, frames[f].H, frames[f].W, frames[f].target.c_str(), 1, pose, true);
      if (!rc) rc = add_output_means(acc_out);
      const int slot = (int)(f % (size_t)rec.slots);
      per_slot[slot]++;
      for (int k = 0; k < 2; k++) {
        std::vector<float> am(NS), mn(NS);
        rc |= net_calib_end(nets[k], m->stream, am.data(), mn.data());
        for (size_t i = 0; i < NS; i++) {
          rec.amax[k][i] = std::max(rec.amax[k][i], am[i]);
          mean_acc[k][i] += mn[i];
          rec.fmeans[k][(size_t)slot * NS + i] += mn[i];
        }
      }
      if (rc) return 1;
    }
    for (int k = 0; k < 2; k++) {
      f16_mean[k].resize(NS);
      for (size_t i = 0; i < NS; i++) f16_mean[k][i] = (float)(mean_acc[k][i] * inv_frames);
      for (int sl = 0; sl < rec.slots; sl++)
        for (size_t i = 0; i < NS; i++) rec.fmeans[k][(size_t)sl * NS + i] /= (float)per_slot[sl];
      f16_out_mean[k].assign(acc_out[k].begin(), acc_out[k].end());
    }
  }
  for (int k = 0; k < 2; k++) { rec.bias_fix[k].assign((size_t)13 * 512, 0.f); rec.tok_fix[k].assign(512, 0.f); rec.out_fix[k].assign(k == 0 ? 8 : 512, 0.f); }
  // quantise (or re-quantise) this precision's networks without corrections
  if (apply_record(m, precision, rec)) return 1;
  invalidate_graphs(m);
  // (not select_precision: it would put the PREVIOUS record's output correction back on a network that is being re-calibrated)
  if (!m->ws_p[precision]) m->ws_p[precision] = nn_scratch_create(precision);
  m->prec = precision; m->refiner = m->refiner_p[precision]; m->scorer = m->scorer_p[precision]; m->ws = m->ws_p[precision];
  Net *qn[2] = {m->refiner, m->scorer};
  std::vector<float> mq[2];
  auto target = [&](int k, int a, int c) {   // f16 mean the output channel c of the layer writing activation a should have
    const std::vector<float> &t = f16_mean[k];
    return a == 5 ? 0.5f * (t[a * 512 + c] + t[a * 512 + c + 128]) : t[a * 512 + c];
  };
  const int n_sweeps = g_calib_sweeps;   // 2 (tools/q8_check.py, round 4: 0 / 1 / 2 / 3 sweeps -> 88 / 93 / 95-100 / 98 % of the refined poses within 1 mm / 1 deg of the f16 path)
  for (int sweep = 0; sweep < n_sweeps; sweep++)
    for (int layer = 0; layer < 13; layer++) {
      const int a = layer + 2, C = net_q8_bias_channels(layer);
      if (!net_q8_layer_on(qn[0], layer)) continue;   // [r6] a 2-byte layer of a partly 8-bit trunk has nothing to correct
      if (pass(2, a, nullptr, mq, nullptr)) return 1;
      for (int k = 0; k < 2; k++) {
        std::vector<float> &fix = rec.bias_fix[k];
        for (int c = 0; c < C; c++) {
          const float got = a == 5 ? 0.5f * (mq[k][a * 512 + c] + mq[k][a * 512 + c + 128]) : mq[k][a * 512 + c];
          fix[(size_t)layer * 512 + c] += target(k, a, c) - got;
        }
        if (net_apply_q8(qn[k], rec.amax[k].data(), fix.data(), rec.tok_fix[k].data(), false)) return 1;
      }
    }
  if (g_calib_tok && pass(2, 14, nullptr, mq, nullptr)) return 1;
  for (int k = 0; g_calib_tok && k < 2; k++) {
    for (int c = 0; c < 512; c++) rec.tok_fix[k][c] = f16_mean[k][14 * 512 + c] - mq[k][14 * 512 + c];
    if (net_apply_q8(qn[k], rec.amax[k].data(), rec.bias_fix[k].data(), rec.tok_fix[k].data(), false)) return 1;
  }
  // 5. what is left at the OUTPUTS (the heads are non-linear in the token mean): the mean refiner outputs / pooled score feature of
  //    the 8-bit model over the frames are moved onto the f16 model's through the output layers' biases
  if (g_calib_out) {
    std::vector<float> om[2];
    if (pass(2, 14, nullptr, mq, om)) return 1;
    for (int k = 0; k < 2; k++) {
      for (size_t c = 0; c < om[k].size(); c++) rec.out_fix[k][c] = f16_out_mean[k][c] - om[k][c];
      if (net_q8_set_out_fix(qn[k], rec.out_fix[k].data())) return 1;
    }
  }
  for (int k = 0; k < 2; k++)
    for (const std::vector<float> *v : {&rec.amax[k], &rec.bias_fix[k], &rec.tok_fix[k], &rec.out_fix[k], &rec.fmeans[k]})
      for (float x : *v) FP_CHECK(std::isfinite(x), "[FoundationPose] fp_calibrate: the solved record is not finite (broken weights or frames)");
  m->calib[precision] = rec;   // only now: every step succeeded
  invalidate_graphs(m);
  return select_precision(m, prev);
}

// Locking [r5]: exclusive (against every other call of the process) only while networks are LOADED -- the Registers of the
// calibration and the re-quantisation uploads into existing buffers run under the shared lifetime lock like any Register, so other
// models keep serving while one calibrates.
static int calibrate_locked(fp_model *m, const std::vector<CalibFrame> &frames, int precision) {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(precision == PREC_FP8 || precision == PREC_INT8, "[FoundationPose] fp_calibrate: precision must be FP_PREC_FP8 or FP_PREC_INT8");
  FP_CHECK(!m->refiner_path.empty() && !m->scorer_path.empty(), "[FoundationPose] fp_calibrate needs both networks");
  const int prev = m->prec;
  if (!m->refiner_p[precision] || !m->scorer_p[precision] || !m->refiner_p[PREC_F16] || !m->scorer_p[PREC_F16]) {
    PreparedNets q8, f16;   // host phase outside the lock
    if (q8.prepare(m->refiner_path, m->refiner_p[precision] != nullptr, m->scorer_path, m->scorer_p[precision] != nullptr, precision) ||
        f16.prepare(m->refiner_path, m->refiner_p[PREC_F16] != nullptr, m->scorer_path, m->scorer_p[PREC_F16] != nullptr, PREC_F16)) return 1;
    LifeExclusive life;   // device phase: one allocation + upload per network
    DeviceScope on_device(m->device);
    if (q8.adopt(m) || f16.adopt(m)) return 1;
    FP_HIP_OK(hipStreamSynchronize(m->stream));
    int rc = select_precision(m, precision) || select_precision(m, PREC_F16);
    rc = select_precision(m, rc ? PREC_F16 : prev) || rc;
    if (rc) return 1;
  }
  SerialGuard serial(m->device);
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  const CalibRecord before = m->calib[precision];
  const int rc = calibrate_impl(m, frames, precision);
  if (rc) {   // leave the model usable and the precision's networks consistent with its (previous) record
    const std::string why = g_last_error;
    for (Net *n : {m->refiner_p[precision], m->scorer_p[precision], m->refiner_p[PREC_F16], m->scorer_p[PREC_F16]}) if (n) net_calib_abort(n);
    (void)hipStreamSynchronize(m->stream);
    invalidate_graphs(m);
    restore_record(m, precision, before);
    const bool q8_prev = prev == PREC_FP8 || prev == PREC_INT8;
    (void)select_precision(m, (q8_prev && !m->calibrated(prev)) ? PREC_F16 : prev);
    set_error(why);
  }
  return rc;
}

static int copy_frame_in(fp_model *m, CalibFrame &f, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W) {
  const size_t px = (size_t)H * W;
  f.rgb.resize(px * 3); f.depth.resize(px); f.mask.resize(px);
  if (memspace == FP_HOST) {
    std::memcpy(f.rgb.data(), rgb, px * 3); std::memcpy(f.depth.data(), depth, px * 4); std::memcpy(f.mask.data(), mask, px);
    return 0;
  }
  FP_HIP_OK(hipMemcpyAsync(f.rgb.data(), rgb, px * 3, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipMemcpyAsync(f.depth.data(), depth, px * 4, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipMemcpyAsync(f.mask.data(), mask, px, hipMemcpyDeviceToHost, m->stream));
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  return 0;
}

int fp_calibrate_begin(fp_model *m, int precision) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(precision == PREC_FP8 || precision == PREC_INT8, "[FoundationPose] fp_calibrate_begin: precision must be FP_PREC_FP8 or FP_PREC_INT8");
  FP_CHECK(!m->refiner_path.empty() && !m->scorer_path.empty(), "[FoundationPose] fp_calibrate needs both networks");
  m->calib_frames.clear();
  m->calib_session_prec = precision;
  return 0;
} FP_CATCH_INT
int fp_calibrate_add_frame(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W, const char *target_name) try {
  SerialGuard serial(m ? m->device : -1);
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(m->calib_session_prec >= 0, "[FoundationPose] fp_calibrate_add_frame without fp_calibrate_begin");
  FP_CHECK(rgb && depth && mask, "[FoundationPose] fp_calibrate_add_frame: a calibration frame needs rgb, depth and mask");
  FP_CHECK(m->calib_frames.size() < 1024, "[FoundationPose] fp_calibrate_add_frame: too many frames (1024)");
  Target *t = nullptr;
  if (check_frame_args(m, H, W, target_name ? target_name : "", &t)) return 1;
  CalibFrame f;
  f.H = H; f.W = W; f.target = t->name;
  if (copy_frame_in(m, f, rgb, depth, mask, memspace, H, W)) return 1;
  m->calib_frames.push_back(std::move(f));
  return 0;
} FP_CATCH_INT
int fp_calibrate_finish(fp_model *m) try {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(m->calib_session_prec >= 0, "[FoundationPose] fp_calibrate_finish without fp_calibrate_begin");
  std::vector<CalibFrame> frames;
  frames.swap(m->calib_frames);
  const int precision = m->calib_session_prec;
  m->calib_session_prec = -1;
  return calibrate_locked(m, frames, precision);
} FP_CATCH_INT
int fp_calibrate_abort(fp_model *m) try {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  m->calib_frames.clear();
  m->calib_frames.shrink_to_fit();
  m->calib_session_prec = -1;
  return 0;
} FP_CATCH_INT
int fp_calibrate_frames(const fp_model *m) { return m && m->calib_session_prec >= 0 ? (int)m->calib_frames.size() : -1; }

int fp_calibrate(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W, const char *target_name,
                 int precision) try {
  FP_CHECK(m != nullptr, "[FoundationPose] null model");
  FP_CHECK(m->calib_session_prec < 0, "[FoundationPose] fp_calibrate while a fp_calibrate_begin session is open (finish or abort it first)");
  if (fp_calibrate_begin(m, precision)) return 1;
  if (fp_calibrate_add_frame(m, rgb, depth, mask, memspace, H, W, target_name)) { (void)fp_calibrate_abort(m); return 1; }
  return fp_calibrate_finish(m);
} FP_CATCH_INT
int fp_calibrate_fp8(fp_model *m, const void *rgb, const void *depth, const void *mask, int memspace, int H, int W,
                     const char *target_name) try {
  return fp_calibrate(m, rgb, depth, mask, memspace, H, W, target_name, PREC_FP8);
} FP_CATCH_INT

// ---- the calibration record, version 2: [magic "FPQ8", 2, precision, slots] + amax [2][15][512] + bias_fix [2][13][512] + tok_fix [2][512]
// + out_fix [8 | 512] + frame means [2][16 slots][15][512] (f32; unused slots zero).  Version 1 (round 4: no frame means, weights rounded
// to nearest) is still accepted.
static constexpr uint32_t kCalibMagic = 0x38515046u;
static constexpr size_t kCalibFloats = (size_t)2 * 15 * 512 + (size_t)2 * 13 * 512 + (size_t)2 * 512 + 8 + 512;
static constexpr size_t kCalibMeanFloats = (size_t)2 * kCalibSlots * 15 * 512;
static constexpr size_t kCalibSizeV1 = 16 + kCalibFloats * sizeof(float);
size_t fp_calibration_size(void) { return 16 + (kCalibFloats + kCalibMeanFloats) * sizeof(float); }
int fp_get_calibration_blob(const fp_model *m, int precision, void *out, size_t capacity) try {
  FP_CHECK(m && out && (precision == PREC_FP8 || precision == PREC_INT8), "[FoundationPose] fp_get_calibration_blob: invalid arguments");
  const CalibRecord &r = m->calib[precision];
  FP_CHECK(r.valid() && !r.bias_fix[0].empty(), "[FoundationPose] no calibration available for this precision");
  FP_CHECK(capacity >= fp_calibration_size(), "[FoundationPose] fp_get_calibration_blob: buffer too small (fp_calibration_size)");
  const int slots = r.slots;
  uint32_t hdr[4] = {kCalibMagic, 2u, (uint32_t)precision, (uint32_t)slots};
  unsigned char *p = (unsigned char *)out;
  std::memcpy(p, hdr, 16); p += 16;
  for (int k = 0; k < 2; k++) { std::memcpy(p, r.amax[k].data(), 15 * 512 * 4); p += 15 * 512 * 4; }
  for (int k = 0; k < 2; k++) { std::memcpy(p, r.bias_fix[k].data(), 13 * 512 * 4); p += 13 * 512 * 4; }
  for (int k = 0; k < 2; k++) { std::memcpy(p, r.tok_fix[k].data(), 512 * 4); p += 512 * 4; }
  for (int k = 0; k < 2; k++) { const size_t n = k == 0 ? 8 : 512; std::memcpy(p, r.out_fix[k].data(), n * 4); p += n * 4; }
  for (int k = 0; k < 2; k++) {
    const size_t n = (size_t)kCalibSlots * 15 * 512, have = (size_t)slots * 15 * 512;
    std::memset(p, 0, n * 4);
    if (have) std::memcpy(p, r.fmeans[k].data(), have * 4);
    p += n * 4;
  }
  return 0;
} FP_CATCH_INT
int fp_set_calibration_blob(fp_model *m, const void *blob, size_t bytes) try {
  LifeExclusive life;
  FP_CHECK(m && blob && (bytes == fp_calibration_size() || bytes == kCalibSizeV1), "[FoundationPose] fp_set_calibration_blob: invalid arguments / size");
  DeviceScope on_device(m->device);
  uint32_t hdr[4];
  const unsigned char *p = (const unsigned char *)blob;
  std::memcpy(hdr, p, 16); p += 16;
  const bool v2 = hdr[1] == 2u && bytes == fp_calibration_size(), v1 = hdr[1] == 1u && bytes == kCalibSizeV1;
  FP_CHECK(hdr[0] == kCalibMagic && (v1 || v2) && (hdr[2] == (uint32_t)PREC_FP8 || hdr[2] == (uint32_t)PREC_INT8) && (v1 ? hdr[3] == 0u : hdr[3] <= (uint32_t)kCalibSlots),
           "[FoundationPose] not a calibration record of this library version");
  const int precision = (int)hdr[2], slots = v2 ? (int)hdr[3] : 0;
  const size_t n_floats = kCalibFloats + (v2 ? kCalibMeanFloats : 0);
  {   // every float of the record must be finite (and the |max| values non-negative) BEFORE anything of the model is touched
    std::vector<float> tmp(n_floats);   // (the caller's buffer need not be aligned)
    std::memcpy(tmp.data(), p, n_floats * sizeof(float));
    const float *f = tmp.data();
    for (size_t i = 0; i < n_floats; i++) FP_CHECK(std::isfinite(f[i]), "[FoundationPose] calibration record holds non-finite values");
    for (size_t i = 0; i < (size_t)2 * 15 * 512; i++) FP_CHECK(f[i] >= 0.f, "[FoundationPose] calibration record holds a negative |max|");
  }
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  CalibRecord rec;
  auto take = [&](std::vector<float> &dst, size_t n) { dst.resize(n); std::memcpy(dst.data(), p, n * 4); p += n * 4; };
  for (int k = 0; k < 2; k++) take(rec.amax[k], 15 * 512);
  for (int k = 0; k < 2; k++) take(rec.bias_fix[k], 13 * 512);
  for (int k = 0; k < 2; k++) take(rec.tok_fix[k], 512);
  for (int k = 0; k < 2; k++) take(rec.out_fix[k], k == 0 ? 8 : 512);
  rec.slots = slots;
  for (int k = 0; v2 && k < 2; k++) { take(rec.fmeans[k], (size_t)kCalibSlots * 15 * 512); rec.fmeans[k].resize((size_t)slots * 15 * 512); }
  const CalibRecord before = m->calib[precision];
  if (apply_record(m, precision, rec)) {   // (re-quantises the networks of the precision that are already loaded)
    // a failure behind the first network leaves it re-quantised to the NEW record while the model still reports the old one
    const std::string why = fp_last_error();
    restore_record(m, precision, before);
    invalidate_graphs(m);
    set_error(why);
    return 1;
  }
  m->calib[precision] = rec;
  invalidate_graphs(m);
  return 0;
} FP_CATCH_INT
// legacy per-tensor view (round 2/3 API): |max| over the channels of each trunk activation, [refiner 16 | scorer 16]
int fp_get_calibration(const fp_model *m, float amax_out[32]) try {
  FP_CHECK(m && amax_out && (m->calibrated(PREC_FP8) || m->calibrated(PREC_INT8)), "[FoundationPose] no calibration available");
  const int pr = m->calibrated(PREC_FP8) ? PREC_FP8 : PREC_INT8;   // (the round-2 API knew FP8 only)
  for (int k = 0; k < 2; k++)
    for (int a = 0; a < 16; a++) {
      float v = 0.f;
      if (a < 15) for (int c = 0; c < 512; c++) v = std::max(v, m->calib[pr].amax[k][a * 512 + c]);
      amax_out[k * 16 + a] = v;
    }
  return 0;
} FP_CATCH_INT
// legacy: per-tensor |max| only -> every channel of a tensor gets the tensor's scale, no bias / token correction (FP8 networks)
int fp_set_calibration(fp_model *m, const float amax[32]) try {
  LifeExclusive life;
  FP_CHECK(m && amax, "[FoundationPose] fp_set_calibration: invalid arguments");
  DeviceScope on_device(m->device);
  FP_HIP_OK(hipStreamSynchronize(m->stream));
  CalibRecord rec;   // (no frame means: a per-tensor record's weights are rounded to nearest)
  for (int k = 0; k < 2; k++) {
    rec.amax[k].assign((size_t)15 * 512, 0.f);
    for (int a = 0; a < 15; a++)
      for (int c = 0; c < 512; c++) rec.amax[k][a * 512 + c] = amax[k * 16 + a];
    rec.bias_fix[k].assign((size_t)13 * 512, 0.f); rec.tok_fix[k].assign(512, 0.f); rec.out_fix[k].assign(k == 0 ? 8 : 512, 0.f);
  }
  for (int pr : {PREC_FP8, PREC_INT8}) m->calib[pr] = rec;
  for (int pr : {PREC_FP8, PREC_INT8})
    if (apply_record(m, pr, rec)) return 1;
  invalidate_graphs(m);
  return 0;
} FP_CATCH_INT

// ------------------------------------------------------------------------------------------------
// A network on its own, with the blob interface the reference's orchestrator drives through deploy_core's BaseInferCore
// (GetBuffer / GetTensor / SetBufferLocation / RawPtr / SetShape / SyncInfer, D6F/src/foundationpose.cpp:126-139,331-354,
// 410-436); include/infer_core_amd.hpp puts those C++ names on top of these calls.
// ------------------------------------------------------------------------------------------------
struct fp_net {
  int device = 0;
  hipStream_t stream = nullptr;
  Net *net = nullptr;
  NNScratch *ws = nullptr;
  bool scorer = false;
  int max_batch = 0;
  float *in_dev[2] = {nullptr, nullptr};   // render_input, transf_input  [max_batch,160,160,6] f32
  float *in_host[2] = {nullptr, nullptr};  // pinned, allocated on first use
  float *out_dev[2] = {nullptr, nullptr};  // trans, rot [max_batch,3]  |  scores [max_batch] (+ unused)
  float *out_host[2] = {nullptr, nullptr};
  float *feat_dev = nullptr;               // scorer: pooled features
  __half *nn_in = nullptr;                 // packed 2-byte network input
};
static size_t net_blob_elems(const fp_net *n, int idx, bool out) {
  if (!out) return (size_t)n->max_batch * FP_CROP_HW * FP_CROP_HW * 6;
  return (size_t)n->max_batch * (n->scorer ? 1 : 3) * (idx == 0 || !n->scorer ? 1 : 0);
}
static int net_blob_index(const fp_net *n, const char *name, bool *out) {
  const std::string s(name ? name : "");
  if (s == "render_input") { *out = false; return 0; }
  if (s == "transf_input") { *out = false; return 1; }
  if (!n->scorer && s == "trans") { *out = true; return 0; }
  if (!n->scorer && s == "rot") { *out = true; return 1; }
  if (n->scorer && s == "scores") { *out = true; return 0; }
  return -1;
}

static void destroy_net_impl(fp_net *n);
fp_net *fp_net_create(const char *weights_path, int is_scorer, int max_batch) try {
  if (!weights_path || max_batch <= 0) { set_error("[FoundationPose] fp_net_create: invalid arguments"); return nullptr; }
  if (max_batch > FP_MAX_BATCH) {
    set_error("[FoundationPose] fp_net_create: max_batch " + std::to_string(max_batch) + " above the batch limit FP_MAX_BATCH = " + std::to_string(FP_MAX_BATCH));
    return nullptr;
  }
  std::string err;
  std::unique_ptr<Net, void (*)(Net *)> prepared(net_prepare(weights_path, is_scorer != 0, PREC_F16, &err), net_free);   // host phase, outside the lock
  if (!prepared) { set_error("[FoundationPose] Failed to load network weights: " + err); return nullptr; }
  LifeExclusive life;   // (see SerialGuard)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("[FoundationPose] no HIP device available (this library has no CPU path)"); return nullptr; }
  std::unique_ptr<fp_net> n(new fp_net());
  if (hipGetDevice(&n->device) != hipSuccess) { set_error("[FoundationPose] hipGetDevice failed"); return nullptr; }
  n->scorer = is_scorer != 0;
  n->max_batch = max_batch;
  if (net_commit(prepared.get(), &err)) { set_error("[FoundationPose] Failed to load network weights: " + err); return nullptr; }
  n->net = prepared.release();
  n->ws = nn_scratch_create(PREC_F16);
  const size_t in_elems = (size_t)max_batch * FP_CROP_HW * FP_CROP_HW * 6;
  bool ok = stream_acquire(&n->stream) == hipSuccess;
  for (int i = 0; ok && i < 2; i++) ok = !dev_alloc(&n->in_dev[i], in_elems) && !dev_alloc(&n->out_dev[i], (size_t)max_batch * 3);
  ok = ok && !dev_alloc(&n->feat_dev, (size_t)max_batch * 512) && !dev_alloc(&n->nn_in, (size_t)2 * max_batch * FP_NN_IN_IMG_HALFS);
  ok = ok && hipMemsetAsync(n->nn_in, 0, (size_t)2 * max_batch * FP_NN_IN_IMG_HALFS * sizeof(__half), n->stream) == hipSuccess;
  if (!ok) { set_error("[FoundationPose] fp_net_create: device allocation failed"); destroy_net_impl(n.release()); return nullptr; }
  return n.release();
} FP_CATCH_PTR

static void destroy_net_impl(fp_net *n) {
  if (!n) return;
  DeviceScope on_device(n->device);
  if (n->stream) (void)hipStreamSynchronize(n->stream);
  for (int i = 0; i < 2; i++) {
    dev_free(n->in_dev[i]); dev_free(n->out_dev[i]);
    if (n->in_host[i]) (void)hipHostFree(n->in_host[i]);
    if (n->out_host[i]) (void)hipHostFree(n->out_host[i]);
  }
  dev_free(n->feat_dev); dev_free(n->nn_in);
  if (n->net) net_free(n->net);
  if (n->ws) nn_scratch_free(n->ws);
  if (n->stream) { (void)hipStreamSynchronize(n->stream); stream_release(n->stream); }
  delete n;
}
void fp_net_destroy(fp_net *n) {
  LifeExclusive life;
  destroy_net_impl(n);
}

// raw pointer of a blob in the given memory space (BlobsTensor::GetTensor(name)->RawPtr()); NULL + fp_last_error for an
// unknown name (the reference's GetTensor throws)
void *fp_net_blob(fp_net *n, const char *name, int memspace) try {
  bool out = false;
  const int idx = n ? net_blob_index(n, name, &out) : -1;
  if (idx < 0) { set_error(std::string("[FoundationPose] no blob named '") + (name ? name : "") + "'"); return nullptr; }
  if (memspace == FP_DEVICE) return out ? (void *)n->out_dev[idx] : (void *)n->in_dev[idx];
  float **h = out ? &n->out_host[idx] : &n->in_host[idx];
  if (!*h) {
    const size_t elems = out ? (size_t)n->max_batch * 3 : (size_t)n->max_batch * FP_CROP_HW * FP_CROP_HW * 6;
    if (hipHostMalloc((void **)h, elems * sizeof(float), hipHostMallocDefault) != hipSuccess) { set_error("[FoundationPose] pinned allocation failed"); return nullptr; }
  }
  return *h;
} FP_CATCH_PTR
int fp_net_max_batch(const fp_net *n) { return n ? n->max_batch : 0; }

// SyncInfer: inputs are taken from the blobs' FP_HOST or FP_DEVICE copies (render_loc / transf_loc), outputs are left in
// the device blobs and, with out_loc == FP_HOST, copied to the host blobs as well; returns when they are complete.
int fp_net_infer(fp_net *n, int batch, int render_loc, int transf_loc, int out_loc) try {
  SerialGuard serial(n ? n->device : -1);
  FP_CHECK(n && batch > 0 && batch <= n->max_batch, "[FoundationPose] fp_net_infer: batch out of range");
  const size_t px = (size_t)batch * FP_CROP_HW * FP_CROP_HW;
  const int locs[2] = {render_loc, transf_loc};
  for (int i = 0; i < 2; i++)
    if (locs[i] == FP_HOST) {
      FP_CHECK(n->in_host[i] != nullptr, "[FoundationPose] fp_net_infer: host input blob was never requested");
      FP_HIP_OK(hipMemcpyAsync(n->in_dev[i], n->in_host[i], px * 24, hipMemcpyHostToDevice, n->stream));
    }
  launch_pack_f32x6(n->stream, n->in_dev[0], n->nn_in, px, OUT_F16X8);
  launch_pack_f32x6(n->stream, n->in_dev[1], n->nn_in + (size_t)batch * FP_NN_IN_IMG_HALFS, px, OUT_F16X8);
  if (n->scorer) {
    if (scorer_features(n->stream, nullptr, n->net, n->ws, n->nn_in, batch, n->feat_dev)) return 1;
    if (scorer_head(n->stream, nullptr, n->net, n->ws, n->feat_dev, batch, n->out_dev[0])) return 1;
  } else {
    if (refiner_forward(n->stream, nullptr, n->net, n->ws, n->nn_in, batch, n->out_dev[0], n->out_dev[1])) return 1;
  }
  if (out_loc == FP_HOST) {
    const int nout = n->scorer ? 1 : 2;
    for (int i = 0; i < nout; i++) {
      if (!fp_net_blob(n, n->scorer ? "scores" : (i == 0 ? "trans" : "rot"), FP_HOST)) return 1;
      FP_HIP_OK(hipMemcpyAsync(n->out_host[i], n->out_dev[i], (size_t)batch * (n->scorer ? 1 : 3) * sizeof(float), hipMemcpyDeviceToHost, n->stream));
    }
  }
  FP_HIP_OK(hipStreamSynchronize(n->stream));
  return 0;
} FP_CATCH_INT

int fp_profile_enable(fp_model *m, int on) try {
  FP_CHECK(m, "null model");
  SerialGuard serial(m->device);
  m->prof.on = on != 0;
  return 0;
} FP_CATCH_INT
int fp_profile_reset(fp_model *m) try {
  FP_CHECK(m, "null model");
  SerialGuard serial(m->device);
  (void)hipStreamSynchronize(m->stream);
  m->prof.reset();
  return 0;
} FP_CATCH_INT
int fp_profile_report(fp_model *m, char *buf, int buf_len) try {
  FP_CHECK(m && buf && buf_len > 0, "fp_profile_report: invalid arguments");
  SerialGuard serial(m->device);
  (void)hipStreamSynchronize(m->stream);
  m->prof.collect();
  std::string out;
  char line[256];
  for (auto &e : m->prof.entries) {
    std::snprintf(line, sizeof(line), "%s %ld %.6f %.6e %.6e\n", e.name.c_str(), e.calls, e.ms, e.flops, e.bytes);
    out += line;
  }
  std::snprintf(buf, (size_t)buf_len, "%s", out.c_str());
  return 0;
} FP_CATCH_INT

}  // extern "C"
