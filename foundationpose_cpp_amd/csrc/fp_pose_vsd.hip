// BOP's visible surface discrepancy of N poses on the device (fp_pose_vsd).  Two kernels: a vertex pass over
// (pose, vertex) and a tile kernel over (pose, tile) items that rasterises the estimate and its ground truth into two LDS z-buffers,
// compares them with the observed depth pixel by pixel and adds integer pixel counts to the pose's counters.  Every rule that decides
// the depth of a pixel is fp_frame_rules.h's (shared with fp_render_pose); the rules of the metric itself are vsd_pixel below.  Compiled
// with -ffp-contract=off like the rest of the geometry: every f32 operation is separately rounded, tests/vsd_ref.py restates them.
#include "fp_frame_rules.h"

namespace fp {

namespace {

constexpr unsigned VSD_EMPTY = ~0u;   // a z-buffer entry no triangle has reached: larger than the bits of every positive float
constexpr int VSD_TILE = FRAME_RENDER_TILE, VSD_THREADS = FRAME_RENDER_THREADS;
constexpr int VSD_PX_PER_THREAD = VSD_TILE * VSD_TILE / VSD_THREADS;

// (a) vertex pass: pose p of the launch (the estimates of a chunk, then its ground truths) times vertex i -> the snapped vertex only
// (nothing is shaded, so no camera-space copy); a refused vertex raises its bit of the pose's own word.
__global__ __launch_bounds__(256) void vsd_vertex_kernel(const float *__restrict__ verts, int V, const FramePose *__restrict__ poses_est, int n_est,
                                                         const FramePose *__restrict__ poses_gt, int4 *__restrict__ snap, int *__restrict__ flags_est, int *__restrict__ flags_gt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
  if (i >= V) return;
  float4 cam;
  const int bad = frame_vertex_rule(verts, (size_t)i, p < n_est ? poses_est[p] : poses_gt[p - n_est], snap[(size_t)p * V + i], cam);
  if (bad) atomicOr(p < n_est ? flags_est + p : flags_gt + (p - n_est), bad);
}

// the walk of frame_raster_kernel into a z-buffer of 32-bit keys: no triangle id is kept, and positive floats order like their bit
// patterns, so the unsigned minimum of bits(z) is the z of the 64-bit key bits(z) << 32 | triangle
__device__ __forceinline__ void vsd_walk(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap, int X0, int Y0, int X1,
                                         int Y1, unsigned *zbuf, int tid) {
  for (int t = tid; t < F; t += VSD_THREADS) {
    const int i0 = faces[(size_t)t * 3], i1 = faces[(size_t)t * 3 + 1], i2 = faces[(size_t)t * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const int4 a = snap[i0], b = snap[i1], c = snap[i2];
    frame_tri_walk(a, b, c, X0, Y0, X1, Y1, [&](int px, int py, float z) { atomicMin(&zbuf[(py - Y0) * VSD_TILE + (px - X0)], __float_as_uint(z)); });
  }
}

// the metric's rules at one pixel (c, r): model_e / model_g say whether the renderings cover it, z_e / z_g are their depths, D is the
// RAW observed depth.  Distances from the camera centre, BOP19 visibility with missing depth counted as visible.
struct VsdPixel {
  bool vis_e, vis_g;
  float d;   // |d_g - d_e|, meaningful on the intersection
};
__device__ __forceinline__ bool vsd_hidden(float D, float d, float d_t, float delta) { return !(D < FP_MIN_DEPTH) && (d - d_t) > delta; }
__device__ __forceinline__ VsdPixel vsd_pixel(int c, int r, bool model_e, float z_e, bool model_g, float z_g, float D, const VsdParams &P) {
  const float X = ((float)c - P.cx) / P.fx, Y = ((float)r - P.cy) / P.fy;
  const float q = sqrtf((X * X + Y * Y) + 1.0f);
  const float d_t = D * q, d_e = z_e * q, d_g = z_g * q;
  VsdPixel o;
  o.vis_g = model_g && !vsd_hidden(D, d_g, d_t, P.delta);
  o.vis_e = model_e && (!vsd_hidden(D, d_e, d_t, P.delta) || o.vis_g);
  o.d = fabsf(d_g - d_e);
  return o;
}

__device__ __forceinline__ unsigned vsd_count(bool b) { return (unsigned)__popcll(__ballot(b)); }

// (c) tile kernel: one workgroup per item {pose of the chunk, tile}.  PAIRED: the pose's own ground truth is walked into a second
// z-buffer; otherwise the call's one truth was rasterised once into plane_g [H,W] (0 = background) and is read from there.
template <bool PAIRED>
__global__ __launch_bounds__(VSD_THREADS) void vsd_tile_kernel(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap_e,
                                                               const int4 *__restrict__ snap_g, const float *__restrict__ plane_g,
                                                               const int2 *__restrict__ items, const float *__restrict__ obs, int H, int W,
                                                               int ntx, VsdParams P, int pose0, int *__restrict__ counters) {
  constexpr int T = VSD_TILE;
  __shared__ unsigned zb_e[T * T];
  __shared__ unsigned zb_g[PAIRED ? T * T : 1];
  __shared__ unsigned total[VSD_WORDS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  const int X0 = (tile % ntx) * T, Y0 = (tile / ntx) * T;
  const int X1 = min(X0 + T - 1, W - 1), Y1 = min(Y0 + T - 1, H - 1);
  for (int i = tid; i < T * T; i += VSD_THREADS) {
    zb_e[i] = VSD_EMPTY;
    if (PAIRED) zb_g[i] = VSD_EMPTY;
  }
  if (tid < VSD_WORDS) total[tid] = 0;
  __syncthreads();
  vsd_walk(faces, F, V, snap_e + (size_t)pose * V, X0, Y0, X1, Y1, zb_e, tid);
  if (PAIRED) vsd_walk(faces, F, V, snap_g + (size_t)pose * V, X0, Y0, X1, Y1, zb_g, tid);
  __syncthreads();
  // wave-uniform counts: 6 of the masks, then one per threshold
  unsigned n_model_e = 0, n_model_g = 0, n_vis_e = 0, n_vis_g = 0, n_inter = 0, n_union = 0;
  unsigned n_fail[VSD_MAX_TAUS];
#pragma unroll
  for (int t = 0; t < VSD_MAX_TAUS; t++) n_fail[t] = 0;
#pragma unroll
  for (int k = 0; k < VSD_PX_PER_THREAD; k++) {
    const int i = k * VSD_THREADS + tid;
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const bool in = px < W && py < H;
    const size_t at = in ? (size_t)py * W + px : 0;
    const unsigned key_e = zb_e[i];
    const bool model_e = in && key_e != VSD_EMPTY;
    const float z_e = model_e ? __uint_as_float(key_e) : 0.0f;
    bool model_g;
    float z_g;
    if (PAIRED) {
      const unsigned key_g = zb_g[i];
      model_g = in && key_g != VSD_EMPTY;
      z_g = model_g ? __uint_as_float(key_g) : 0.0f;
    } else {
      z_g = in ? plane_g[at] : 0.0f;
      model_g = z_g != 0.0f;
    }
    const float D = in ? obs[at] : 0.0f;
    const VsdPixel v = vsd_pixel(px, py, model_e, z_e, model_g, z_g, D, P);
    const bool inter = v.vis_g && v.vis_e;
    n_model_e += vsd_count(model_e); n_model_g += vsd_count(model_g);
    n_vis_e += vsd_count(v.vis_e); n_vis_g += vsd_count(v.vis_g);
    n_inter += vsd_count(inter); n_union += vsd_count(v.vis_g || v.vis_e);
#pragma unroll
    for (int t = 0; t < VSD_MAX_TAUS; t++)
      if (t < P.T) n_fail[t] += vsd_count(inter && v.d >= P.thr[t]);   // (uniform)
  }
  if ((tid & 63) == 0) {
    const unsigned six[6] = {n_model_e, n_model_g, n_vis_e, n_vis_g, n_inter, n_union};
#pragma unroll
    for (int j = 0; j < 6; j++)
      if (six[j]) atomicAdd(&total[j], six[j]);
#pragma unroll
    for (int t = 0; t < VSD_MAX_TAUS; t++)
      if (n_fail[t]) atomicAdd(&total[6 + t], n_fail[t]);
  }
  __syncthreads();
  if (tid < VSD_WORDS) {
    const unsigned n = total[tid];
    if (n) atomicAdd(counters + (size_t)(pose0 + pose) * VSD_WORDS + tid, (int)n);
  }
}

}  // namespace

void launch_vsd_vertex(hipStream_t s, const DeviceMesh &m, const FramePose *poses_est, int n_est, const FramePose *poses_gt, int n_gt, int4 *snap,
                       int *flags_est, int *flags_gt) {
  FP_GEOM_LOG("vsd_vertex");
  if (n_est + n_gt <= 0 || m.V <= 0) return;
  hipLaunchKernelGGL(vsd_vertex_kernel, dim3((unsigned)((m.V + 255) / 256), (unsigned)(n_est + n_gt)), dim3(256), 0, s, m.verts, m.V, poses_est, n_est,
                     poses_gt, snap, flags_est, flags_gt);
}

void launch_vsd_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap_e, const int4 *snap_g, const float *plane_g, const int2 *items, int n_items,
                      const float *depth, int H, int W, const VsdParams &P, int pose0, int *counters) {
  FP_GEOM_LOG("vsd_tile");
  if (n_items <= 0) return;
  const int ntx = (W + VSD_TILE - 1) / VSD_TILE;
  if (snap_g)
    hipLaunchKernelGGL(vsd_tile_kernel<true>, dim3((unsigned)n_items), dim3(VSD_THREADS), 0, s, m.faces, m.F, m.V, snap_e, snap_g, plane_g, items, depth, H,
                       W, ntx, P, pose0, counters);
  else
    hipLaunchKernelGGL(vsd_tile_kernel<false>, dim3((unsigned)n_items), dim3(VSD_THREADS), 0, s, m.faces, m.F, m.V, snap_e, snap_g, plane_g, items, depth, H,
                       W, ntx, P, pose0, counters);
}

}  // namespace fp
