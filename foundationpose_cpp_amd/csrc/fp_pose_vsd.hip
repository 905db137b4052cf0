// BOP's visible surface discrepancy of N poses on the device (fp_pose_vsd).  Two kernels: the batched vertex pass
// over (pose, vertex), and here a tile kernel over (pose, tile) items that rasterises the estimate and its ground truth into two LDS z-buffers,
// compares them with the observed depth pixel by pixel and adds integer pixel counts to the pose's counters.  Every rule that decides
// the depth of a pixel is fp_frame_rules.h's (shared with fp_render_pose); the rules of the metric itself are vsd_pixel below.  Compiled
// with -ffp-contract=off like the rest of the geometry: every f32 operation is separately rounded, tests/vsd_ref.py restates them.
#include "fp_frame_rules.h"

namespace fp {

namespace {

// no triangle id is kept: the z-buffers hold FrameKeyZ's 32-bit keys, whose minimum is the z frame_raster_kernel's 64-bit key resolves to
typedef FrameKeyZ Key;
constexpr int VSD_PX_PER_THREAD = FRAME_RENDER_TILE * FRAME_RENDER_TILE / FRAME_RENDER_THREADS;

// (a) the vertex pass is launch_pose_vertices' (fp_frame_render.hip): the estimates of a chunk, then its ground truths, the snapped
// vertex only (nothing is shaded, so no camera-space copy).

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

// (c) tile kernel: one workgroup per item {pose of the chunk, tile}.  PAIRED: the pose's own ground truth is walked into a second
// z-buffer; otherwise the call's one truth was rasterised once into plane_g [H,W] (0 = background) and is read from there.
template <bool PAIRED>
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void vsd_tile_kernel(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap_e,
                                                                        const int4 *__restrict__ snap_g, const float *__restrict__ plane_g,
                                                                        const int2 *__restrict__ items, const float *__restrict__ obs, int H, int W,
                                                                        int ntx, VsdParams P, int pose0, int *__restrict__ counters) {
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zb_e[T * T];
  __shared__ Key::type zb_g[PAIRED ? T * T : 1];
  __shared__ unsigned total[VSD_WORDS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  const FrameTile rect = frame_tile_rect_of(tile, ntx, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  frame_zbuf_clear<Key>(zb_e, tid);
  if (PAIRED) frame_zbuf_clear<Key>(zb_g, tid);
  if (tid < VSD_WORDS) total[tid] = 0;
  __syncthreads();
  frame_face_walk<Key>(faces, F, V, snap_e + (size_t)pose * V, rect, zb_e, tid);
  if (PAIRED) frame_face_walk<Key>(faces, F, V, snap_g + (size_t)pose * V, rect, zb_g, tid);
  __syncthreads();
  // wave-uniform counts: 6 of the masks, then one per threshold
  unsigned n_model_e = 0, n_model_g = 0, n_vis_e = 0, n_vis_g = 0, n_inter = 0, n_union = 0;
  unsigned n_fail[VSD_MAX_TAUS];
#pragma unroll
  for (int t = 0; t < VSD_MAX_TAUS; t++) n_fail[t] = 0;
#pragma unroll
  for (int k = 0; k < VSD_PX_PER_THREAD; k++) {
    const int i = k * FRAME_RENDER_THREADS + tid;
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const bool in = px < W && py < H;
    const size_t at = in ? (size_t)py * W + px : 0;
    const Key::type key_e = zb_e[i];
    const bool model_e = in && key_e != Key::EMPTY;
    const float z_e = model_e ? Key::z(key_e) : 0.0f;
    bool model_g;
    float z_g;
    if (PAIRED) {
      const Key::type key_g = zb_g[i];
      model_g = in && key_g != Key::EMPTY;
      z_g = model_g ? Key::z(key_g) : 0.0f;
    } else {
      z_g = in ? plane_g[at] : 0.0f;
      model_g = z_g != 0.0f;
    }
    const float D = in ? obs[at] : 0.0f;
    const VsdPixel v = vsd_pixel(px, py, model_e, z_e, model_g, z_g, D, P);
    const bool inter = v.vis_g && v.vis_e;
    n_model_e += wave_count(model_e); n_model_g += wave_count(model_g);
    n_vis_e += wave_count(v.vis_e); n_vis_g += wave_count(v.vis_g);
    n_inter += wave_count(inter); n_union += wave_count(v.vis_g || v.vis_e);
#pragma unroll
    for (int t = 0; t < VSD_MAX_TAUS; t++)
      if (t < P.T) n_fail[t] += wave_count(inter && v.d >= P.thr[t]);   // (uniform)
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

void launch_vsd_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap_e, const int4 *snap_g, const float *plane_g, const int2 *items, int n_items,
                      const float *depth, int H, int W, const VsdParams &P, int pose0, int *counters) {
  FP_GEOM_LOG("vsd_tile");
  if (n_items <= 0) return;
  const int ntx = scene_tiles_x(W);
  if (snap_g)
    hipLaunchKernelGGL(vsd_tile_kernel<true>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap_e, snap_g, plane_g, items, depth, H,
                       W, ntx, P, pose0, counters);
  else
    hipLaunchKernelGGL(vsd_tile_kernel<false>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap_e, snap_g, plane_g, items, depth, H,
                       W, ntx, P, pose0, counters);
}

}  // namespace fp
