// Colour agreement of N poses with the uploaded frame (fp_pose_color): the device half.  Two kernels: the batched
// vertex pass over (pose, vertex), which keeps the snapped vertex only (its z word holds the corner depth), and here a tile kernel over
// (pose, tile) items that rasterises the pose into a 64-bit LDS z-buffer exactly as frame_raster_kernel does, gives every visible model
// pixel the model's unshaded colour there (nearest texel with wrap, or interpolated vertex colours) and adds, per channel, the five
// integer sums of a normalised cross-correlation with the frame's bytes, plus four pixel counts.  Every rule that decides the depth and
// the triangle of a pixel, and the weights inside the triangle, is fp_frame_rules.h's; the rules of the colour are color_pixel below.
// Compiled with -ffp-contract=off like the rest of the geometry: every f32 operation is separately rounded, tests/color_ref.py restates
// them.  The correlation itself is the host's.
#include "fp_frame_rules.h"

namespace fp {

namespace {

typedef FrameKeyZTri Key;   // the colour needs the winning triangle: frame_raster_kernel's 64-bit keys
constexpr int COLOR_PX_PER_THREAD = FRAME_RENDER_TILE * FRAME_RENDER_TILE / FRAME_RENDER_THREADS;
constexpr int COLOR_WAVES = FRAME_RENDER_THREADS / 64;

// (a) the vertex pass is launch_pose_vertices' (fp_frame_render.hip): the poses of a chunk, the snapped vertex only.

// the model's colour at a pixel with weights g inside the triangle of vertices i0 i1 i2: false when the pixel has none
struct ColorSource {
  const float2 *uvs;       // [V] (u, 1 - v)
  const uint8_t *tex;      // [TH, TW, 3]
  int TH, TW;
  const uint32_t *vcol;    // [V] r | g << 8 | b << 16
};
template <bool VCOL>
__device__ __forceinline__ bool color_pixel(const ColorSource &S, int i0, int i1, int i2, const FrameWeights &g, int m[3]) {
  if (VCOL) {
    const uint32_t c0 = S.vcol[i0], c1 = S.vcol[i1], c2 = S.vcol[i2];
    bool ok = true;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float v = (g.g0 * (float)((c0 >> (8 * ch)) & 255u) + g.g1 * (float)((c1 >> (8 * ch)) & 255u)) + g.g2 * (float)((c2 >> (8 * ch)) & 255u);
      ok = ok && !(v != v);
      m[ch] = (int)rintf(fminf(fmaxf(v, 0.0f), 255.0f));   // (of a NaN: 0, and the pixel is not compared)
    }
    return ok;
  }
  const float2 t0 = S.uvs[i0], t1 = S.uvs[i1], t2 = S.uvs[i2];
  const float U = (g.g0 * t0.x + g.g1 * t1.x) + g.g2 * t2.x;
  const float Vt = (g.g0 * t0.y + g.g1 * t1.y) + g.g2 * t2.y;
  if (!(fabsf(U) <= 3.402823466e+38f) || !(fabsf(Vt) <= 3.402823466e+38f)) return false;   // not finite: nothing is read
  const float fu = U - floorf(U), fv = Vt - floorf(Vt);   // in [0, 1]
  const int tx = min((int)(fu * (float)S.TW), S.TW - 1), ty = min((int)(fv * (float)S.TH), S.TH - 1);
  const uint8_t *p = S.tex + ((size_t)ty * S.TW + tx) * 3;
  m[0] = p[0]; m[1] = p[1]; m[2] = p[2];
  return true;
}

// (b) tile kernel: one workgroup per item {pose of the launch's chunk, tile}.  flags / acc are indexed by pose0 + pose.
template <bool VCOL>
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void color_tile_kernel(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap,
                                                                          ColorSource S, const int2 *__restrict__ items,
                                                                          const uint8_t *__restrict__ rgb, const float *__restrict__ obs, int H, int W,
                                                                          int ntx, float tol, const int *__restrict__ flags, int pose0,
                                                                          unsigned long long *__restrict__ acc) {
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zbuf[T * T];
  __shared__ unsigned part[COLOR_WAVES][COLOR_WORDS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  if (flags[pose0 + pose]) return;   // (uniform) a refused pose: the host gives its record the status bit
  const FrameTile rect = frame_tile_rect_of(tile, ntx, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  frame_zbuf_clear<Key>(zbuf, tid);
  __syncthreads();
  const int4 *__restrict__ sn = snap + (size_t)pose * V;
  frame_face_walk<Key>(faces, F, V, sn, rect, zbuf, tid);
  __syncthreads();
  // a tile has at most 1 024 pixels and a product is at most 65 025: every partial sum of the workgroup fits 32 bits
  unsigned sum[COLOR_SUMS];
#pragma unroll
  for (int j = 0; j < COLOR_SUMS; j++) sum[j] = 0;
  unsigned n_model = 0, n_visible = 0, n_compared = 0, n_nocolor = 0;   // wave-uniform
#pragma unroll
  for (int k = 0; k < COLOR_PX_PER_THREAD; k++) {
    const int i = k * FRAME_RENDER_THREADS + tid;
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const bool in = px < W && py < H;
    const Key::type key = zbuf[i];
    const bool model = in && key != Key::EMPTY;   // (a key exists only for a triangle whose three indices are below V)
    bool visible = false, compared = false;
    if (model) {
      const float z = Key::z(key);
      const size_t at = (size_t)py * W + px;
      visible = !frame_occluded(obs[at], z, tol);
      if (visible) {
        const size_t tri = (size_t)Key::tri(key);
        const int i0 = faces[tri * 3], i1 = faces[tri * 3 + 1], i2 = faces[tri * 3 + 2];
        const FrameWeights g = frame_tri_weights(sn[i0], sn[i1], sn[i2], px, py, z);
        int m[3];
        compared = color_pixel<VCOL>(S, i0, i1, i2, g, m);
        if (compared) {
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const unsigned mv = (unsigned)m[ch], ov = rgb[at * 3 + ch];
            sum[ch] += mv; sum[3 + ch] += ov; sum[6 + ch] += mv * mv; sum[9 + ch] += ov * ov; sum[12 + ch] += mv * ov;
          }
        }
      }
    }
    n_model += wave_count(model); n_visible += wave_count(visible);
    n_compared += wave_count(compared); n_nocolor += wave_count(visible && !compared);
  }
  // per wave, then across the four waves through LDS, then one integer atomic per quantity: integer sums do not depend on the order
  const int wave = tid >> 6, lane = tid & 63;
  if (n_compared) {   // (uniform)
#pragma unroll
    for (int j = 0; j < COLOR_SUMS; j++) {
      unsigned v = sum[j];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      sum[j] = v;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < COLOR_SUMS; j++) part[wave][j] = sum[j];
    part[wave][COLOR_SUMS] = n_model; part[wave][COLOR_SUMS + 1] = n_visible;   // (ballots: the counts of the wave's own lanes)
    part[wave][COLOR_SUMS + 2] = n_compared; part[wave][COLOR_SUMS + 3] = n_nocolor;
  }
  __syncthreads();
  if (tid < COLOR_WORDS) {
    unsigned v = 0;
#pragma unroll
    for (int w = 0; w < COLOR_WAVES; w++) v += part[w][tid];
    if (v) atomicAdd(acc + (size_t)(pose0 + pose) * COLOR_WORDS + tid, (unsigned long long)v);
  }
}

}  // namespace

void launch_color_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const uint8_t *rgb, const float *depth,
                        int H, int W, float tol_m, const int *flags, int pose0, unsigned long long *acc) {
  FP_GEOM_LOG("color_tile");
  if (n_items <= 0) return;
  const int ntx = scene_tiles_x(W);
  const ColorSource S = {reinterpret_cast<const float2 *>(m.uvs), m.tex, m.TH, m.TW, m.vcol};
  if (m.vcol)
    hipLaunchKernelGGL(color_tile_kernel<true>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, S, items, rgb, depth, H, W,
                       ntx, tol_m, flags, pose0, acc);
  else
    hipLaunchKernelGGL(color_tile_kernel<false>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, S, items, rgb, depth, H, W,
                       ntx, tol_m, flags, pose0, acc);
}

}  // namespace fp
