// Refinement of N poses on the outline of a mask of the uploaded frame (fp_refine_silhouette): the device half.
// Two kernels of its own: the signed squared distance of the mask out of fp_mask_distance's two maps, and a tile kernel over (pose, tile)
// items that rasterises the pose's tile, grown by one pixel on each side, into a 32-bit LDS z-buffer with frame_tri_walk, finds the
// contour pixels of the pose among the tile's own 32 x 32, and reduces the 6 x 6 normal system of the pose's outline against the mask's as
// 28 integer sums plus seven pixel counts.  The vertex pass is launch_pose_vertices' (fp_frame_render.hip), the distance transform
// fp_pose_silhouette.hip's.  Every rule that decides the depth of a pixel is fp_frame_rules.h's; the rules of the residual are
// silref_pixel below.  Compiled with -ffp-contract=off like the rest of the geometry: every f32 operation is separately rounded,
// tests/silref_ref.py restates them.  The solve is the host's.
#include "fp_frame_rules.h"

namespace fp {

namespace {

typedef FrameKeyZ Key;   // the depth decides; the triangle is not needed
constexpr int SILREF_THREADS = 256;
constexpr int SILREF_GROWN = FRAME_RENDER_TILE + 2;   // the tile and one pixel on each side
constexpr int SILREF_PX_PER_THREAD = FRAME_RENDER_TILE * FRAME_RENDER_TILE / FRAME_RENDER_THREADS;
constexpr int SILREF_WAVES = FRAME_RENDER_THREADS / 64;

// (a) the signed map: one thread per pixel
__global__ __launch_bounds__(SILREF_THREADS) void mask_signed_d2(const uint8_t *__restrict__ mask, const uint32_t *__restrict__ d2, size_t px,
                                                                 int32_t *__restrict__ sd) {
  const size_t i = (size_t)blockIdx.x * SILREF_THREADS + threadIdx.x;
  if (i >= px) return;
  sd[i] = mask[i] > 0 ? -(int32_t)d2[px + i] : (int32_t)d2[i];   // (both are at most FP_SIL_D2_NONE = 2^31 - 1)
}

// the distance in pixels to the mask's outline, negative inside: 0 on the mask's own contour pixels, 1 on the first ring outside
__device__ __forceinline__ float silref_psi(int32_t sd) { return sd > 0 ? sqrtf((float)sd) : sd == 0 ? 0.0f : 1.0f - sqrtf((float)(-sd)); }

// the rules of the residual at one contour pixel (c, r) at model depth z: psi at the pixel, (gx, gy) the gradient of psi there.
// J and e are set; steep: one of them is a NaN or above SILREF_MAX_TERM in magnitude.
struct SilrefPixel {
  bool steep;
  float J[6], e;
};
__device__ __forceinline__ SilrefPixel silref_pixel(int c, int r, float z, float psi, float gx, float gy, const SilrefParams &P) {
  SilrefPixel o;
  const float X = ((float)c - P.cx) / P.fx, Y = ((float)r - P.cy) / P.fy;
  const float ax = (gx * P.kx) / z, ay = (gy * P.ky) / z;
  const float az = -(ax * X + ay * Y);
  const float cx = (z * X - P.t[0]) / P.rad, cy = (z * Y - P.t[1]) / P.rad, cz = (z - P.t[2]) / P.rad;
  o.J[0] = cy * az - cz * ay; o.J[1] = cz * ax - cx * az; o.J[2] = cx * ay - cy * ax;
  o.J[3] = ax; o.J[4] = ay; o.J[5] = az;
  o.e = -psi / P.s;
  bool ok = fabsf(o.e) <= SILREF_MAX_TERM;   // (false for a NaN)
#pragma unroll
  for (int a = 0; a < 6; a++) ok = ok && fabsf(o.J[a]) <= SILREF_MAX_TERM;
  o.steep = !ok;
  return o;
}

__device__ __forceinline__ long long silref_q24(float v) { return llrintf(v * 16777216.0f); }   // (the scaling is exact)

// (b) tile kernel: one workgroup per item {pose of the launch's chunk, tile}.  params / flags / acc are indexed by pose0 + pose.
template <bool OCCLUSION>
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void silref_tile(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap,
                                                                    const int2 *__restrict__ items, const float *__restrict__ obs,
                                                                    const int32_t *__restrict__ sd, int H, int W, int ntx, int gate2, float tol,
                                                                    const SilrefParams *__restrict__ params, const int *__restrict__ flags, int pose0,
                                                                    unsigned long long *__restrict__ acc) {
  constexpr int T = FRAME_RENDER_TILE, G = SILREF_GROWN;
  __shared__ Key::type zbuf[G * G];   // entry (ly, lx) is pixel (Y0 - 1 + ly, X0 - 1 + lx); one outside the frame stays EMPTY
  __shared__ long long part[SILREF_WAVES][SILREF_SUMS];
  __shared__ unsigned counts[SILREF_COUNTS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  if (flags[pose0 + pose]) return;   // (uniform) a refused pose: the host drops its record
  const FrameTile rect = frame_tile_rect_of(tile, ntx, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  // the tile grown by one pixel on each side, cut to the frame
  const int GX0 = max(X0 - 1, 0), GY0 = max(Y0 - 1, 0), GX1 = min(rect.X1 + 1, W - 1), GY1 = min(rect.Y1 + 1, H - 1);
  for (int i = tid; i < G * G; i += FRAME_RENDER_THREADS) zbuf[i] = Key::EMPTY;
  if (tid < SILREF_COUNTS) counts[tid] = 0;
  __syncthreads();
  const int4 *__restrict__ sn = snap + (size_t)pose * V;
  for (int t = tid; t < F; t += FRAME_RENDER_THREADS) {   // frame_face_walk's loop with this kernel's rectangle and stride
    const int i0 = faces[(size_t)t * 3], i1 = faces[(size_t)t * 3 + 1], i2 = faces[(size_t)t * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const int4 a = sn[i0], b = sn[i1], c = sn[i2];
    frame_tri_walk(a, b, c, GX0, GY0, GX1, GY1, [&](int px, int py, float z) {
      atomicMin(&zbuf[(py - Y0 + 1) * G + (px - X0 + 1)], Key::pack(z, (unsigned)t));
    });
  }
  __syncthreads();
  const SilrefParams P = params[pose0 + pose];
  long long sum[SILREF_SUMS];
#pragma unroll
  for (int j = 0; j < SILREF_SUMS; j++) sum[j] = 0;
  unsigned n_model = 0, n_contour = 0, n_used = 0, n_occluded = 0, n_far = 0, n_flat = 0, n_steep = 0;   // wave-uniform
#pragma unroll
  for (int k = 0; k < SILREF_PX_PER_THREAD; k++) {
    const int i = k * FRAME_RENDER_THREADS + tid;
    const int lx = (i & (T - 1)) + 1, ly = i / T + 1;
    const int px = X0 + lx - 1, py = Y0 + ly - 1;
    const Key::type key = zbuf[ly * G + lx];
    const bool model = px < W && py < H && key != Key::EMPTY;
    // a contour pixel: a model pixel with a neighbour INSIDE the frame that is not one
    const bool contour = model && ((px > 0 && zbuf[ly * G + lx - 1] == Key::EMPTY) || (px + 1 < W && zbuf[ly * G + lx + 1] == Key::EMPTY) ||
                                   (py > 0 && zbuf[(ly - 1) * G + lx] == Key::EMPTY) || (py + 1 < H && zbuf[(ly + 1) * G + lx] == Key::EMPTY));
    int cls = 0;   // 1 used, 2 occluded, 3 far, 4 flat, 5 steep
    SilrefPixel q;
    if (contour) {
      const float z = Key::z(key);
      const size_t row = (size_t)py * W;
      const int32_t s0 = sd[row + px];
      if (OCCLUSION && frame_occluded(obs[row + px], z, tol)) cls = 2;
      else if (gate2 > 0 && (s0 < 0 ? -(long long)s0 : (long long)s0) > (long long)gate2) cls = 3;
      else {
        const float psi = silref_psi(s0);
        const float gx = (silref_psi(sd[row + min(px + 1, W - 1)]) - silref_psi(sd[row + max(px - 1, 0)])) * 0.5f;
        const float gy = (silref_psi(sd[(size_t)min(py + 1, H - 1) * W + px]) - silref_psi(sd[(size_t)max(py - 1, 0) * W + px])) * 0.5f;
        if (gx == 0.0f && gy == 0.0f) cls = 4;
        else {
          q = silref_pixel(px, py, z, psi, gx, gy, P);
          cls = q.steep ? 5 : 1;
        }
      }
    }
    n_model += wave_count(model); n_contour += wave_count(contour);
    n_used += wave_count(cls == 1); n_occluded += wave_count(cls == 2);
    n_far += wave_count(cls == 3); n_flat += wave_count(cls == 4); n_steep += wave_count(cls == 5);
    if (cls == 1) {
      int j = 0;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) sum[j++] += silref_q24(q.J[a] * q.J[b]);
#pragma unroll
      for (int a = 0; a < 6; a++) sum[21 + a] += silref_q24(q.J[a] * q.e);
      sum[27] += silref_q24(q.e * q.e);
    }
  }
  // per wave, then across the four waves through LDS, then one integer atomic per quantity: integer sums do not depend on the order
  const int wave = tid >> 6, lane = tid & 63;
  if (n_used) {   // (uniform)
#pragma unroll
    for (int j = 0; j < SILREF_SUMS; j++) {
      long long v = sum[j];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      sum[j] = v;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < SILREF_SUMS; j++) part[wave][j] = sum[j];
    const unsigned seven[SILREF_COUNTS] = {n_model, n_contour, n_used, n_occluded, n_far, n_flat, n_steep};
#pragma unroll
    for (int j = 0; j < SILREF_COUNTS; j++)
      if (seven[j]) atomicAdd(&counts[j], seven[j]);
  }
  __syncthreads();
  unsigned long long *dst = acc + (size_t)(pose0 + pose) * SILREF_WORDS;
  if (tid < SILREF_SUMS) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < SILREF_WAVES; w++) v += part[w][tid];
    if (v) atomicAdd(dst + tid, (unsigned long long)v);   // (two's complement: the 64-bit sum is that of the signed terms)
  } else if (tid < SILREF_WORDS) {
    const unsigned n = counts[tid - SILREF_SUMS];
    if (n) atomicAdd(dst + tid, (unsigned long long)n);
  }
}

}  // namespace

void launch_mask_signed_d2(hipStream_t s, const uint8_t *mask, const uint32_t *d2, int H, int W, int32_t *sd) {
  FP_GEOM_LOG("mask_signed_d2");
  const size_t px = (size_t)H * W;
  hipLaunchKernelGGL(mask_signed_d2, dim3((unsigned)((px + SILREF_THREADS - 1) / SILREF_THREADS)), dim3(SILREF_THREADS), 0, s, mask, d2, px, sd);
}

void launch_silref_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const float *depth,
                         const int32_t *sd, int H, int W, int gate2, float tol_m, bool occlusion, const SilrefParams *params, const int *flags,
                         int pose0, unsigned long long *acc) {
  FP_GEOM_LOG("silref_tile");
  if (n_items <= 0) return;
  const int ntx = scene_tiles_x(W);
  if (occlusion)
    hipLaunchKernelGGL(silref_tile<true>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, items, depth, sd, H, W, ntx,
                       gate2, tol_m, params, flags, pose0, acc);
  else
    hipLaunchKernelGGL(silref_tile<false>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, items, depth, sd, H, W, ntx,
                       gate2, tol_m, params, flags, pose0, acc);
}

}  // namespace fp
