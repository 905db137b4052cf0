// Projective point-to-plane ICP of N poses on the observed depth (fp_refine_depth): the device half.  Two kernels:
// the batched vertex pass over (pose, vertex), which keeps the snapped and the camera-space vertex, and here a tile kernel over (pose, tile) items that
// rasterises the pose into a 64-bit LDS z-buffer exactly as frame_raster_kernel does, associates every model pixel with the observed
// depth, and reduces the 6 x 6 normal system of the pose as 28 integer sums plus six pixel counts.  Every rule that decides the depth
// and the triangle of a pixel is fp_frame_rules.h's; the rules of the residual are icp_pixel below.  Compiled with -ffp-contract=off
// like the rest of the geometry: every f32 operation is separately rounded, tests/icp_ref.py restates them.  The solve is the host's.
#include "fp_frame_rules.h"

namespace fp {

namespace {

typedef FrameKeyZTri Key;   // the normals need the winning triangle: frame_raster_kernel's 64-bit keys
constexpr int ICP_PX_PER_THREAD = FRAME_RENDER_TILE * FRAME_RENDER_TILE / FRAME_RENDER_THREADS;
constexpr int ICP_WAVES = FRAME_RENDER_THREADS / 64;

// (a) the vertex pass is launch_pose_vertices' (fp_frame_render.hip): the poses of a chunk, the snapped vertex and its camera-space
// copy (the normals need it).

// the rules of the residual at one pixel (c, r) of a model pixel: z the model depth, p0 p1 p2 the winning triangle's camera-space
// corners, D the RAW observed depth.  cls: 0 not valid, 1 used, 2 front, 3 behind, 4 grazing; J and e are set when used.
struct IcpPixel {
  int cls;
  float J[6], e;
};
__device__ __forceinline__ IcpPixel icp_pixel(int c, int r, float z, const float4 &p0, const float4 &p1, const float4 &p2, float D, const IcpParams &P) {
  IcpPixel o;
  o.cls = 0;
  if (!(D >= FP_MIN_DEPTH) || !(D <= 3.402823466e+38f)) return o;   // missing, NaN or infinite
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const float len2 = (nx * nx + ny * ny) + nz * nz;
  const bool flat = !(len2 > 0.0f);   // no normal: never used (s = 0 makes it grazing unless it is front or behind)
  const float len = sqrtf(len2);
  const float hx = flat ? 0.0f : nx / len, hy = flat ? 0.0f : ny / len, hz = flat ? 0.0f : nz / len;
  const float X = ((float)c - P.cx) / P.fx, Y = ((float)r - P.cy) / P.fy;
  const float l = sqrtf((X * X + Y * Y) + 1.0f);
  const float s = (hx * X + hy * Y) + hz;
  const float dz = D - z;
  const float along = dz * l;
  if (along < -P.max_dist) { o.cls = 2; return o; }
  if (along > P.max_dist) { o.cls = 3; return o; }
  if (fabsf(s) / l < ICP_MIN_COS) { o.cls = 4; return o; }
  o.cls = 1;
  o.e = (dz * s) / P.rad;
  const float qx = D * X, qy = D * Y, qz = D;
  const float cx = (qx - P.t[0]) / P.rad, cy = (qy - P.t[1]) / P.rad, cz = (qz - P.t[2]) / P.rad;
  o.J[0] = cy * hz - cz * hy; o.J[1] = cz * hx - cx * hz; o.J[2] = cx * hy - cy * hx;
  o.J[3] = hx; o.J[4] = hy; o.J[5] = hz;
  return o;
}

__device__ __forceinline__ long long icp_q32(float v) { return llrintf(v * 4294967296.0f); }   // (the scaling is exact)

// (b) tile kernel: one workgroup per item {pose of the launch's chunk, tile}.  params / flags / acc are indexed by pose0 + pose.
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void icp_tile_kernel(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap,
                                                                        const float4 *__restrict__ cam, const int2 *__restrict__ items,
                                                                        const float *__restrict__ obs, int H, int W, int ntx,
                                                                        const IcpParams *__restrict__ params, const int *__restrict__ flags, int pose0,
                                                                        unsigned long long *__restrict__ acc) {
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zbuf[T * T];
  __shared__ long long part[ICP_WAVES][ICP_SUMS];
  __shared__ unsigned counts[ICP_COUNTS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  if (flags[pose0 + pose]) return;   // (uniform) a refused pose: its vertices were not stored, the host drops its record
  const FrameTile rect = frame_tile_rect_of(tile, ntx, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  frame_zbuf_clear<Key>(zbuf, tid);
  if (tid < ICP_COUNTS) counts[tid] = 0;
  __syncthreads();
  const float4 *__restrict__ cm = cam + (size_t)pose * V;
  frame_face_walk<Key>(faces, F, V, snap + (size_t)pose * V, rect, zbuf, tid);
  __syncthreads();
  const IcpParams P = params[pose0 + pose];
  long long sum[ICP_SUMS];
#pragma unroll
  for (int j = 0; j < ICP_SUMS; j++) sum[j] = 0;
  unsigned n_model = 0, n_valid = 0, n_used = 0, n_front = 0, n_behind = 0, n_grazing = 0;   // wave-uniform
#pragma unroll
  for (int k = 0; k < ICP_PX_PER_THREAD; k++) {
    const int i = k * FRAME_RENDER_THREADS + tid;
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const bool in = px < W && py < H;
    const Key::type key = zbuf[i];
    const bool model = in && key != Key::EMPTY;   // (a key exists only for a triangle whose three indices are below V)
    IcpPixel q;
    q.cls = 0;
    if (model) {
      const float z = Key::z(key);
      const size_t tri = (size_t)Key::tri(key);
      q = icp_pixel(px, py, z, cm[faces[tri * 3]], cm[faces[tri * 3 + 1]], cm[faces[tri * 3 + 2]], obs[(size_t)py * W + px], P);
    }
    n_model += wave_count(model); n_valid += wave_count(q.cls != 0);
    n_used += wave_count(q.cls == 1); n_front += wave_count(q.cls == 2);
    n_behind += wave_count(q.cls == 3); n_grazing += wave_count(q.cls == 4);
    if (q.cls == 1) {
      int j = 0;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) sum[j++] += icp_q32(q.J[a] * q.J[b]);
#pragma unroll
      for (int a = 0; a < 6; a++) sum[21 + a] += icp_q32(q.J[a] * q.e);
      sum[27] += icp_q32(q.e * q.e);
    }
  }
  // per wave, then across the four waves through LDS, then one integer atomic per quantity: integer sums do not depend on the order
  const int wave = tid >> 6, lane = tid & 63;
  if (n_used) {   // (uniform)
#pragma unroll
    for (int j = 0; j < ICP_SUMS; j++) {
      long long v = sum[j];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      sum[j] = v;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < ICP_SUMS; j++) part[wave][j] = sum[j];
    const unsigned six[ICP_COUNTS] = {n_model, n_valid, n_used, n_front, n_behind, n_grazing};
#pragma unroll
    for (int j = 0; j < ICP_COUNTS; j++)
      if (six[j]) atomicAdd(&counts[j], six[j]);
  }
  __syncthreads();
  unsigned long long *dst = acc + (size_t)(pose0 + pose) * ICP_WORDS;
  if (tid < ICP_SUMS) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < ICP_WAVES; w++) v += part[w][tid];
    if (v) atomicAdd(dst + tid, (unsigned long long)v);   // (two's complement: the 64-bit sum is that of the signed terms)
  } else if (tid < ICP_WORDS) {
    const unsigned n = counts[tid - ICP_SUMS];
    if (n) atomicAdd(dst + tid, (unsigned long long)n);
  }
}

}  // namespace

void launch_icp_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const float4 *cam, const int2 *items, int n_items, const float *depth,
                      int H, int W, const IcpParams *params, const int *flags, int pose0, unsigned long long *acc) {
  FP_GEOM_LOG("icp_tile");
  if (n_items <= 0) return;
  const int ntx = scene_tiles_x(W);
  hipLaunchKernelGGL(icp_tile_kernel, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, cam, items, depth, H, W, ntx, params,
                     flags, pose0, acc);
}

}  // namespace fp
