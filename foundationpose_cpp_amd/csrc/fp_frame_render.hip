// Frame-resolution rendering of one pose (fp_render_pose): model depth, model / visible masks, triangle ids and
// a flat-shaded overlay at the size of the uploaded frame.  Two kernels, both new; nothing here is shared with the 160x160 crop
// rasteriser of fp_geometry.hip.  Compiled with -ffp-contract=off like the rest of the geometry: every f32 operation below is
// separately rounded, in the order written, and tests/frame_render_ref.py restates it operation by operation.
#include "fp_internal.h"

#include <algorithm>
#include <cmath>

namespace fp {

namespace {

constexpr unsigned long long FR_EMPTY = ~0ull;   // a z-buffer entry no triangle has reached: larger than every key

// (a) vertex pass: p = R v + t, projection with K, snap to 1/16 px.  A vertex in front of the near constant, or one whose snapped
// coordinates would leave the exact range of the edge functions, raises its bit of *flag and stores zeros (the host refuses the pose
// before the raster kernel is launched).
__global__ __launch_bounds__(256) void frame_vertex_kernel(const float *__restrict__ verts, int V, FramePose P, int4 *__restrict__ snap,
                                                           float4 *__restrict__ cam, int *__restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const float vx = verts[(size_t)i * 3], vy = verts[(size_t)i * 3 + 1], vz = verts[(size_t)i * 3 + 2];
  const float x = ((P.r[0] * vx + P.r[1] * vy) + P.r[2] * vz) + P.t[0];
  const float y = ((P.r[3] * vx + P.r[4] * vy) + P.r[5] * vz) + P.t[1];
  const float z = ((P.r[6] * vx + P.r[7] * vy) + P.r[8] * vz) + P.t[2];
  int bad = 0;
  int xi = 0, yi = 0;
  if (!(z >= FRAME_RENDER_NEAR)) bad |= FRAME_RENDER_FLAG_NEAR;   // (also a NaN)
  else {
    const float u = P.fx * (x / z) + P.cx;
    const float w = P.fy * (y / z) + P.cy;
    const float us = u * 16.0f, ws = w * 16.0f;
    if (!(fabsf(us) <= (float)FRAME_RENDER_SNAP_MAX) || !(fabsf(ws) <= (float)FRAME_RENDER_SNAP_MAX)) bad |= FRAME_RENDER_FLAG_RANGE;
    else { xi = (int)rintf(us); yi = (int)rintf(ws); }
  }
  snap[i] = make_int4(xi, yi, __float_as_int(z), 0);
  cam[i] = make_float4(x, y, z, 0.0f);
  if (bad) atomicOr(flag, bad);
}

// top-left fill rule on an edge with direction (dx, dy) of a triangle of positive area (y grows downwards): a sample exactly on the
// edge belongs to the triangle when the edge is a left edge (dy < 0) or a top edge (dy == 0, dx > 0).  Returned as the smallest
// edge-function value that still counts as covered: 0 for such an edge, 1 for the others.
__device__ __forceinline__ long long edge_bias(long long dx, long long dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// (b) raster + resolve: one workgroup per FRAME_RENDER_TILE x FRAME_RENDER_TILE pixel tile.  The tile's z-buffer is 64-bit keys
// bits(z) << 32 | triangle in LDS (8 KB), resolved with ds_min_u64; the threads walk all triangles, reject by bounding box against the
// tile and rasterise the rest.  After the barrier every requested output of the tile is written once.  Tiles outside
// [tx0, tx1] x [ty0, ty1] (the host's conservative screen bound of the object) skip the walk and write background.
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void frame_raster_kernel(const int32_t *__restrict__ faces, int F, int V,
                                                                            const int4 *__restrict__ snap, const float4 *__restrict__ cam,
                                                                            const uint8_t *__restrict__ rgb, const float *__restrict__ obs,
                                                                            int H, int W, int tx0, int ty0, int tx1, int ty1, float tol,
                                                                            FrameRenderOut o) {
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ unsigned long long zbuf[T * T];
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * T, Y0 = blockIdx.y * T;
  const int X1 = min(X0 + T - 1, W - 1), Y1 = min(Y0 + T - 1, H - 1);
  for (int i = tid; i < T * T; i += FRAME_RENDER_THREADS) zbuf[i] = FR_EMPTY;
  __syncthreads();
  const bool walk = (int)blockIdx.x >= tx0 && (int)blockIdx.x <= tx1 && (int)blockIdx.y >= ty0 && (int)blockIdx.y <= ty1;   // uniform
  if (walk) {
    for (int t = tid; t < F; t += FRAME_RENDER_THREADS) {
      const int i0 = faces[(size_t)t * 3], i1 = faces[(size_t)t * 3 + 1], i2 = faces[(size_t)t * 3 + 2];
      if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
      const int4 a = snap[i0], b = snap[i1], c = snap[i2];
      // pixels whose sample point (16 px, 16 py) lies inside the triangle's bounding box, clipped to the tile and the frame
      const int px0 = max((min(a.x, min(b.x, c.x)) + 15) >> 4, X0), px1 = min(max(a.x, max(b.x, c.x)) >> 4, X1);
      const int py0 = max((min(a.y, min(b.y, c.y)) + 15) >> 4, Y0), py1 = min(max(a.y, max(b.y, c.y)) >> 4, Y1);
      if (px0 > px1 || py0 > py1) continue;
      const long long area = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
      if (area == 0) continue;
      const long long s = area < 0 ? -1 : 1, A = s * area;
      // edge i is opposite corner i: 0 = b -> c, 1 = c -> a, 2 = a -> b; both windings are brought to positive area by the sign s
      const long long d0x = s * (c.x - b.x), d0y = s * (c.y - b.y);
      const long long d1x = s * (a.x - c.x), d1y = s * (a.y - c.y);
      const long long d2x = s * (b.x - a.x), d2y = s * (b.y - a.y);
      const long long b0 = edge_bias(d0x, d0y), b1 = edge_bias(d1x, d1y), b2 = edge_bias(d2x, d2y);
      const float za = __int_as_float(a.z), zb = __int_as_float(b.z), zc = __int_as_float(c.z);
      const float fA = (float)A;
      const long long sx = 16ll * px0;
      for (int py = py0; py <= py1; py++) {
        const long long sy = 16ll * py;
        long long e0 = d0x * (sy - b.y) - d0y * (sx - b.x);
        long long e1 = d1x * (sy - c.y) - d1y * (sx - c.x);
        long long e2 = d2x * (sy - a.y) - d2y * (sx - a.x);
        for (int px = px0; px <= px1; px++, e0 -= 16 * d0y, e1 -= 16 * d1y, e2 -= 16 * d2y) {
          if (((e0 - b0) | (e1 - b1) | (e2 - b2)) < 0) continue;
          const float w0 = (float)e0 / fA, w1 = (float)e1 / fA, w2 = (float)e2 / fA;
          const float z = 1.0f / ((w0 / za + w1 / zb) + w2 / zc);
          const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)t;
          atomicMin(&zbuf[(py - Y0) * T + (px - X0)], key);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < T * T; i += FRAME_RENDER_THREADS) {
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    if (px >= W || py >= H) continue;
    const size_t at = (size_t)py * W + px;
    const unsigned long long key = zbuf[i];
    const bool model = key != FR_EMPTY;
    const float z = model ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    const int tri = model ? (int)(unsigned)key : -1;
    bool visible = model;
    if (model && (o.vis || o.overlay)) {
      const float D = obs[at];
      if (!(D < FP_MIN_DEPTH) && D < z - tol) visible = false;   // something observed in front of the model
    }
    if (o.depth) o.depth[at] = z;
    if (o.mask) o.mask[at] = model ? 255 : 0;
    if (o.vis) o.vis[at] = visible ? 255 : 0;
    if (o.tri) o.tri[at] = tri + 1;
    if (o.overlay) {
      int r = rgb[at * 3], g = rgb[at * 3 + 1], bl = rgb[at * 3 + 2];
      if (visible) {
        // flat Lambert term of the triangle's camera-space normal (two-sided), quantised to the integer shade k in [64, 255]
        const float4 p0 = cam[faces[(size_t)tri * 3]], p1 = cam[faces[(size_t)tri * 3 + 1]], p2 = cam[faces[(size_t)tri * 3 + 2]];
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
        const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float len2 = (nx * nx + ny * ny) + nz * nz;
        const float lam = len2 > 0.0f ? fabsf(nz) / sqrtf(len2) : 0.0f;
        const int k = 64 + (int)rintf(lam * 191.0f);
        r = (r + (FRAME_RENDER_TINT_R * k + 127) / 255 + 1) >> 1;
        g = (g + (FRAME_RENDER_TINT_G * k + 127) / 255 + 1) >> 1;
        bl = (bl + (FRAME_RENDER_TINT_B * k + 127) / 255 + 1) >> 1;
      }
      o.overlay[at * 3] = (uint8_t)r; o.overlay[at * 3 + 1] = (uint8_t)g; o.overlay[at * 3 + 2] = (uint8_t)bl;
    }
  }
}

}  // namespace

void launch_frame_vertex(hipStream_t s, const DeviceMesh &m, const FramePose &pose, int4 *snap, float4 *cam, int *flag) {
  FP_GEOM_LOG("frame_vertex");
  hipLaunchKernelGGL(frame_vertex_kernel, dim3((unsigned)((m.V + 255) / 256)), dim3(256), 0, s, m.verts, m.V, pose, snap, cam, flag);
}

void launch_frame_raster(hipStream_t s, const DeviceMesh &m, const int4 *snap, const float4 *cam, const uint8_t *rgb, const float *depth,
                         int H, int W, const FrameTileBound &b, float tol_m, const FrameRenderOut &out) {
  FP_GEOM_LOG("frame_raster");
  const dim3 grid((unsigned)((W + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE), (unsigned)((H + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE));
  hipLaunchKernelGGL(frame_raster_kernel, grid, dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, cam, rgb, depth, H, W, b.tx0, b.ty0,
                     b.tx1, b.ty1, tol_m, out);
}

// The tiles the object can reach: the projection of the box around the sphere of radius `radius` about the pose's translation (every
// vertex of the centred mesh lies inside that sphere once `radius` is the largest vertex norm times a bound of the pose's linear part),
// grown by two pixels and evaluated in double.  A sphere that reaches the near constant, or any non-finite input, gives the whole
// frame: the bound only ever spares work, it never decides a pixel.
FrameTileBound frame_tile_bound(const FramePose &P, double radius, int H, int W) {
  const int ntx = (W + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE, nty = (H + FRAME_RENDER_TILE - 1) / FRAME_RENDER_TILE;
  FrameTileBound whole = {0, 0, ntx - 1, nty - 1};
  // spectral norm of the linear part <= sqrt of the largest absolute row sum of R^T R (1 for a rotation)
  double nrm = 0;
  for (int i = 0; i < 3; i++) {
    double row = 0;
    for (int j = 0; j < 3; j++) {
      double d = 0;
      for (int k = 0; k < 3; k++) d += (double)P.r[k * 3 + i] * (double)P.r[k * 3 + j];
      row += std::fabs(d);
    }
    nrm = std::max(nrm, row);
  }
  const double r = radius * std::sqrt(nrm) * (1.0 + 1e-4) + 1e-6;
  const double tx = P.t[0], ty = P.t[1], tz = P.t[2];
  if (!std::isfinite(r) || !std::isfinite(tx) || !std::isfinite(ty) || !std::isfinite(tz)) return whole;
  const double zn = tz - r, zf = tz + r;
  if (!(zn > (double)FRAME_RENDER_NEAR)) return whole;
  const double xl = std::min((tx - r) / zn, (tx - r) / zf), xh = std::max((tx + r) / zn, (tx + r) / zf);
  const double yl = std::min((ty - r) / zn, (ty - r) / zf), yh = std::max((ty + r) / zn, (ty + r) / zf);
  const double u0 = (double)P.fx * xl + P.cx - 2.0, u1 = (double)P.fx * xh + P.cx + 2.0;
  const double w0 = (double)P.fy * yl + P.cy - 2.0, w1 = (double)P.fy * yh + P.cy + 2.0;
  if (!std::isfinite(u0) || !std::isfinite(u1) || !std::isfinite(w0) || !std::isfinite(w1) || P.fx < 0 || P.fy < 0) return whole;
  // (clamped before the conversion to int; a bound that misses the frame leaves an empty range: every tile writes background)
  FrameTileBound b;
  b.tx0 = (int)std::floor(std::min(std::max(u0, 0.0), (double)ntx * FRAME_RENDER_TILE) / FRAME_RENDER_TILE);
  b.ty0 = (int)std::floor(std::min(std::max(w0, 0.0), (double)nty * FRAME_RENDER_TILE) / FRAME_RENDER_TILE);
  b.tx1 = u1 < 0 ? -1 : (int)std::min<double>(std::floor(u1 / FRAME_RENDER_TILE), ntx - 1);
  b.ty1 = w1 < 0 ? -1 : (int)std::min<double>(std::floor(w1 / FRAME_RENDER_TILE), nty - 1);
  return b;
}

}  // namespace fp
