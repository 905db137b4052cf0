// Frame-resolution rendering of one pose (fp_render_pose): model depth, model / visible masks, triangle ids and
// a flat-shaded overlay at the size of the uploaded frame.  Two kernels: index bookkeeping, the tile's z-buffer and the output planes
// are here, every rule that decides a pixel is in fp_frame_rules.h, shared with fp_scene_render.hip.  Compiled with
// -ffp-contract=off like the rest of the geometry.
#include "fp_frame_rules.h"

#include <algorithm>
#include <cmath>

namespace fp {

namespace {

// (a) vertex pass: the vertex rule per vertex; a refused vertex raises its bit of its pose's word.  Two forms of one body
// (frame_vertex_store): fp_render_pose's one pose arrives by value as a kernel argument, so that call uploads nothing; the batched form
// takes its poses from device memory, pose p of the launch (blockIdx.y) being poses_a[p] for p < n_a and poses_b[p - n_a] beyond,
// writes pose p's vertices at snap[p V ..] (cam likewise, null: not stored) and raises flags_a[p] or flags_b[p - n_a].
__global__ __launch_bounds__(256) void frame_vertex_kernel(const float *__restrict__ verts, int V, FramePose P, int4 *__restrict__ snap,
                                                           float4 *__restrict__ cam, int *__restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  frame_vertex_store(verts, i, P, snap + i, cam ? cam + i : nullptr, flag);
}
__global__ __launch_bounds__(256) void pose_vertex_kernel(const float *__restrict__ verts, int V, const FramePose *__restrict__ poses_a, int n_a,
                                                          const FramePose *__restrict__ poses_b, int4 *__restrict__ snap, float4 *__restrict__ cam,
                                                          int *__restrict__ flags_a, int *__restrict__ flags_b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
  if (i >= V) return;
  const size_t at = (size_t)p * V + i;
  frame_vertex_store(verts, i, p < n_a ? poses_a[p] : poses_b[p - n_a], snap + at, cam ? cam + at : nullptr, p < n_a ? flags_a + p : flags_b + (p - n_a));
}

// (b) raster + resolve: one workgroup per FRAME_RENDER_TILE x FRAME_RENDER_TILE pixel tile.  The tile's z-buffer is 64-bit keys
// bits(z) << 32 | triangle in LDS (8 KB), resolved with ds_min_u64; the threads walk all triangles, reject by bounding box against the
// tile and rasterise the rest (frame_face_walk).  After the barrier every requested output of the tile is written once.  Tiles outside
// [tx0, tx1] x [ty0, ty1] (the host's conservative screen bound of the object) skip the walk and write background.
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void frame_raster_kernel(const int32_t *__restrict__ faces, int F, int V,
                                                                            const int4 *__restrict__ snap, const float4 *__restrict__ cam,
                                                                            const uint8_t *__restrict__ rgb, const float *__restrict__ obs,
                                                                            int H, int W, int tx0, int ty0, int tx1, int ty1, float tol,
                                                                            FrameRenderOut o) {
  typedef FrameKeyZTri Key;
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zbuf[T * T];
  const int tid = threadIdx.x;
  const FrameTile rect = frame_tile_rect((int)blockIdx.x, (int)blockIdx.y, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  frame_zbuf_clear<Key>(zbuf, tid);
  __syncthreads();
  const bool walk = (int)blockIdx.x >= tx0 && (int)blockIdx.x <= tx1 && (int)blockIdx.y >= ty0 && (int)blockIdx.y <= ty1;   // uniform
  if (walk) frame_face_walk<Key>(faces, F, V, snap, rect, zbuf, tid);
  __syncthreads();
  for (int i = tid; i < T * T; i += FRAME_RENDER_THREADS) {
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    if (px >= W || py >= H) continue;
    const size_t at = (size_t)py * W + px;
    const Key::type key = zbuf[i];
    const bool model = key != Key::EMPTY;
    const float z = model ? Key::z(key) : 0.0f;
    const int tri = model ? (int)Key::tri(key) : -1;
    bool visible = model;
    if (model && (o.vis || o.overlay)) visible = !frame_occluded(obs[at], z, tol);   // something observed in front of the model?
    if (o.depth) o.depth[at] = z;
    if (o.mask) o.mask[at] = model ? 255 : 0;
    if (o.vis) o.vis[at] = visible ? 255 : 0;
    if (o.tri) o.tri[at] = tri + 1;
    if (o.overlay) {
      int r = rgb[at * 3], g = rgb[at * 3 + 1], bl = rgb[at * 3 + 2];
      if (visible) {
        const int k = frame_shade(cam[faces[(size_t)tri * 3]], cam[faces[(size_t)tri * 3 + 1]], cam[faces[(size_t)tri * 3 + 2]]);
        r = frame_tint(r, FRAME_RENDER_TINT_R, k); g = frame_tint(g, FRAME_RENDER_TINT_G, k); bl = frame_tint(bl, FRAME_RENDER_TINT_B, k);
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

void launch_pose_vertices(hipStream_t s, const char *log_name, const DeviceMesh &m, const FramePose *poses_a, int n_a, const FramePose *poses_b, int n_b,
                          int4 *snap, float4 *cam, int *flags_a, int *flags_b) {
  FP_GEOM_LOG(log_name);
  if (n_a + n_b <= 0 || m.V <= 0) return;
  hipLaunchKernelGGL(pose_vertex_kernel, dim3((unsigned)((m.V + 255) / 256), (unsigned)(n_a + n_b)), dim3(256), 0, s, m.verts, m.V, poses_a, n_a, poses_b,
                     snap, cam, flags_a, flags_b);
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
