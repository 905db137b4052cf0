// The raster rules of the frame-resolution renderers, each written once: fp_render_pose (fp_frame_render.hip),
// fp_render_scene (fp_scene_render.hip, section 4.9), fp_pose_vsd (fp_pose_vsd.hip, section 4.11), fp_refine_depth (fp_pose_icp.hip,
// section 4.12), fp_pose_color (fp_pose_color.hip, section 4.14) and fp_pose_silhouette (fp_pose_silhouette.hip, section 4.15) promise the
// same pixels because their kernels call these functions;
// and the tile engine around the rules, which the kernels that rasterise one mesh under one pose share.  Device code only, for files
// compiled with -ffp-contract=off: every f32 operation below is separately rounded, in the order written, and
// tests/frame_render_ref.py restates it operation by operation.  The 160x160 crop rasteriser of fp_geometry.hip has rules of its own.
#pragma once
#include "fp_internal.h"

namespace fp {

// vertex rule: p = R v + t, projection with K, snap to 1/16 px.  A vertex in front of the near constant, or one whose snapped
// coordinates would leave the exact range of the edge functions, returns its refusal bit and stores zeros (the host refuses the pose
// before a raster kernel is launched).  snap = {xi, yi, bits(z), 0}, cam = {x, y, z, 0}.
__device__ __forceinline__ int frame_vertex_rule(const float *__restrict__ verts, size_t i, const FramePose &P, int4 &snap, float4 &cam) {
  const float vx = verts[i * 3], vy = verts[i * 3 + 1], vz = verts[i * 3 + 2];
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
  snap = make_int4(xi, yi, __float_as_int(z), 0);
  cam = make_float4(x, y, z, 0.0f);
  return bad;
}

// top-left fill rule on an edge with direction (dx, dy) of a triangle of positive area (y grows downwards): a sample exactly on the
// edge belongs to the triangle when the edge is a left edge (dy < 0) or a top edge (dy == 0, dx > 0).  Returned as the smallest
// edge-function value that still counts as covered: 0 for such an edge, 1 for the others.
__device__ __forceinline__ long long edge_bias(long long dx, long long dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// pixels whose sample point (16 px, 16 py) lies inside the triangle's bounding box, clipped to [X0..X1] x [Y0..Y1] (a tile cut to the
// frame, or the whole frame); false when there is none
struct FrameBox {
  int px0, px1, py0, py1;
};
__device__ __forceinline__ bool frame_tri_box(const int4 &a, const int4 &b, const int4 &c, int X0, int Y0, int X1, int Y1, FrameBox &q) {
  q.px0 = max((min(a.x, min(b.x, c.x)) + 15) >> 4, X0); q.px1 = min(max(a.x, max(b.x, c.x)) >> 4, X1);
  q.py0 = max((min(a.y, min(b.y, c.y)) + 15) >> 4, Y0); q.py1 = min(max(a.y, max(b.y, c.y)) >> 4, Y1);
  return q.px0 <= q.px1 && q.py0 <= q.py1;
}
// twice the signed area, in 1/256 px^2; a triangle of area 0 covers nothing
__device__ __forceinline__ long long frame_tri_area(const int4 &a, const int4 &b, const int4 &c) {
  return (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
}

// triangle walk: hit(px, py, z) for every pixel of [X0..X1] x [Y0..Y1] whose sample point the triangle covers, z the perspective-
// correct depth there.  Edge functions are exact 64-bit integers, stepped incrementally along a row.
template <typename Hit>
__device__ __forceinline__ void frame_tri_walk(const int4 &a, const int4 &b, const int4 &c, int X0, int Y0, int X1, int Y1, Hit hit) {
  FrameBox q;
  if (!frame_tri_box(a, b, c, X0, Y0, X1, Y1, q)) return;
  const long long area = frame_tri_area(a, b, c);
  if (area == 0) return;
  const long long s = area < 0 ? -1 : 1, A = s * area;
  // edge i is opposite corner i: 0 = b -> c, 1 = c -> a, 2 = a -> b; both windings are brought to positive area by the sign s
  const long long d0x = s * (c.x - b.x), d0y = s * (c.y - b.y);
  const long long d1x = s * (a.x - c.x), d1y = s * (a.y - c.y);
  const long long d2x = s * (b.x - a.x), d2y = s * (b.y - a.y);
  const long long b0 = edge_bias(d0x, d0y), b1 = edge_bias(d1x, d1y), b2 = edge_bias(d2x, d2y);
  const float za = __int_as_float(a.z), zb = __int_as_float(b.z), zc = __int_as_float(c.z);
  const float fA = (float)A;
  const long long sx = 16ll * q.px0;
  for (int py = q.py0; py <= q.py1; py++) {
    const long long sy = 16ll * py;
    long long e0 = d0x * (sy - b.y) - d0y * (sx - b.x);
    long long e1 = d1x * (sy - c.y) - d1y * (sx - c.x);
    long long e2 = d2x * (sy - a.y) - d2y * (sx - a.x);
    for (int px = q.px0; px <= q.px1; px++, e0 -= 16 * d0y, e1 -= 16 * d1y, e2 -= 16 * d2y) {
      if (((e0 - b0) | (e1 - b1) | (e2 - b2)) < 0) continue;
      const float w0 = (float)e0 / fA, w1 = (float)e1 / fA, w2 = (float)e2 / fA;
      hit(px, py, 1.0f / ((w0 / za + w1 / zb) + w2 / zc));
    }
  }
}

// perspective-correct weights of the sample point (16 px, 16 py) in the triangle a, b, c that won the pixel with depth z (the key's):
// the edge functions as frame_tri_walk forms them (exact 64-bit integers, so stepping or recomputing gives the same values), the affine
// weights w_k = e_k / A as there, then g_k = (w_k / z_k) * z with z_k the corner depths.  An attribute q with corner values q_k is
// (g0 * q0 + g1 * q1) + g2 * q2 at the pixel (fp_pose_color).  The triangle has an area: it covered the sample.
struct FrameWeights {
  float g0, g1, g2;
};
__device__ __forceinline__ FrameWeights frame_tri_weights(const int4 &a, const int4 &b, const int4 &c, int px, int py, float z) {
  const long long area = frame_tri_area(a, b, c);
  const long long s = area < 0 ? -1 : 1, A = s * area;
  const long long d0x = s * (c.x - b.x), d0y = s * (c.y - b.y);
  const long long d1x = s * (a.x - c.x), d1y = s * (a.y - c.y);
  const long long d2x = s * (b.x - a.x), d2y = s * (b.y - a.y);
  const long long sx = 16ll * px, sy = 16ll * py;
  const long long e0 = d0x * (sy - b.y) - d0y * (sx - b.x);
  const long long e1 = d1x * (sy - c.y) - d1y * (sx - c.x);
  const long long e2 = d2x * (sy - a.y) - d2y * (sx - a.x);
  const float fA = (float)A;
  const float w0 = (float)e0 / fA, w1 = (float)e1 / fA, w2 = (float)e2 / fA;
  FrameWeights g;
  g.g0 = (w0 / __int_as_float(a.z)) * z;
  g.g1 = (w1 / __int_as_float(b.z)) * z;
  g.g2 = (w2 / __int_as_float(c.z)) * z;
  return g;
}

// ---- the pose-tile engine: what every kernel that rasterises ONE mesh under one pose into a FRAME_RENDER_TILE x FRAME_RENDER_TILE
// LDS z-buffer does before its own pixel loop (frame_raster_kernel, vsd_tile_kernel, icp_tile_kernel, color_tile_kernel, silhouette_tile): the tile's
// rectangle, the z-buffer's keys, the walk over all faces.  scene_raster_kernel walks per-tile lists of several objects instead of all faces of
// one; it shares the rectangle and the keys.

// the pixels [X0..X1] x [Y0..Y1] of tile (bx, by), cut to the H x W frame
struct FrameTile {
  int X0, Y0, X1, Y1;
};
__device__ __forceinline__ FrameTile frame_tile_rect(int bx, int by, int H, int W) {
  constexpr int T = FRAME_RENDER_TILE;
  return {bx * T, by * T, min(bx * T + T - 1, W - 1), min(by * T + T - 1, H - 1)};
}
// ... of tile number `tile` of a grid of ntx tiles per row
__device__ __forceinline__ FrameTile frame_tile_rect_of(int tile, int ntx, int H, int W) { return frame_tile_rect(tile % ntx, tile / ntx, H, W); }

// z-buffer keys.  EMPTY (an entry no triangle has reached) is larger than every key; positive floats order like their bit patterns, so
// the unsigned minimum of a key is the nearest depth -- and, with the triangle below the depth, the lowest triangle among equal depths.
// FrameKeyZ keeps the depth only: its minimum is the z of the FrameKeyZTri minimum.
struct FrameKeyZ {
  typedef unsigned type;
  static constexpr type EMPTY = ~0u;
  static __device__ __forceinline__ type pack(float z, unsigned) { return __float_as_uint(z); }
  static __device__ __forceinline__ float z(type key) { return __uint_as_float(key); }
};
struct FrameKeyZTri {
  typedef unsigned long long type;
  static constexpr type EMPTY = ~0ull;
  static __device__ __forceinline__ type pack(float z, unsigned tri) { return ((type)__float_as_uint(z) << 32) | tri; }
  static __device__ __forceinline__ float z(type key) { return __uint_as_float((unsigned)(key >> 32)); }
  static __device__ __forceinline__ unsigned tri(type key) { return (unsigned)key; }
};
template <typename Key>
__device__ __forceinline__ void frame_zbuf_clear(typename Key::type *zbuf, int tid) {
  for (int i = tid; i < FRAME_RENDER_TILE * FRAME_RENDER_TILE; i += FRAME_RENDER_THREADS) zbuf[i] = Key::EMPTY;
}
// the face walk: the workgroup's threads share the F faces of the mesh, skip a face with an index outside the V vertices, and
// rasterise the others (rejected by bounding box against the tile first) into the tile's z-buffer with an LDS atomic minimum.
// snap: the pose's own snapped vertices.  Barriers before (the clear) and after (the resolve) are the caller's.
template <typename Key>
__device__ __forceinline__ void frame_face_walk(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap, const FrameTile &r,
                                                typename Key::type *zbuf, int tid) {
  for (int t = tid; t < F; t += FRAME_RENDER_THREADS) {
    const int i0 = faces[(size_t)t * 3], i1 = faces[(size_t)t * 3 + 1], i2 = faces[(size_t)t * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const int4 a = snap[i0], b = snap[i1], c = snap[i2];
    frame_tri_walk(a, b, c, r.X0, r.Y0, r.X1, r.Y1, [&](int px, int py, float z) {
      atomicMin(&zbuf[(py - r.Y0) * FRAME_RENDER_TILE + (px - r.X0)], Key::pack(z, (unsigned)t));
    });
  }
}

// the body of a vertex pass: vertex i under pose P -> the snapped vertex *snap and, where cam is not null (something is shaded, or a
// normal is needed), its camera-space copy *cam; a refused vertex raises its bit of *flag.
__device__ __forceinline__ void frame_vertex_store(const float *__restrict__ verts, int i, const FramePose &P, int4 *__restrict__ snap,
                                                   float4 *__restrict__ cam, int *__restrict__ flag) {
  int4 sn;
  float4 cm;
  const int bad = frame_vertex_rule(verts, (size_t)i, P, sn, cm);
  *snap = sn;
  if (cam) *cam = cm;
  if (bad) atomicOr(flag, bad);
}

// a model pixel at depth z is hidden when something valid was observed more than tol in front of it (D is the RAW observed depth)
__device__ __forceinline__ bool frame_occluded(float D, float z, float tol) { return !(D < FP_MIN_DEPTH) && D < z - tol; }

// flat Lambert term of a triangle's camera-space normal (two-sided), quantised to the integer shade k in [64, 255]
__device__ __forceinline__ int frame_shade(const float4 &p0, const float4 &p1, const float4 &p2) {
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const float len2 = (nx * nx + ny * ny) + nz * nz;
  const float lam = len2 > 0.0f ? fabsf(nz) / sqrtf(len2) : 0.0f;
  return 64 + (int)rintf(lam * 191.0f);
}
// one channel of the overlay: the frame's colour c and the tint scaled by the shade k, averaged with rounding
__device__ __forceinline__ int frame_tint(int c, int tint, int k) { return (c + (tint * k + 127) / 255 + 1) >> 1; }

}  // namespace fp
