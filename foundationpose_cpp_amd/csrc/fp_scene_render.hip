// Frame-resolution rendering of all tracked objects of a frame in one pass (fp_render_scene): nearest model depth,
// instance map, visible mask, triangle ids, the amodal coverage word of every pixel, a per-object tinted overlay and the per-object
// pixel counts.  Per object the rules are fp_render_pose's: both call fp_frame_rules.h (the same -ffp-contract=off); what is added
// here is that the triangles of all objects are binned into the 32 x 32 px tiles first, so a tile walks only its own list, and that
// the objects meet in one z-buffer whose keys carry the GLOBAL triangle index.  tests/scene_render_ref.py restates the rules.
#include "fp_frame_rules.h"

namespace fp {

namespace {

typedef FrameKeyZTri Key;   // the z-buffer's keys; the triangle they carry is the GLOBAL index g

// the object that owns global index g: the last o with start[o] <= g (objects without vertices / faces own nothing)
template <typename I>
__device__ __forceinline__ int scene_owner(const I *start, int K, I g) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// (a) vertex pass over the concatenated vertices of all objects: the vertex rule with the owner's pose; one refusal word per object.
__global__ __launch_bounds__(256) void scene_vertex_kernel(const SceneTable *__restrict__ tb, int total, int4 *__restrict__ snap,
                                                           float4 *__restrict__ cam, int *__restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int o = scene_owner(tb->vert_start, tb->K, i);
  const int bad = frame_vertex_rule(tb->verts[o], (size_t)(i - tb->vert_start[o]), tb->pose[o], snap[i], cam[i]);
  if (bad) atomicOr(flags + o, bad);
}

// The corners of global triangle g and its owner; false for a face with an index outside the owner's vertices.
struct SceneTri {
  int4 a, b, c;
  int o;
  int i0, i1, i2;   // scene vertex indices
};
__device__ __forceinline__ bool scene_load_tri(const SceneTable *__restrict__ tb, const int *vert_start, const unsigned *face_start, int K,
                                               const int4 *__restrict__ snap, unsigned g, SceneTri &t) {
  t.o = scene_owner(face_start, K, g);
  const int32_t *f = tb->faces[t.o] + (size_t)(g - face_start[t.o]) * 3;
  const int base = vert_start[t.o], V = vert_start[t.o + 1] - base;
  const int i0 = f[0], i1 = f[1], i2 = f[2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  t.i0 = base + i0; t.i1 = base + i1; t.i2 = base + i2;
  t.a = snap[t.i0]; t.b = snap[t.i1]; t.c = snap[t.i2];
  return true;
}

// (b) binning.  The tiles of triangle g: those its bounding box of sample points reaches, the triangle walk's own box and area tests
// with the whole frame as the clip rectangle; none for a bad face, zero area or a box that misses the frame.  FILL = false counts per tile, FILL = true appends g to the
// lists at the cursors the scan left.  Neighbouring triangles of a mesh fall into the same few tiles, and one global atomic per
// (tile, triangle) pair serialises on those few addresses; so a workgroup first counts its 256 triangles per tile in LDS and then
// claims, per tile it touched, its whole share with ONE global atomic.  The LDS histogram holds SC_BIN_CHUNK tiles (all 2040 of a
// 1920 x 1080 frame); a larger grid is walked chunk after chunk.
constexpr int SC_BIN_CHUNK = 2048;
template <bool FILL>
__global__ __launch_bounds__(256) void scene_bin_kernel(const SceneTable *__restrict__ tb, unsigned total, const int4 *__restrict__ snap,
                                                        int H, int W, int ntx, int ntiles, unsigned *__restrict__ count_or_cursor,
                                                        unsigned *__restrict__ list) {
  __shared__ unsigned hist[SC_BIN_CHUNK];
  __shared__ unsigned base[FILL ? SC_BIN_CHUNK : 1];
  const int tid = threadIdx.x;
  const unsigned g = blockIdx.x * blockDim.x + tid;
  int tx0 = 0, tx1 = -1, ty0 = 0, ty1 = -1;   // (empty: the thread still meets every barrier)
  SceneTri t;
  if (g < total && scene_load_tri(tb, tb->vert_start, tb->face_start, tb->K, snap, g, t)) {
    FrameBox q;
    if (frame_tri_box(t.a, t.b, t.c, 0, 0, W - 1, H - 1, q) && frame_tri_area(t.a, t.b, t.c) != 0) {   // inside the grid: 0 <= p < W, H
      tx0 = q.px0 / FRAME_RENDER_TILE; tx1 = q.px1 / FRAME_RENDER_TILE; ty0 = q.py0 / FRAME_RENDER_TILE; ty1 = q.py1 / FRAME_RENDER_TILE;
    }
  }
  for (int c0 = 0; c0 < ntiles; c0 += SC_BIN_CHUNK) {   // uniform
    const int n = min(SC_BIN_CHUNK, ntiles - c0);
    for (int i = tid; i < n; i += 256) hist[i] = 0;
    __syncthreads();
    for (int ty = ty0; ty <= ty1; ty++)
      for (int tx = tx0; tx <= tx1; tx++) {
        const int tile = ty * ntx + tx - c0;
        if (tile >= 0 && tile < n) atomicAdd(&hist[tile], 1u);
      }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const unsigned k = hist[i];
      if (k) {
        const unsigned at = atomicAdd(count_or_cursor + c0 + i, k);
        if (FILL) base[i] = at;
      }
      if (FILL) hist[i] = 0;
    }
    if (FILL) {
      __syncthreads();
      for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) {
          const int tile = ty * ntx + tx - c0;
          if (tile >= 0 && tile < n) list[base[tile] + atomicAdd(&hist[tile], 1u)] = g;
        }
    }
    __syncthreads();
  }
}

// exclusive scan of the per-tile counts by ONE workgroup: thread i sums a contiguous run of tiles, the 256 partial sums are scanned in
// LDS, then every thread writes its run's offsets.  offset[ntiles] (32 bits) and *total (64 bits, what the host checks) = all entries.
__global__ __launch_bounds__(256) void scene_scan_kernel(const unsigned *__restrict__ count, int ntiles, unsigned *__restrict__ offset,
                                                         unsigned *__restrict__ cursor, unsigned long long *__restrict__ total) {
  __shared__ unsigned long long part[256];
  const int tid = threadIdx.x;
  const int run = (ntiles + 255) / 256;
  const int t0 = min(tid * run, ntiles), t1 = min(t0 + run, ntiles);
  unsigned long long sum = 0;
  for (int t = t0; t < t1; t++) sum += count[t];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned long long add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  unsigned long long at = part[tid] - sum;   // exclusive
  for (int t = t0; t < t1; t++) {
    offset[t] = (unsigned)at;
    cursor[t] = (unsigned)at;
    at += count[t];
  }
  if (tid == 255) {
    offset[ntiles] = (unsigned)part[255];
    *total = part[255];
  }
}

// (c) raster + resolve: one workgroup per tile walks the tile's list.  LDS: the tile's z-buffer of 64-bit keys bits(z) << 32 | g
// (ds_min_u64), its coverage words (bit o: a triangle of object o covers the sample; 64-bit LDS OR), the offset tables and 64 x 3
// counters.  After the barrier every requested output of the tile is written once and the tile's per-object counts are added to the
// call's counters.  A tile with an empty list writes background and adds nothing.
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void scene_raster_kernel(const SceneTable *__restrict__ tb, const int4 *__restrict__ snap,
                                                                            const float4 *__restrict__ cam, const unsigned *__restrict__ offset,
                                                                            const unsigned *__restrict__ list, const uint8_t *__restrict__ rgb,
                                                                            const float *__restrict__ obs, int H, int W, float tol, SceneRenderOut out) {
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zbuf[T * T];
  __shared__ unsigned long long cover[T * T];
  __shared__ unsigned long long present;                    // objects with an entry in this tile's list
  __shared__ unsigned face_start[SCENE_MAX_OBJECTS + 1];
  __shared__ int vert_start[SCENE_MAX_OBJECTS + 1];
  __shared__ int cnt[SCENE_MAX_OBJECTS * 3];
  const int tid = threadIdx.x;
  const int K = tb->K;
  const FrameTile rect = frame_tile_rect((int)blockIdx.x, (int)blockIdx.y, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0, X1 = rect.X1, Y1 = rect.Y1;
  const unsigned tile = blockIdx.y * gridDim.x + blockIdx.x;
  const unsigned l0 = offset[tile], l1 = offset[tile + 1];   // uniform
  if (l0 != l1) {
    for (int i = tid; i < T * T; i += FRAME_RENDER_THREADS) { zbuf[i] = Key::EMPTY; cover[i] = 0; }
    for (int i = tid; i <= K; i += FRAME_RENDER_THREADS) { face_start[i] = tb->face_start[i]; vert_start[i] = tb->vert_start[i]; }
    for (int i = tid; i < SCENE_MAX_OBJECTS * 3; i += FRAME_RENDER_THREADS) cnt[i] = 0;
    if (tid == 0) present = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (unsigned e = l0 + tid; e < l1; e += FRAME_RENDER_THREADS) {
      const unsigned g = list[e];
      SceneTri tr;
      if (!scene_load_tri(tb, vert_start, face_start, K, snap, g, tr)) continue;
      const unsigned long long obit = 1ull << tr.o;
      mine |= obit;
      frame_tri_walk(tr.a, tr.b, tr.c, X0, Y0, X1, Y1, [&](int px, int py, float z) {
        const int at = (py - Y0) * T + (px - X0);
        atomicMin(&zbuf[at], Key::pack(z, g));
        atomicOr(&cover[at], obit);
      });
    }
    if (mine) atomicOr(&present, mine);
    __syncthreads();
  }
  const bool walked = l0 != l1;   // uniform
  const unsigned long long here = walked ? present : 0;
  for (int i = tid; i < T * T; i += FRAME_RENDER_THREADS) {   // (a tile row per half-wave: 128-byte runs of the 4-byte outputs)
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const bool in = px < W && py < H;
    const size_t at = (size_t)py * W + px;
    const Key::type key = walked ? zbuf[i] : Key::EMPTY;
    const unsigned long long bits = walked && in ? cover[i] : 0;
    const bool model = in && key != Key::EMPTY;
    int o = -1, tri = -1;
    bool visible = model;
    if (model) {
      const unsigned g = Key::tri(key);
      o = scene_owner(face_start, K, g);
      tri = (int)(g - face_start[o]);
    }
    const float z = model ? Key::z(key) : 0.0f;
    if (model && (out.vis || out.overlay || out.counters)) visible = !frame_occluded(obs[at], z, tol);   // ... in front of the nearest model?
    if (in) {
      if (out.depth) out.depth[at] = z;
      if (out.inst) out.inst[at] = (uint8_t)(o + 1);
      if (out.vis) out.vis[at] = visible ? 255 : 0;
      if (out.tri) out.tri[at] = tri + 1;
      if (out.cover) out.cover[at] = bits;
      if (out.overlay) {
        int r = rgb[at * 3], gr = rgb[at * 3 + 1], bl = rgb[at * 3 + 2];
        if (visible) {
          // shade of the winning triangle, tint of its object
          const int32_t *f = tb->faces[o] + (size_t)tri * 3;
          const int base = vert_start[o];
          const int k = frame_shade(cam[base + f[0]], cam[base + f[1]], cam[base + f[2]]);
          const int p = o & 7;
          r = frame_tint(r, SCENE_PALETTE[p][0], k); gr = frame_tint(gr, SCENE_PALETTE[p][1], k); bl = frame_tint(bl, SCENE_PALETTE[p][2], k);
        }
        out.overlay[at * 3] = (uint8_t)r; out.overlay[at * 3 + 1] = (uint8_t)gr; out.overlay[at * 3 + 2] = (uint8_t)bl;
      }
    }
    if (out.counters) {
      // per-object counts of this wave's 64 pixels: one ballot per object of the tile and count, added to LDS by one lane
      for (unsigned long long rem = here; rem; rem &= rem - 1) {
        const int q = __ffsll((long long)rem) - 1;
        const unsigned long long cov = __ballot((int)((bits >> q) & 1));
        const unsigned long long fro = __ballot(o == q);
        const unsigned long long vis = __ballot(o == q && visible);
        if ((tid & 63) == 0) {
          if (cov) atomicAdd(&cnt[q * 3], __popcll(cov));
          if (fro) atomicAdd(&cnt[q * 3 + 1], __popcll(fro));
          if (vis) atomicAdd(&cnt[q * 3 + 2], __popcll(vis));
        }
      }
    }
  }
  if (walked && out.counters) {
    __syncthreads();
    if (tid < K * 3 && cnt[tid] != 0) atomicAdd(out.counters + tid, cnt[tid]);
  }
}

}  // namespace

void launch_scene_vertex(hipStream_t s, const SceneTable *table, int total_verts, int4 *snap, float4 *cam, int *flags) {
  FP_GEOM_LOG("scene_vertex");
  if (total_verts <= 0) return;
  hipLaunchKernelGGL(scene_vertex_kernel, dim3((unsigned)((total_verts + 255) / 256)), dim3(256), 0, s, table, total_verts, snap, cam, flags);
}

void launch_scene_bin_count(hipStream_t s, const SceneTable *table, unsigned total_faces, const int4 *snap, int H, int W, unsigned *count,
                            unsigned *offset, unsigned *cursor, unsigned long long *total) {
  FP_GEOM_LOG("scene_bin_count");
  const int ntx = scene_tiles_x(W), ntiles = ntx * scene_tiles_y(H);
  if (total_faces > 0)
    hipLaunchKernelGGL(scene_bin_kernel<false>, dim3((total_faces + 255u) / 256u), dim3(256), 0, s, table, total_faces, snap, H, W, ntx, ntiles, count,
                       (unsigned *)nullptr);
  FP_GEOM_LOG("scene_bin_scan");
  hipLaunchKernelGGL(scene_scan_kernel, dim3(1), dim3(256), 0, s, count, ntiles, offset, cursor, total);
}

void launch_scene_bin_fill(hipStream_t s, const SceneTable *table, unsigned total_faces, const int4 *snap, int H, int W, unsigned *cursor,
                           unsigned *list) {
  FP_GEOM_LOG("scene_bin_fill");
  if (total_faces == 0) return;
  hipLaunchKernelGGL(scene_bin_kernel<true>, dim3((total_faces + 255u) / 256u), dim3(256), 0, s, table, total_faces, snap, H, W,
                     scene_tiles_x(W), scene_tiles_x(W) * scene_tiles_y(H), cursor, list);
}

void launch_scene_raster(hipStream_t s, const SceneTable *table, const int4 *snap, const float4 *cam, const unsigned *offset,
                         const unsigned *list, const uint8_t *rgb, const float *depth, int H, int W, float tol_m, const SceneRenderOut &out) {
  FP_GEOM_LOG("scene_raster");
  const dim3 grid((unsigned)scene_tiles_x(W), (unsigned)scene_tiles_y(H));
  hipLaunchKernelGGL(scene_raster_kernel, grid, dim3(FRAME_RENDER_THREADS), 0, s, table, snap, cam, offset, list, rgb, depth, H, W, tol_m, out);
}

}  // namespace fp
