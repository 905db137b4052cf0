// Silhouette agreement of N poses with a mask of the uploaded frame (fp_pose_silhouette / fp_mask_distance): the
// device half.  Three kernels of its own: the two passes of an exact Euclidean distance transform of the mask (squared distances to the
// nearest mask pixel and to the nearest other pixel, both at once), and a tile kernel over (pose, tile) items that rasterises the pose
// into a 32-bit LDS z-buffer exactly as frame_raster_kernel does and counts, over the pose's pixels, how the (visible) model and the mask
// overlap, with the squared distances of the pixels where they do not.  The vertex pass is launch_pose_vertices' (fp_frame_render.hip).
// Every rule that decides the depth of a pixel is fp_frame_rules.h's; everything new is integer, tests/silhouette_ref.py restates it.
#include "fp_frame_rules.h"

namespace fp {

namespace {

constexpr unsigned EDT_NONE_COL = 0xFFFFu;        // column distance: no seed in this column (H <= 8192, so a distance is < 8192)
constexpr unsigned EDT_NONE = 0x7fffffffu;        // FP_SIL_D2_NONE
constexpr int EDT_COL_THREADS = 64, EDT_ROW_THREADS = 256;
constexpr int SIL_PX_PER_THREAD = FRAME_RENDER_TILE * FRAME_RENDER_TILE / FRAME_RENDER_THREADS;
constexpr int SIL_WAVES = FRAME_RENDER_THREADS / 64;

// (a) columns pass: one thread per column, adjacent threads adjacent columns, so every row's reads and writes are coalesced.  Going down,
// then up, the distance along the column to the nearest seed of each set: set 0 = the mask pixels (byte > 0), set 1 = the others.
// g [2, H, W]; any [2] |= 1 where a set has a seed at all.
__global__ __launch_bounds__(EDT_COL_THREADS) void mask_edt_cols(const uint8_t *__restrict__ mask, int H, int W, uint16_t *__restrict__ g,
                                                                 int *__restrict__ any) {
  const int c = blockIdx.x * EDT_COL_THREADS + threadIdx.x;
  if (c >= W) return;
  const size_t plane = (size_t)H * W;
  unsigned dm = EDT_NONE_COL, db = EDT_NONE_COL;
  for (int r = 0; r < H; r++) {
    const size_t at = (size_t)r * W + c;
    const bool on = mask[at] > 0;
    dm = on ? 0u : (dm == EDT_NONE_COL ? dm : dm + 1u);
    db = on ? (db == EDT_NONE_COL ? db : db + 1u) : 0u;
    g[at] = (uint16_t)dm;
    g[plane + at] = (uint16_t)db;
  }
  // (the last row's values tell whether the column has a seed of either set)
  if (dm != EDT_NONE_COL) atomicOr(any, 1);
  if (db != EDT_NONE_COL) atomicOr(any + 1, 1);
  dm = EDT_NONE_COL; db = EDT_NONE_COL;
  for (int r = H - 1; r >= 0; r--) {
    const size_t at = (size_t)r * W + c;
    const bool on = mask[at] > 0;
    dm = on ? 0u : (dm == EDT_NONE_COL ? dm : dm + 1u);
    db = on ? (db == EDT_NONE_COL ? db : db + 1u) : 0u;
    if (dm < g[at]) g[at] = (uint16_t)dm;
    if (db < g[plane + at]) g[plane + at] = (uint16_t)db;
  }
}

// min over c' of (c - c')^2 + g(c')^2 for the row `g` [W] staged in LDS: outwards from c, k = 0, 1, 2, ..., until k^2 >= best -- every later
// term is >= k^2, so the minimum is exact.  At most 8191^2 + 8191^2 < 2^31.
__device__ __forceinline__ unsigned edt_row_min(const uint16_t *g, int c, int W) {
  unsigned best = EDT_NONE;
  const unsigned g0 = g[c];
  if (g0 != EDT_NONE_COL) best = g0 * g0;
  for (int k = 1; (unsigned)(k * k) < best; k++) {
    const int lo = c - k, hi = c + k;
    if (lo < 0 && hi >= W) break;
    if (lo >= 0) {
      const unsigned v = g[lo];
      if (v != EDT_NONE_COL) best = min(best, v * v + (unsigned)(k * k));
    }
    if (hi < W) {
      const unsigned v = g[hi];
      if (v != EDT_NONE_COL) best = min(best, v * v + (unsigned)(k * k));
    }
  }
  return best;
}

// (b) rows pass: workgroup (x, r) stages row r's column distances of both sets in LDS (2 W 16-bit words: squaring on the way out of LDS
// costs one multiply and halves the footprint of staged squares) and gives EDT_ROW_THREADS pixels of the row their two squared distances.
// A set without a seed anywhere (any[set] == 0) is not searched.  tot[0] += the mask pixels, tot[1] += clip(d2 to the other set) over
// them (t2 > 0: the clip), by wave sums and one 64-bit atomic per workgroup and word.
__global__ __launch_bounds__(EDT_ROW_THREADS) void mask_edt_rows(const uint16_t *__restrict__ g, const int *__restrict__ any, int H, int W,
                                                                 uint32_t *__restrict__ d2, unsigned t2, unsigned long long *__restrict__ tot) {
  extern __shared__ uint16_t row[];   // [2, W]
  __shared__ unsigned long long part[EDT_ROW_THREADS / 64][2];
  const int r = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)H * W;
  const bool any_m = any[0] != 0, any_b = any[1] != 0;   // (uniform)
  for (int i = tid; i < W; i += EDT_ROW_THREADS) {
    row[i] = g[(size_t)r * W + i];
    row[W + i] = g[plane + (size_t)r * W + i];
  }
  __syncthreads();
  const int c = blockIdx.x * EDT_ROW_THREADS + tid;
  unsigned long long n = 0, sum = 0;
  if (c < W) {
    const unsigned dm = any_m ? edt_row_min(row, c, W) : EDT_NONE;
    const unsigned db = any_b ? edt_row_min(row + W, c, W) : EDT_NONE;
    d2[(size_t)r * W + c] = dm;
    d2[plane + (size_t)r * W + c] = db;
    if (dm == 0) {   // a mask pixel
      n = 1;
      sum = t2 ? min(db, t2) : db;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n += __shfl_xor(n, d, 64);
    sum += __shfl_xor(sum, d, 64);
  }
  if ((tid & 63) == 0) { part[tid >> 6][0] = n; part[tid >> 6][1] = sum; }
  __syncthreads();
  if (tid < 2) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < EDT_ROW_THREADS / 64; w++) v += part[w][tid];
    if (v) atomicAdd(tot + tid, v);
  }
}

// (c) tile kernel: one workgroup per item {pose of the launch's chunk, tile}.  flags / acc are indexed by pose0 + pose; a pose's
// accumulator is SIL_WORDS 64-bit words: n_model, n_visible, n_inter, n_spill, the sum of clip(d2 to the mask) over the spill pixels, the
// sum of clip(d2 to the background) over the inter pixels.
template <bool AMODAL>
__global__ __launch_bounds__(FRAME_RENDER_THREADS) void silhouette_tile(const int32_t *__restrict__ faces, int F, int V, const int4 *__restrict__ snap,
                                                                        const int2 *__restrict__ items, const float *__restrict__ obs,
                                                                        const uint8_t *__restrict__ mask, const uint32_t *__restrict__ d2, int H, int W,
                                                                        int ntx, float tol, unsigned t2, const int *__restrict__ flags, int pose0,
                                                                        unsigned long long *__restrict__ acc) {
  typedef FrameKeyZ Key;   // the depth decides; the triangle is not needed
  constexpr int T = FRAME_RENDER_TILE;
  __shared__ Key::type zbuf[T * T];
  __shared__ unsigned long long part[SIL_WAVES][SIL_WORDS];
  const int tid = threadIdx.x;
  const int2 item = items[blockIdx.x];
  const int pose = item.x, tile = item.y;
  if (flags[pose0 + pose]) return;   // (uniform) a refused pose: the host gives its record the status bit
  const FrameTile rect = frame_tile_rect_of(tile, ntx, H, W);
  const int X0 = rect.X0, Y0 = rect.Y0;
  frame_zbuf_clear<Key>(zbuf, tid);
  __syncthreads();
  frame_face_walk<Key>(faces, F, V, snap + (size_t)pose * V, rect, zbuf, tid);
  __syncthreads();
  const size_t plane = (size_t)H * W;
  // a clipped squared distance can reach 2^30 (trunc_px 32767) and FP_SIL_D2_NONE is 2^31 - 1: four pixels of one thread, let alone the
  // 1 024 of a tile, do not fit 32 bits, so both sums are 64-bit from the first addition on
  unsigned long long sum_spill = 0, sum_inter = 0;
  unsigned n_model = 0, n_visible = 0, n_inter = 0, n_spill = 0;   // wave-uniform
#pragma unroll
  for (int k = 0; k < SIL_PX_PER_THREAD; k++) {
    const int i = k * FRAME_RENDER_THREADS + tid;
    const int px = X0 + (i & (T - 1)), py = Y0 + i / T;
    const Key::type key = zbuf[i];
    const bool model = px < W && py < H && key != Key::EMPTY;
    bool visible = false, inter = false;
    if (model) {
      const size_t at = (size_t)py * W + px;
      visible = AMODAL ? true : !frame_occluded(obs[at], Key::z(key), tol);
      if (visible) {
        inter = mask[at] > 0;
        const unsigned v = d2[inter ? plane + at : at];
        const unsigned long long cv = t2 ? min(v, t2) : v;
        if (inter) sum_inter += cv;
        else sum_spill += cv;
      }
    }
    n_model += wave_count(model); n_visible += wave_count(visible);
    n_inter += wave_count(inter); n_spill += wave_count(visible && !inter);
  }
  // per wave, then across the four waves through LDS, then one integer atomic per non-zero word: integer sums do not depend on the order
  const int wave = tid >> 6, lane = tid & 63;
  if (n_visible) {   // (uniform)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      sum_spill += __shfl_xor(sum_spill, d, 64);
      sum_inter += __shfl_xor(sum_inter, d, 64);
    }
  }
  if (lane == 0) {
    part[wave][0] = n_model; part[wave][1] = n_visible; part[wave][2] = n_inter; part[wave][3] = n_spill;   // (ballots: the wave's own lanes)
    part[wave][4] = sum_spill; part[wave][5] = sum_inter;
  }
  __syncthreads();
  if (tid < SIL_WORDS) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < SIL_WAVES; w++) v += part[w][tid];
    if (v) atomicAdd(acc + (size_t)(pose0 + pose) * SIL_WORDS + tid, v);
  }
}

}  // namespace

void launch_mask_edt_cols(hipStream_t s, const uint8_t *mask, int H, int W, uint16_t *g, int *any) {
  FP_GEOM_LOG("mask_edt_cols");
  hipLaunchKernelGGL(mask_edt_cols, dim3((unsigned)((W + EDT_COL_THREADS - 1) / EDT_COL_THREADS)), dim3(EDT_COL_THREADS), 0, s, mask, H, W, g, any);
}

void launch_mask_edt_rows(hipStream_t s, const uint16_t *g, const int *any, int H, int W, uint32_t *d2, long long t2, unsigned long long *tot) {
  FP_GEOM_LOG("mask_edt_rows");
  hipLaunchKernelGGL(mask_edt_rows, dim3((unsigned)((W + EDT_ROW_THREADS - 1) / EDT_ROW_THREADS), (unsigned)H), dim3(EDT_ROW_THREADS),
                     (size_t)2 * W * sizeof(uint16_t), s, g, any, H, W, d2, (unsigned)t2, tot);
}

void launch_silhouette_tiles(hipStream_t s, const DeviceMesh &m, const int4 *snap, const int2 *items, int n_items, const float *depth,
                             const uint8_t *mask, const uint32_t *d2, int H, int W, float tol_m, long long t2, bool amodal, const int *flags, int pose0,
                             unsigned long long *acc) {
  FP_GEOM_LOG("silhouette_tile");
  if (n_items <= 0) return;
  const int ntx = scene_tiles_x(W);
  if (amodal)
    hipLaunchKernelGGL(silhouette_tile<true>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, items, depth, mask, d2, H, W,
                       ntx, tol_m, (unsigned)t2, flags, pose0, acc);
  else
    hipLaunchKernelGGL(silhouette_tile<false>, dim3((unsigned)n_items), dim3(FRAME_RENDER_THREADS), 0, s, m.faces, m.F, m.V, snap, items, depth, mask, d2, H, W,
                       ntx, tol_m, (unsigned)t2, flags, pose0, acc);
}

}  // namespace fp
