// Pose errors on the device (fp_pose_errors): ADD, MSSD and MSPD from one PAIRED kernel -- per (pose, symmetry)
// the same vertex under two transforms -- and ADD-S from a brute-force NEAREST-NEIGHBOUR kernel over Vs^2 point pairs per pose.  Every
// result is a maximum, a minimum or a sum of integers, so a record does not depend on thread order.  The file is compiled with
// -ffp-contract=off like the other geometry units: every f32 operation below is separately rounded, and the one place that wants a fused
// multiply-add (the squared distance of the inner loop) spells it fmaf.  tests/pose_error_ref.py holds both kernels to float64.
#include "fp_internal.h"

namespace fp {

namespace {

constexpr int PE_THREADS = POSE_ERROR_THREADS, PE_Q = POSE_ERROR_QUERIES, PE_TILE = POSE_ERROR_TILE;
constexpr int PE_WAVES = PE_THREADS / 64;
constexpr float PE_Q20 = 1048576.0f;

struct Mat34 {
  float r[9], t[3];
};
__device__ __forceinline__ Mat34 load_mat(const float *__restrict__ p) {
  Mat34 m;
  for (int k = 0; k < 9; k++) m.r[k] = p[k];
  for (int k = 0; k < 3; k++) m.t[k] = p[9 + k];
  return m;
}
__device__ __forceinline__ void transform(const Mat34 &m, float vx, float vy, float vz, float &x, float &y, float &z) {
  x = ((m.r[0] * vx + m.r[1] * vy) + m.r[2] * vz) + m.t[0];
  y = ((m.r[3] * vx + m.r[4] * vy) + m.r[5] * vz) + m.t[1];
  z = ((m.r[6] * vx + m.r[7] * vy) + m.r[8] * vz) + m.t[2];
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_down((int)v, off));
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// Paired kernel: one workgroup per (pose, symmetry) pair p; a = est[pose] v, b = comp[p] v in camera space.  Leaves max |a - b|, the
// largest projected distance, whether any z fails z >= FRAME_RENDER_NEAR, and sum llrintf(|a - b| * 2^20) (the host reads the sum of
// symmetry 0 only).  A maximum of non-negative floats is the unsigned maximum of their bit patterns.
__global__ __launch_bounds__(PE_THREADS) void pose_error_pair_kernel(const float *__restrict__ verts, int Vs, int step, float fx, float fy,
                                                                     float cx, float cy, const float *__restrict__ est,
                                                                     const float *__restrict__ comp, int S1, long long pair0,
                                                                     PoseErrPair *__restrict__ out) {
  __shared__ unsigned w_d[PE_WAVES], w_px[PE_WAVES];
  __shared__ int w_near[PE_WAVES];
  __shared__ long long w_sum[PE_WAVES];
  const int tid = threadIdx.x;
  const long long pair = pair0 + blockIdx.x;
  const long long pose = pair / S1;
  const Mat34 A = load_mat(est + pose * 12), B = load_mat(comp + pair * 12);
  unsigned max_d = 0, max_px = 0;
  int near = 0;
  long long sum = 0;
  for (int v = tid; v < Vs; v += PE_THREADS) {
    const float *p = verts + (size_t)v * step * 3;
    const float vx = p[0], vy = p[1], vz = p[2];
    float ax, ay, az, bx, by, bz;
    transform(A, vx, vy, vz, ax, ay, az);
    transform(B, vx, vy, vz, bx, by, bz);
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    max_d = max(max_d, __float_as_uint(d));
    sum += llrintf(d * PE_Q20);
    if (!(az >= FRAME_RENDER_NEAR) || !(bz >= FRAME_RENDER_NEAR)) near = 1;   // (also a NaN)
    else {
      const float du = (fx * (ax / az) + cx) - (fx * (bx / bz) + cx);
      const float dw = (fy * (ay / az) + cy) - (fy * (by / bz) + cy);
      max_px = max(max_px, __float_as_uint(sqrtf(du * du + dw * dw)));
    }
  }
  max_d = wave_max_u32(max_d);
  max_px = wave_max_u32(max_px);
  near = __any(near) ? 1 : 0;
  sum = wave_sum_i64(sum);
  if ((tid & 63) == 0) { w_d[tid >> 6] = max_d; w_px[tid >> 6] = max_px; w_near[tid >> 6] = near; w_sum[tid >> 6] = sum; }
  __syncthreads();
  if (tid == 0) {
    PoseErrPair r = {0, 0, 0, 0, 0};
    for (int w = 0; w < PE_WAVES; w++) {
      r.max_d_bits = max(r.max_d_bits, w_d[w]);
      r.max_px_bits = max(r.max_px_bits, w_px[w]);
      r.near |= w_near[w];
      r.sum_q20 += w_sum[w];
    }
    out[pair] = r;
  }
}

// Nearest-neighbour kernel in the relative frame: with D = E^-1 G (formed on the host in double), |G u - E v| = |D u - v|, so the
// targets are the static centred vertices, the same for every pose.  The launch's items are (pose, query) pairs, pose-major; a lane
// owns PE_Q of them in registers (item g = block * PE_THREADS * PE_Q + k * PE_THREADS + lane, so a wave reads neighbouring vertices).
// The targets pass through LDS in tiles of PE_TILE points, structure of arrays: in the inner loop every lane reads the SAME address,
// which the LDS broadcasts without a bank conflict.  A ragged last tile is padded with copies of the last vertex up to a multiple of
// the unroll factor (a duplicate never changes a minimum); items beyond the launch's last contribute 0.  The inner loop is subtract,
// square, add and min on the squared distance; one sqrtf per item at the end, then llrintf(d * 2^20) into the pose's 64-bit sum: by a
// wave reduction and one atomic when the wave's 64 items belong to one pose, else per lane.
__global__ __launch_bounds__(PE_THREADS) void pose_error_nn_kernel(const float *__restrict__ verts, int Vs, int step,
                                                                   const float *__restrict__ rel, int pose0, long long n_items,
                                                                   unsigned long long *__restrict__ sums) {
  constexpr int UNROLL = 8;
  static_assert(PE_TILE % UNROLL == 0, "the padded tile stays inside the LDS arrays");
  __shared__ float tx[PE_TILE], ty[PE_TILE], tz[PE_TILE];
  const int tid = threadIdx.x;
  float qx[PE_Q], qy[PE_Q], qz[PE_Q], best[PE_Q];
  int pose[PE_Q];
  bool live[PE_Q];
#pragma unroll
  for (int k = 0; k < PE_Q; k++) {
    const long long g = (long long)blockIdx.x * (PE_THREADS * PE_Q) + k * PE_THREADS + tid;
    live[k] = g < n_items;
    const long long gc = live[k] ? g : n_items - 1;
    pose[k] = (int)(gc / Vs);
    const int u = (int)(gc - (long long)pose[k] * Vs);
    const float *p = verts + (size_t)u * step * 3;
    const Mat34 D = load_mat(rel + (size_t)(pose0 + pose[k]) * 12);
    transform(D, p[0], p[1], p[2], qx[k], qy[k], qz[k]);
    best[k] = INFINITY;
  }
  for (int t0 = 0; t0 < Vs; t0 += PE_TILE) {   // uniform
    const int n = min(PE_TILE, Vs - t0), n_pad = (n + UNROLL - 1) / UNROLL * UNROLL;
    __syncthreads();   // (the previous tile has been read)
    for (int i = tid; i < n_pad; i += PE_THREADS) {
      const float *p = verts + (size_t)min(t0 + i, Vs - 1) * step * 3;
      tx[i] = p[0]; ty[i] = p[1]; tz[i] = p[2];
    }
    __syncthreads();
    for (int j = 0; j < n_pad; j += UNROLL) {
#pragma unroll
      for (int jj = 0; jj < UNROLL; jj++) {
        const float x = tx[j + jj], y = ty[j + jj], z = tz[j + jj];
#pragma unroll
        for (int k = 0; k < PE_Q; k++) {
          const float dx = qx[k] - x, dy = qy[k] - y, dz = qz[k] - z;
          best[k] = fminf(best[k], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PE_Q; k++) {
    const long long q = live[k] ? llrintf(sqrtf(best[k]) * PE_Q20) : 0;
    const int first = __shfl(pose[k], 0);
    if (__all(pose[k] == first)) {   // wave-uniform
      const long long s = wave_sum_i64(q);
      if ((tid & 63) == 0 && s != 0) atomicAdd(sums + pose0 + first, (unsigned long long)s);
    } else if (q != 0) {
      atomicAdd(sums + pose0 + pose[k], (unsigned long long)q);
    }
  }
}

}  // namespace

void launch_pose_error_pairs(hipStream_t s, const float *verts, int Vs, int step, float fx, float fy, float cx, float cy, const float *est,
                             const float *comp, int S1, long long pair0, int n_pairs, PoseErrPair *out) {
  FP_GEOM_LOG("pose_error_pairs");
  if (n_pairs <= 0 || Vs <= 0) return;
  hipLaunchKernelGGL(pose_error_pair_kernel, dim3((unsigned)n_pairs), dim3(PE_THREADS), 0, s, verts, Vs, step, fx, fy, cx, cy, est, comp, S1,
                     pair0, out);
}

void launch_pose_error_nn(hipStream_t s, const float *verts, int Vs, int step, const float *rel, int pose0, int n_poses,
                          unsigned long long *sums) {
  FP_GEOM_LOG("pose_error_nn");
  if (n_poses <= 0 || Vs <= 0) return;
  const long long n_items = (long long)n_poses * Vs, per_block = PE_THREADS * PE_Q;
  hipLaunchKernelGGL(pose_error_nn_kernel, dim3((unsigned)((n_items + per_block - 1) / per_block)), dim3(PE_THREADS), 0, s, verts, Vs, step, rel,
                     pose0, n_items, sums);
}

}  // namespace fp
