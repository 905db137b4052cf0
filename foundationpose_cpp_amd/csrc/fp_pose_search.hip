// Depth search of N poses (fp_pose_search): the device half.  One kernel, one workgroup per pose: every sampled
// vertex of the centred mesh is rotated once with its normal, then pushed back along the ray of the pose's origin step by step; at every
// step the point is projected into the RAW depth of the frame and put into one of five classes.  The counts of a (pose, step) are wave
// ballots added to an LDS table, the best step is picked in the workgroup, and one thread stores the pose's record: no global atomics,
// integers only, so a record does not depend on the batch around it.  Compiled with -ffp-contract=off like the rest of the geometry:
// every f32 operation is separately rounded, tests/search_ref.py restates them.
#include "fp_internal.h"

namespace fp {

namespace {

__global__ __launch_bounds__(SEARCH_THREADS) void pose_search_kernel(const float *__restrict__ verts, const float *__restrict__ normals,
                                                                     const FramePose *__restrict__ poses, const float *__restrict__ depth,
                                                                     SearchParams S, SearchRec *__restrict__ out) {
  __shared__ int table[SEARCH_MAX_STEPS][SEARCH_CLASSES];
  __shared__ int refused[SEARCH_MAX_STEPS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < SEARCH_MAX_STEPS * SEARCH_CLASSES; i += SEARCH_THREADS) (&table[0][0])[i] = 0;
  if (tid < SEARCH_MAX_STEPS) refused[tid] = 0;
  __syncthreads();
  const FramePose P = poses[blockIdx.x];
  const float ray_x = P.t[0] / P.t[2], ray_y = P.t[1] / P.t[2];   // the ray of the pose's own origin
  const float w_max = (float)(S.W - 1), h_max = (float)(S.H - 1);
  // every thread of a wave makes every round (a thread without a point has live == false), so the ballots below are whole
  for (int base = 0; base < S.P; base += SEARCH_THREADS) {
    const int pt = base + tid;
    const bool live = pt < S.P;
    const size_t v = live ? (size_t)pt * (size_t)S.vertex_step : 0;   // (P = ceil(V / vertex_step): the last point is a vertex)
    const float x = verts[v * 3], y = verts[v * 3 + 1], z = verts[v * 3 + 2];
    const float nx = normals[v * 3], ny = normals[v * 3 + 1], nz = normals[v * 3 + 2];
    const float rx = (P.r[0] * x + P.r[1] * y) + P.r[2] * z;
    const float ry = (P.r[3] * x + P.r[4] * y) + P.r[5] * z;
    const float rz = (P.r[6] * x + P.r[7] * y) + P.r[8] * z;
    const float mx = (P.r[0] * nx + P.r[1] * ny) + P.r[2] * nz;
    const float my = (P.r[3] * nx + P.r[4] * ny) + P.r[5] * nz;
    const float mz = (P.r[6] * nx + P.r[7] * ny) + P.r[8] * nz;
    for (int k = 0; k < S.n_steps; k++) {
      const float s = (float)k * S.step_m;
      const float qx = rx + (P.t[0] + s * ray_x), qy = ry + (P.t[1] + s * ray_y), qz = rz + (P.t[2] + s);
      const bool near = live && qz < FRAME_RENDER_NEAR;
      const float a = -((mx * qx + my * qy) + mz * qz);
      const bool facing = live && a > 0.0f && a * a > SEARCH_MIN_COS2 * ((qx * qx + qy * qy) + qz * qz);
      const float uf = rintf(P.fx * (qx / qz) + P.cx), vf = rintf(P.fy * (qy / qz) + P.cy);
      // compared as floats: a NaN or a huge value is outside, and what is inside converts exactly
      const bool inside = uf >= 0.0f && uf <= w_max && vf >= 0.0f && vf <= h_max;
      float D = 0.0f;
      if (facing && inside) D = depth[(size_t)(int)vf * (size_t)S.W + (size_t)(int)uf];
      const bool seen = D >= FP_MIN_DEPTH && D <= 3.402823466e+38f;   // not missing, NaN or infinite
      const float dz = D - qz;
      const bool hit = facing && inside && seen;
      const int n_facing = (int)wave_count(facing);
      const int n_inlier = (int)wave_count(hit && fabsf(dz) <= S.tol_m);
      const int n_front = (int)wave_count(hit && dz < -S.tol_m);
      const int n_behind = (int)wave_count(hit && dz > S.tol_m);
      const int n_outside = (int)wave_count(facing && !inside);
      const int n_missing = (int)wave_count(facing && inside && !seen);
      const bool any_near = __ballot(near) != 0ull;
      if (lane == 0) {   // integer LDS adds: the order does not matter
        if (n_facing) atomicAdd(&table[k][0], n_facing);
        if (n_inlier) atomicAdd(&table[k][1], n_inlier);
        if (n_front) atomicAdd(&table[k][2], n_front);
        if (n_behind) atomicAdd(&table[k][3], n_behind);
        if (n_outside) atomicAdd(&table[k][4], n_outside);
        if (n_missing) atomicAdd(&table[k][5], n_missing);
        if (any_near) atomicOr(&refused[k], 1);
      }
    }
  }
  __syncthreads();
  // the best step: the largest score, the lowest step on ties; a refused step competes with no score.  key = score + 2^31 above the
  // reversed step, -1 for a step that does not compete.
  long long key = -1;
  if (tid < S.n_steps && !refused[tid]) {
    const long long score = (long long)table[tid][1] - (long long)table[tid][3] - (long long)table[tid][4];
    key = ((score + 2147483648ll) << 8) | (long long)(SEARCH_MAX_STEPS - 1 - tid);
  }
  if (tid < 64) {   // (SEARCH_MAX_STEPS == 64: the first wave holds every step)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const long long other = __shfl_xor(key, d, 64);
      key = other > key ? other : key;
    }
  }
  if (tid == 0) {
    const long long kbest = key;
    SearchRec r;
    for (int j = 0; j < SEARCH_CLASSES; j++) r.n[j] = 0;
    r.score = 0; r.best_step = -1; r.n_points = S.P; r.status = SEARCH_STATUS_REFUSED_NEAR;
    if (kbest >= 0) {
      const int k = SEARCH_MAX_STEPS - 1 - (int)(kbest & 255);
      for (int j = 0; j < SEARCH_CLASSES; j++) r.n[j] = table[k][j];
      r.score = table[k][1] - table[k][3] - table[k][4];
      r.best_step = k; r.status = 0;
    }
    out[blockIdx.x] = r;
  }
}

}  // namespace

void launch_pose_search(hipStream_t s, const DeviceMesh &m, const FramePose *poses, int n, const float *depth, const SearchParams &S, SearchRec *out) {
  FP_GEOM_LOG("pose_search");
  if (n <= 0 || S.P <= 0) return;
  hipLaunchKernelGGL(pose_search_kernel, dim3((unsigned)n), dim3(SEARCH_THREADS), 0, s, m.verts, m.normals, poses, depth, S, out);
}

}  // namespace fp
