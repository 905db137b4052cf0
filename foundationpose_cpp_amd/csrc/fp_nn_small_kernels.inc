// fp_nn_small_kernels.inc -- bandwidth-trivial helper kernels (device code)
// Part of the fp_nn.hip translation unit (included there, inside namespace fp unless stated): kernel templates must be visible
// where they are launched, so this is a textual split, not a separate compilation unit.

// =================================================================================================
// small kernels
// =================================================================================================

// x[b,t,:] += pe[t,:]  (rows = B*T, 512 channels, 8 halfs per thread)
template <int DT>
__global__ void add_pos_embed_kernel(typename ElemT<DT>::t *__restrict__ x, const typename ElemT<DT>::t *__restrict__ pe, int T, size_t rows) {
  using E8 = typename ElemT<DT>::v8;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // 16-B chunk index
  if (i >= rows * (EMBED / 8)) return;
  size_t row = i / (EMBED / 8);
  int c = (int)(i - row * (EMBED / 8));
  int t = (int)(row % T);
  E8 a = reinterpret_cast<const E8 *>(x)[i];
  E8 pv = reinterpret_cast<const E8 *>(pe)[(size_t)t * (EMBED / 8) + c];
  E8 r;
#pragma unroll
  for (int e = 0; e < 8; e++) r[e] = (typename ElemT<DT>::t)((float)a[e] + (float)pv[e]);
  reinterpret_cast<E8 *>(x)[i] = r;
}

// out[b,c] = mean_t x[b,t,c]  (f32 out).  Deterministic (no atomics: the arg-max over near-tied scores must not depend
// on summation order).  block = (b, 64-channel group); a lane loads 8 channels (16 B) of one token, so a wave covers 8
// tokens per load and walks the sequence in strides of 32 tokens (13 dependent steps for T = 400 instead of 100: at
// N = 1 this kernel was 30 us of a 570 us Track); the 8 token slots combine through shfl_xor, the 4 waves through LDS,
// both in a fixed order.
template <int DT>
__global__ __launch_bounds__(256) void token_mean_kernel(const typename ElemT<DT>::t *__restrict__ x, float *__restrict__ out, int T, int tstride) {
  using E8 = typename ElemT<DT>::v8;
  __shared__ float part[4][64];
  const int b = blockIdx.x, cg = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane >> 3, c8 = (lane & 7) * 8;
  const typename ElemT<DT>::t *src = x + (size_t)b * tstride * EMBED + cg * 64 + c8;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; e++) s[e] = 0.f;
  for (int t = wave * 8 + slot; t < T; t += 32) {
    E8 v = *reinterpret_cast<const E8 *>(src + (size_t)t * EMBED);
#pragma unroll
    for (int e = 0; e < 8; e++) s[e] += (float)v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    s[e] += __shfl_xor(s[e], 8);
    s[e] += __shfl_xor(s[e], 16);
    s[e] += __shfl_xor(s[e], 32);
  }
  if (slot == 0) {
#pragma unroll
    for (int e = 0; e < 8; e++) part[wave][c8 + e] = s[e];
  }
  __syncthreads();
  if (wave == 0) out[(size_t)b * EMBED + cg * 64 + lane] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (float)T;
}

// y[b,o] = bias[o] + sum_c x[b,c] W[o,c]   (f32).  One wave per (output o, block of 8 rows b): the weight row lives in registers
// (C = 512: 8 floats per lane) and is reused for the 8 rows, so W is read B/8 times instead of B times (the 512x512 out_proj of
// the score-net at N = 252: 130 MB -> 16 MB of L2 reads); the summation order of a (b, o) pair is the same as one wave per output.
__global__ __launch_bounds__(256) void small_linear_kernel(const float *__restrict__ x, const float *__restrict__ W,
                                                           const float *__restrict__ bias, float *__restrict__ y, int B,
                                                           int O, int C) {
  const int nbb = (B + 7) / 8;
  size_t widx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (widx >= (size_t)nbb * O) return;
  const int bb = (int)(widx / O), o = (int)(widx - (size_t)bb * O);
  const int b0 = bb * 8, nb = min(8, B - b0);
  if (C == 512) {
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = W[(size_t)o * C + lane + 64 * j];
    for (int i = 0; i < nb; i++) {
      const float *xr = x + (size_t)(b0 + i) * C;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; j++) s += xr[lane + 64 * j] * w[j];
#pragma unroll
      for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
      if (lane == 0) y[(size_t)(b0 + i) * O + o] = s + bias[o];
    }
    return;
  }
  for (int i = 0; i < nb; i++) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += x[(size_t)(b0 + i) * C + c] * W[(size_t)o * C + c];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
    if (lane == 0) y[(size_t)(b0 + i) * O + o] = s + bias[o];
  }
}

#ifdef FP_TEST_HOOKS
// -------------------------------------------------------------------------------------------------
// Kernels of the launch-chain forms of the refiner heads (plan_heads: TAIL_GROUPED_CHAIN / TAIL_HEAD_CHAIN).  The chains are the
// float64-tapped reference of the test build (tests/test_layers_gpu.py); the product runs enc_tail_kernel + enc_heads_kernel and
// does not carry them.
// -------------------------------------------------------------------------------------------------

// y = LayerNorm(x) over 512 channels, eps 1e-5; one wave per row
// rows >= split_row use (gamma1, beta1): the refiner's two heads normalised in one launch
template <int DT>
__global__ __launch_bounds__(256) void layernorm_kernel(const typename ElemT<DT>::t *__restrict__ x, const float *__restrict__ gamma0,
                                                        const float *__restrict__ beta0, typename ElemT<DT>::t *__restrict__ y, size_t rows,
                                                        const float *__restrict__ gamma1, const float *__restrict__ beta1,
                                                        size_t split_row) {
  size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *gamma = row >= split_row ? gamma1 : gamma0, *beta = row >= split_row ? beta1 : beta0;
  using E8 = typename ElemT<DT>::v8;
  E8 v = reinterpret_cast<const E8 *>(x + row * EMBED)[lane];
  float f[8], s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; e++) { f[e] = (float)v[e]; s += f[e]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  float mean = s * (1.0f / EMBED), q = 0.f;
#pragma unroll
  for (int e = 0; e < 8; e++) { f[e] -= mean; q += f[e] * f[e]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  float rstd = rsqrtf(q * (1.0f / EMBED) + 1e-5f);
  E8 r;
#pragma unroll
  for (int e = 0; e < 8; e++) r[e] = (typename ElemT<DT>::t)(f[e] * rstd * gamma[lane * 8 + e] + beta[lane * 8 + e]);
  reinterpret_cast<E8 *>(y + row * EMBED)[lane] = r;
}

// Track [r5]: LayerNorm + PARTIAL token sums for a handful of sequences -- layernorm_kernel + token_mean_kernel were two dependent
// launches of ~5 us each in a graph whose length is its number of launches, and the one-workgroup-per-sequence kernel below is a serial
// chain of 25 rows per wave (20 us for two sequences).  Here blockIdx.y cuts a sequence into `parts` runs of rows; a workgroup's four
// waves take the rows of its run (a wave per row: the arithmetic of layernorm_kernel incl. the rounding to the element type),
// per-lane column sums, fixed-order reduction over the waves -> out[b][part][512] COLUMN SUMS; the consumer (small_linear2_pose_kernel /
// small_linear2_kernel, SmallLinear2::parts) adds the parts in order and divides by the token count.  No atomics: bit-reproducible.
template <int DT>
__global__ __launch_bounds__(256) void layernorm_pmean_kernel(const typename ElemT<DT>::t *__restrict__ x, const float *__restrict__ gamma0,
                                                              const float *__restrict__ beta0, const float *__restrict__ gamma1,
                                                              const float *__restrict__ beta1, int split_b, float *__restrict__ out, int T,
                                                              int tstride, int rows_per_part) {
  using E = typename ElemT<DT>::t;
  using E8 = typename ElemT<DT>::v8;
  __shared__ float part[4][EMBED];
  const int b = blockIdx.x, pt = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *gamma = b >= split_b ? gamma1 : gamma0, *beta = b >= split_b ? beta1 : beta0;
  float gm[8], bt[8], acc[8];
#pragma unroll
  for (int e = 0; e < 8; e++) { gm[e] = gamma[lane * 8 + e]; bt[e] = beta[lane * 8 + e]; acc[e] = 0.f; }
  const E *src = x + (size_t)b * tstride * EMBED;
  const int r0 = pt * rows_per_part, r1 = min(T, r0 + rows_per_part);
  auto fold = [&](const E8 &v) {
    float f[8], s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { f[e] = (float)v[e]; s += f[e]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    float mean = s * (1.0f / EMBED), q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { f[e] -= mean; q += f[e] * f[e]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    float rstd = rsqrtf(q * (1.0f / EMBED) + 1e-5f);
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] += (float)(E)(f[e] * rstd * gm[e] + bt[e]);
  };
  for (int t = r0 + wave; t < r1; t += 16) {   // four rows of a wave in flight
    E8 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (t + 4 * j < r1) v[j] = reinterpret_cast<const E8 *>(src + (size_t)(t + 4 * j) * EMBED)[lane];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (t + 4 * j < r1) fold(v[j]);
  }
#pragma unroll
  for (int e = 0; e < 8; e++) part[wave][lane * 8 + e] = acc[e];
  __syncthreads();
  for (int c = threadIdx.x; c < EMBED; c += 256)
    out[((size_t)b * gridDim.y + pt) * EMBED + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// out[b,:] = mean_t LayerNorm(x[b,t,:]): the encoder's second LayerNorm feeds nothing but the token mean, so the normalised
// tensor never goes to memory (two 103 MB passes per head at N = 252).  One workgroup per sequence, 16 waves, a wave per row
// (the arithmetic of layernorm_kernel incl. the rounding to the element type), per-lane column sums, fixed-order reduction.
// Sequences b >= split_b use (gamma1, beta1): the refiner's two heads in one launch (Track).
template <int DT>
__global__ __launch_bounds__(1024) void layernorm_mean_kernel(const typename ElemT<DT>::t *__restrict__ x, const float *__restrict__ gamma0,
                                                              const float *__restrict__ beta0, const float *__restrict__ gamma1,
                                                              const float *__restrict__ beta1, int split_b, float *__restrict__ out, int T,
                                                              int tstride) {
  using E = typename ElemT<DT>::t;
  using E8 = typename ElemT<DT>::v8;
  __shared__ float part[16][EMBED];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *gamma = b >= split_b ? gamma1 : gamma0, *beta = b >= split_b ? beta1 : beta0;
  float gm[8], bt[8], acc[8];
#pragma unroll
  for (int e = 0; e < 8; e++) { gm[e] = gamma[lane * 8 + e]; bt[e] = beta[lane * 8 + e]; acc[e] = 0.f; }
  const E *src = x + (size_t)b * tstride * EMBED;
  auto fold = [&](const E8 &v) {
    float f[8], s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { f[e] = (float)v[e]; s += f[e]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    float mean = s * (1.0f / EMBED), q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { f[e] -= mean; q += f[e] * f[e]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    float rstd = rsqrtf(q * (1.0f / EMBED) + 1e-5f);
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] += (float)(E)(f[e] * rstd * gm[e] + bt[e]);
  };
  // four rows of a wave in flight (rows wave, wave+16, ...: ascending order inside a wave, so the sums do not depend on the unroll)
  for (int t = wave; t < T; t += 64) {
    E8 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (t + 16 * j < T) v[j] = reinterpret_cast<const E8 *>(src + (size_t)(t + 16 * j) * EMBED)[lane];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (t + 16 * j < T) fold(v[j]);
  }
#pragma unroll
  for (int e = 0; e < 8; e++) part[wave][lane * 8 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < EMBED) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 16; w++) s += part[w][threadIdx.x];
    out[(size_t)b * EMBED + threadIdx.x] = s / (float)T;
  }
}

// the same for two independent layers of equal shape in ONE launch (blockIdx.y picks the layer): the refiner's two heads at Track
// parts > 0 [r5]: x[h] is not the token mean but `parts` partial COLUMN SUMS [parts][C] of layernorm_pmean_kernel; the mean of
// channel c is (p0 + p1 + ... in this fixed order) / tokens (B == 1: Track)
struct SmallLinear2 {
  const float *x[2], *W[2], *bias[2];
  float *y[2];
  int parts = 0;
  float tokens = 1.f;
};
__device__ __forceinline__ float sl2_input(const SmallLinear2 &a, int h, int C, size_t idx) {
  if (a.parts == 0) return a.x[h][idx];
  float v[32];   // (parts <= 32: all loads in flight, then the fixed-order sum)
#pragma unroll
  for (int p = 0; p < 32; p++) v[p] = p < a.parts ? a.x[h][(size_t)p * C + idx] : 0.f;
  float s = v[0];
#pragma unroll
  for (int p = 1; p < 32; p++) s += v[p];
  return s / a.tokens;
}
__global__ __launch_bounds__(256) void small_linear2_kernel(const SmallLinear2 a, int B, int O, int C) {
  const int h = blockIdx.y;
  size_t widx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (widx >= (size_t)B * O) return;
  int b = (int)(widx / O), o = (int)(widx - (size_t)b * O);
  const float *W = a.W[h];
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += sl2_input(a, h, C, (size_t)b * C + c) * W[(size_t)o * C + c];
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
  if (lane == 0) a.y[h][widx] = s + a.bias[h][o];
}

// Track's last kernel: both Linear(512,3) heads (waves 0..5: one output each, the same summation as small_linear2_kernel) and, once
// they are stored, RefinePostProcess of the one hypothesis (pose_update_one) -- small_linear2_kernel + pose_update_kernel in one launch
__global__ __launch_bounds__(1024) void small_linear2_pose_kernel(const SmallLinear2 a, int C, const PoseUpdateFuse f) {
  __shared__ float out[6];
  __shared__ float xm[2][EMBED];   // the two heads' token means (from the partial sums when a.parts > 0: every thread folds a few channels)
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = wv / 3, o = wv - h * 3;
  // (constant head indices: a runtime index into the by-value argument struct would send it to scratch memory)
  // (1024 threads: one (head, channel) mean each -- with up to 25 partial sums per mean the 384-thread form walked the channels three times)
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
    if (i < C) xm[0][i] = sl2_input(a, 0, C, (size_t)i);
    else xm[1][i - C] = sl2_input(a, 1, C, (size_t)(i - C));
  }
  __syncthreads();
  if (wv < 6) {
    const float *x = xm[h], *W = a.W[h];
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += x[c] * W[(size_t)o * C + c];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k);
    if (lane == 0) {
      const float y = s + a.bias[h][o];
      a.y[h][o] = y;
      out[wv] = y;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    pose_update_one(f.poses, out, out + 3, 0, f.diameter, f.poses_in ? f.poses_in : f.poses, f.extra_out);
    // Track's completion signal: the refined pose above went to host-pinned memory; release it to the host and raise the flag the
    // waiting thread polls (an end-of-graph hipStreamSynchronize costs the host ~10 us more than this store takes to arrive)
    if (f.done_flag) __hip_atomic_store(f.done_flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
#endif  // FP_TEST_HOOKS

// cat[i][:, :, C:2C] = cat[0][:, :, C:2C] for i in 1..N-1 (bordered [N,HP,WP,2C] tensor, interior pixels only); CB = bytes
// of C channels.  Used when every hypothesis shares one observed crop (Register's first refine iteration: the sampler
// gives all 252 poses the same translation, foundationpose_sampling.cpp:388-391, so transf_input is identical for all of them).
__global__ void broadcast_b_kernel(unsigned char *__restrict__ cat, int N, int HP, int WP, int H, int W, int pad, int CB) {
  const int chunks = CB / 16;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t per_img = (size_t)H * W * chunks;
  if (i >= per_img * (size_t)(N - 1)) return;
  int img = 1 + (int)(i / per_img);
  size_t r = i - (size_t)(img - 1) * per_img;
  int pix = (int)(r / chunks), ch = (int)(r - (size_t)pix * chunks);
  int y = pix / W, x = pix - y * W;
  size_t off = (((size_t)(y + pad)) * WP + (x + pad)) * (2 * CB) + CB + ch * 16;
  const size_t img_stride = (size_t)HP * WP * 2 * CB;
  *reinterpret_cast<i4 *>(cat + (size_t)img * img_stride + off) = *reinterpret_cast<const i4 *>(cat + off);
}

template <int DT>
__global__ void cast_f32_kernel(const float *__restrict__ in, typename ElemT<DT>::t *__restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (typename ElemT<DT>::t)in[i];
}


// [r6] 8-bit operand copy of a bordered f16 tensor [imgs][HP][WP][C] (interior pixels only; the copy's border bytes were set once
// by ensure_scratch): value * oinv[c], rounded like the dual-output epilogues do.  Used where a 2-byte stage of a partly 8-bit trunk
// hands its output to an 8-bit stage (plan_trunk: qcopy) -- the 2-byte stage keeps its own kernels.  One thread = 8 channels of a pixel.
template <int QDT>
__global__ __launch_bounds__(256) void q8_copy_kernel(const _Float16 *__restrict__ x, unsigned char *__restrict__ q, const float *__restrict__ oinv,
                                                      int HP, int WP, int pad, int C, size_t octs) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= octs) return;
  const int cg = C / 8;
  const int c8 = (int)(i % cg);
  size_t px = i / cg;
  const int H = HP - 2 * pad, W = WP - 2 * pad;
  const int ow = (int)(px % W); px /= W;
  const int oh = (int)(px % H);
  const size_t img = px / H;
  const size_t e = ((img * HP + oh + pad) * WP + ow + pad) * C + c8 * 8;
  const i4 raw = *reinterpret_cast<const i4 *>(x + e);
  const float4 s0 = *reinterpret_cast<const float4 *>(oinv + c8 * 8), s1 = *reinterpret_cast<const float4 *>(oinv + c8 * 8 + 4);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = raw_elem<DT_F16>(raw, k);
  v[0] *= s0.x; v[1] *= s0.y; v[2] *= s0.z; v[3] *= s0.w; v[4] *= s1.x; v[5] *= s1.y; v[6] *= s1.z; v[7] *= s1.w;
  i2 o;
  if constexpr (QDT == DT_FP8) { o[0] = pack4_fp8(v[0], v[1], v[2], v[3]); o[1] = pack4_fp8(v[4], v[5], v[6], v[7]); }
  else { o[0] = pack4_u8(v[0], v[1], v[2], v[3]); o[1] = pack4_u8(v[4], v[5], v[6], v[7]); }
  *reinterpret_cast<i2 *>(q + e) = o;
}


// -------------------------------------------------------------------------------------------------
// First-order compensation of the INT8 weights' rounding error, per IMAGE [r5].
// A quantised 3x3 layer computes sw * sum_k q_k u_k instead of sw * sum_k v_k u_k (v = the folded weight in units of the row's step, u
// the unsigned 8-bit activation).  The MEAN over an image's pixels of the difference is sw * sum_c T[co][c] * mean_px(u_c) with
// T[co][c] = sum over the taps of channel c of (q - v): known exactly on the host, and mean_px(u_c) is a property of the image that is
// at hand on the device.  Subtracting it as a per-image bias removes the part of the 8-bit error that is common to all pixels of an
// image -- which is the part the discriminating heads amplify (the pooled token) and that differs from scene to scene: it is why a
// calibration did not carry over to frames it never saw (tools/q8_sim_cross.py: the weights, not the activations, carry that error).
//   q8_img_sum_kernel : sums[img][c] = sum over the image's padded pixels of (byte ^ 0x80) (border bytes are 0x80 = 0)
//   q8_img_bias_kernel: out[img][co] = bias[co] - cscale[co] * inv_px * sum_c Tt[c][co] * sums[img][c]     (Tt = T transposed)
// -------------------------------------------------------------------------------------------------
#ifdef FP_TEST_HOOKS   // (the three-launch form: A/B only; the product runs q8_img_bias_fused_kernel)
__global__ __launch_bounds__(256) void q8_img_sum_kernel(const unsigned char *__restrict__ x, int px_per_img, int C, int *__restrict__ sums) {
  // blockIdx.y cuts the image's pixels into gridDim.y runs; integer partial sums meet in sums[img][c] through integer atomics (order-
  // independent: the result is reproducible bit for bit); q8_img_bias_kernel consumes the sums and leaves them zero for the next layer
  __shared__ int part[256 * 16];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int lanes_per_px = C / 16;             // 16 channels (one 16-byte load) per thread
  const int cg = tid % lanes_per_px, p0 = tid / lanes_per_px, pstride = 256 / lanes_per_px;
  const int run = (px_per_img + gridDim.y - 1) / gridDim.y, px0 = blockIdx.y * run, px1 = min(px_per_img, px0 + run);
  const unsigned char *base = x + (size_t)img * px_per_img * C + cg * 16;
  int acc[16];
#pragma unroll
  for (int e = 0; e < 16; e++) acc[e] = 0;
  for (int px = px0 + p0; px < px1; px += 4 * pstride) {   // four loads in flight
    i4 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = px + j * pstride < px1 ? *reinterpret_cast<const i4 *>(base + (size_t)(px + j * pstride) * C) : (i4){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[e] += (int)((((unsigned)v[j][e >> 2] >> ((e & 3) * 8)) & 0xffu) ^ 0x80u);
  }
#pragma unroll
  for (int e = 0; e < 16; e++) part[e * 256 + tid] = acc[e];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int g = c / 16, e = c % 16;
    int t = 0;
    for (int j = 0; j < pstride; j++) t += part[e * 256 + j * lanes_per_px + g];
    if (t) atomicAdd(sums + (size_t)img * C + c, t);
  }
}
__global__ __launch_bounds__(256) void q8_img_bias_kernel(int *__restrict__ sums, const float *__restrict__ tmat_t, const float *__restrict__ cscale,
                                                          const float *__restrict__ bias, float inv_px, int Cin, int Cout, float *__restrict__ out) {
  // grid (image, Cout / 64): 64 output channels per workgroup, the input channels split over its four waves (a thread's loads are
  // independent: 16 in flight), fixed-order reduction over the waves; the LAST channel block of an image clears its sums for the next layer
  __shared__ float m[512];
  __shared__ float part[4][64];
  const int img = blockIdx.x, co = blockIdx.y * 64 + (threadIdx.x & 63), cs = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < Cin; c += 256) m[c] = (float)sums[(size_t)img * Cin + c];   // (no float arithmetic here: the loop vectoriser would emit v_pk_mul_f32, tests/test_isa_cpu.py)
  __syncthreads();
  const int c0 = cs * (Cin / 4), c1 = c0 + Cin / 4;
  float a = 0.f;
  for (int c = c0; c < c1; c += 16) {
    float t[16];
#pragma unroll
    for (int j = 0; j < 16; j++) t[j] = tmat_t[(size_t)(c + j) * Cout + co];
#pragma unroll
    for (int j = 0; j < 16; j++) a = __builtin_fmaf(t[j], m[c + j], a);
  }
  part[cs][threadIdx.x & 63] = a;
  __syncthreads();
  if (cs == 0) {
    const float tot = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    out[(size_t)img * Cout + co] = bias[co] - cscale[co] * (tot * inv_px);
  }
}
#endif

// [r5] both steps in ONE launch, one 1024-thread workgroup per image: the channel sums of the image (phase 1) and its per-image bias
// (phase 2).  Three dependent launches per layer (sums, bias, clearing the sums) cost more in launch latency than in work: 13 layers x 3
// launches were 0.83 ms of an 8.5 ms Register.  No atomics, no state between layers: bit-reproducible.
// wp2 > 0: the sums run over the lattice of even rows and even columns only (wp2 = padded width / 2; px_per_img = the number of lattice
// points, inv_px = 1 / the interior ones among them): a quarter of the bytes for a mean whose sampling error is a few per cent of a channel's
// standard deviation -- an order below the scene-to-scene deviation the compensation exists to remove.
// [r5b] IMGS = 4 images per workgroup: the [Cin][Cout] f32 table of a 512 x 512 layer is 1 MB, and one workgroup per image re-read it
// from L2 252 times per launch (1.5 GB over the 13 layers: what the kernel's 0.52 ms per Register were); four images share every load.
constexpr int Q8_BIAS_IMGS = 4;
__global__ __launch_bounds__(1024) void q8_img_bias_fused_kernel(const unsigned char *__restrict__ x, int px_per_img, const float *__restrict__ tmat_t,
                                                                 const float *__restrict__ cscale, const float *__restrict__ bias, float inv_px, int Cin,
                                                                 int Cout, float *__restrict__ out, int wp2, int img_px, int n_img) {
  constexpr int IMGS = Q8_BIAS_IMGS;
  __shared__ int part[16 * 1024];          // phase 1: [16 channels of a thread][thread]; phase 2 (as float4): [image][c-slice][Cout / 4]
  __shared__ float m[IMGS][512];
  const int img0 = blockIdx.x * IMGS, tid = threadIdx.x;
  {   // phase 1: 256 threads per image, the four images side by side
    static_assert(IMGS == 4, "1024 threads = 4 images x 256");
    const int ii = tid >> 8, t2 = tid & 255;
    const int img = min(img0 + ii, n_img - 1);   // (a short last group repeats its last image; only valid images are stored)
    const int lanes_per_px = Cin / 16, cg = t2 % lanes_per_px, p0 = t2 / lanes_per_px, pstride = 256 / lanes_per_px;
    const unsigned char *base = x + (size_t)img * img_px * Cin + cg * 16;
    auto pixel = [&](int s) { return wp2 > 0 ? (2 * (s / wp2)) * (2 * wp2) + 2 * (s % wp2) : s; };   // lattice point s -> pixel index in the padded image
    int acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0;
    for (int px = p0; px < px_per_img; px += 8 * pstride) {   // eight loads in flight
      i4 v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = px + j * pstride < px_per_img ? *reinterpret_cast<const i4 *>(base + (size_t)pixel(px + j * pstride) * Cin) : (i4){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
#pragma unroll
      for (int j = 0; j < 8; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] += (int)((((unsigned)v[j][e >> 2] >> ((e & 3) * 8)) & 0xffu) ^ 0x80u);
    }
#pragma unroll
    for (int e = 0; e < 16; e++) part[e * 1024 + tid] = acc[e];
    __syncthreads();
    for (int o = tid; o < IMGS * Cin; o += 1024) {
      const int i2 = o / Cin, c = o - i2 * Cin, g = c / 16, e = c % 16;
      int t = 0;
      for (int j = 0; j < pstride; j++) t += part[e * 1024 + i2 * 256 + j * lanes_per_px + g];
      m[i2][c] = (float)t;
    }
    __syncthreads();
  }
  // phase 2: a thread owns FOUR output channels (one 16-byte load per input channel) of a slice of the input channels, for all the
  // workgroup's images: Cout / 4 threads per slice, 4096 / Cout slices (8 / 16 / 32 for Cout 512 / 256 / 128)
  float4 *fpart = reinterpret_cast<float4 *>(part);
  const int tps = Cout / 4, nslice = 1024 / tps, q4 = tid % tps, cs = tid / tps;
  const int per = Cin / nslice, c0 = cs * per;
  float4 a[IMGS];
#pragma unroll
  for (int ii = 0; ii < IMGS; ii++) a[ii] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = c0; c < c0 + per; c += 8) {
    float4 t[8];   // (16 per batch spills: 1024 threads leave 128 registers)
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = j < per ? *reinterpret_cast<const float4 *>(tmat_t + (size_t)(c + j) * Cout + q4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int ii = 0; ii < IMGS; ii++) {
        const float mv = j < per ? m[ii][c + j] : 0.f;
        a[ii].x = __builtin_fmaf(t[j].x, mv, a[ii].x); a[ii].y = __builtin_fmaf(t[j].y, mv, a[ii].y);
        a[ii].z = __builtin_fmaf(t[j].z, mv, a[ii].z); a[ii].w = __builtin_fmaf(t[j].w, mv, a[ii].w);
      }
  }
#pragma unroll
  for (int ii = 0; ii < IMGS; ii++) fpart[(ii * nslice + cs) * tps + q4] = a[ii];
  __syncthreads();
  const float *fp1 = reinterpret_cast<const float *>(part);
  for (int o = tid; o < IMGS * Cout; o += 1024) {
    const int ii = o / Cout, co = o - ii * Cout;
    if (img0 + ii >= n_img) break;
    float tot = fp1[(size_t)ii * nslice * Cout + co];
    for (int sl = 1; sl < nslice; sl++) tot += fp1[((size_t)ii * nslice + sl) * Cout + co];
    out[(size_t)(img0 + ii) * Cout + co] = bias[co] - cscale[co] * (tot * inv_px);
  }
}
