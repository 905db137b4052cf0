// fp_nn_attention_kernels.inc -- the attention kernels (device code)
// Part of the fp_nn.hip translation unit (included there, inside namespace fp unless stated): kernel templates must be visible
// where they are launched, so this is a textual split, not a separate compilation unit.

// =================================================================================================
// attention: out[b,t,h*128+d] = softmax_k(q.k/sqrt(128)) v,  qkv = [B,T,1536] (q|k|v, heads contiguous inside each)
// =================================================================================================

// -------------------------------------------------------------------------------------------------
// attention32_kernel [r2]: the round-1 kernel (attention_kernel, retired; EXPERIMENTS.md) was LDS-bandwidth-bound -- a wave owned ONE
// 16-row query tile, so every 32-key block cost it the whole K and V tile (16 KB of fragment reads) for 16 MFMAs, 2.4x what the LDS
// delivers at the MFMA rate, plus sixteen 2-byte transposing LDS writes per thread.  Here:
//   * a wave owns 32 query rows (two 16-row tiles): every K / V fragment feeds two MFMAs (LDS bytes per MFMA halved),
//     a workgroup = 4 waves = 128 query rows (4 workgroups per 400-token sequence and head instead of 7: K/V staged 4x);
//   * O is accumulated TRANSPOSED, O^T[d][q] = V^T P^T: a lane owns one query in S^T and in O^T alike, so the online-softmax
//     rescale is a lane-local multiply (no shuffles) and P^T feeds the MFMA's B operand straight from the softmax registers;
//   * V stays row-major in LDS (16-byte staging writes) and the V^T operand comes from ds_read_b64_tr_b16 (hardware
//     transpose read): [32 keys][16 d] sub-tiles of 1 KB (+32 B so the staging writes of one instruction spread over all
//     banks), a 16-lane group reads one [4 keys][16 d] block = 128 contiguous bytes;
//   * K rows (256 B) are XOR-swizzled by 16-byte slot (slot ^= key & 15): conflict-free staging writes and fragment reads;
//   * two LDS buffers, ONE barrier per key block: tile kb+1 is written (from registers loaded three iterations earlier [r4]) while
//     tile kb is consumed, the global loads of tiles kb+2 / kb+3 are in flight (two register sets);
//   * all K fragments of a block are requested at once, all V^T fragments right after the QK MFMAs so their latency runs under the
//     softmax (asm reads + one explicit wait: hipcc otherwise sinks each read to its first use); the cross-row max / sum use
//     v_permlane16/32_swap instead of four LDS round trips (ds_bpermute) per softmax;
//   * O leaves through LDS as whole 256-byte rows.
// -------------------------------------------------------------------------------------------------
typedef short s4 __attribute__((ext_vector_type(4)));
// reductions over the four 16-lane rows of a wave (lanes li, li+16, li+32, li+48) on the VALU: v_permlane16_swap exchanges rows
// 0<->1 and 2<->3, v_permlane32_swap the two halves (ds_bpermute shuffles put four LDS round trips per softmax on the
// critical path of every key block)
__device__ __forceinline__ float vmax_f32(float a, float b) {  // (fmaxf would be preceded by two canonicalising v_max)
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float rows_max(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float m = vmax_f32(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return vmax_f32(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float rows_sum(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float m = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// NW waves = NW * 32 query rows per workgroup; ABL (timing ablations, wrong results): 1 no staging after the first tile, 2 no softmax, 4 no PV,
// 8 no QK.  Nothing instantiates NW != 4 (8 waves: 9 % slower, the two waves of a SIMD run in lockstep) or ABL & 64 (below) any more; the two
// stay in the signature because the product instantiations compile to other code without either (four v_mov move by one slot each).
template <bool REMAP, int DT, int ABL = 0, int NW = 4>
__global__ __launch_bounds__(NW * 64, 2) void attention32_kernel(const typename ElemT<DT>::t *__restrict__ qkv, typename ElemT<DT>::t *__restrict__ out, int T, int nq,
                                                             int tstride /* rows between the first tokens of consecutive sequences */,
                                                             int qkv_ld /* elements between consecutive qkv rows (>= 1536) */) {
  using E = typename ElemT<DT>::t;
  using E8 = typename ElemT<DT>::v8;
  constexpr int KB = 32 * 256;   // K tile: 32 keys x 128 d
  constexpr int VSUB = 1056;     // V sub-tile [32 keys][16 d] + 32 B
  constexpr int BUF = KB + 8 * VSUB;
  constexpr int NJ = 512 / (NW * 64);  // 16-byte chunks of K (and of V) a thread stages per tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF > NW * 8192 ? 2 * BUF : NW * 8192];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int logical;
  {
    const int nblk = gridDim.x, bi = blockIdx.x;
    const int xcd = bi & 7, within = bi >> 3, q = nblk >> 3, r = nblk & 7;
    logical = REMAP ? (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within : bi;
  }
  const int qt = logical % nq, h = (logical / nq) % HEADS, b = logical / (nq * HEADS);
  const int g = lane >> 4, li = lane & 15;
  const size_t rowstride = (size_t)qkv_ld;
  const E *base = qkv + (size_t)b * tstride * rowstride + h * HDIM;
  const int q0 = qt * (NW * 32) + wave * 32;
  const bool active = q0 < T;  // (wave-uniform) waves past the sequence only help staging

  i4 qf[2][4];
#pragma unroll
  for (int qi = 0; qi < 2; qi++) {
    const int q_ld = min(q0 + qi * 16 + li, T - 1);
#pragma unroll
    for (int ds = 0; ds < 4; ds++) qf[qi][ds] = *reinterpret_cast<const i4 *>(base + (size_t)q_ld * rowstride + ds * 32 + g * 8);
  }
  f4 o[8][2];
#pragma unroll
  for (int dt = 0; dt < 8; dt++)
#pragma unroll
    for (int qi = 0; qi < 2; qi++) o[dt][qi] = (f4){0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  const float sl2e = 0.08838834764831845f * 1.4426950408889634f;  // 1/sqrt(128) * log2(e)

  // staging: thread -> (key = idx >> 4, 16-byte chunk = idx & 15), idx = tid + 256 j: coalesced 256-byte rows
  const int nkb = (T + 31) / 32;
  // three register sets: tile kb+1 (written to LDS during block kb), tiles kb+2 and kb+3 in flight -- a tile's loads have three blocks
  // to arrive (with two sets the staging-only pipeline and the compute-only pipeline added up: tools/bench_attn.py V=17,30)
  i4 kreg[3][NJ], vreg[3][NJ];
  auto load_tile = [&](int kb, i4 (&kr)[NJ], i4 (&vr)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int idx = tid + j * (NW * 64);
      const int row = min(kb * 32 + (idx >> 4), T - 1);
      const E *src = base + (size_t)row * rowstride + (idx & 15) * 8;
      // asm loads: the compiler's own vmcnt bookkeeping collapses to vmcnt(0) at the joins of this loop (every store_tile then waited
      // for the tile requested one block earlier); the waits are counted by hand in wait_tile
      asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(kr[j]) : "v"(src), "n"(EMBED * (int)sizeof(E)));
      asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(vr[j]) : "v"(src), "n"(2 * EMBED * (int)sizeof(E)));
    }
  };
  // the set's 2 NJ loads have landed when at most `newer` younger loads are outstanding (vmcnt retires in order)
  auto wait_tile = [&](int newer_tiles, i4 (&kr)[NJ], i4 (&vr)[NJ]) {
    if (newer_tiles >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NJ) : "memory");
    else if (newer_tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NJ) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < NJ; j++) asm volatile("" : "+v"(kr[j]), "+v"(vr[j]));
  };
  auto store_tile = [&](int buf, const i4 (&kr)[NJ], const i4 (&vr)[NJ]) {
    unsigned char *sb = smem + buf * BUF;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int idx = tid + j * (NW * 64);
      const int key = idx >> 4, chunk = idx & 15;
      *reinterpret_cast<i4 *>(sb + key * 256 + ((chunk ^ (key & 15)) << 4)) = kr[j];
      *reinterpret_cast<i4 *>(sb + KB + (chunk >> 1) * VSUB + key * 32 + (chunk & 1) * 16) = vr[j];
    }
  };
  load_tile(0, kreg[0], vreg[0]);
  wait_tile(0, kreg[0], vreg[0]);
#pragma unroll
  for (int qi = 0; qi < 2; qi++)  // a use of Q the compiler sees: its own wait for these loads happens here, not in front of the MFMAs of every block
#pragma unroll
    for (int ds = 0; ds < 4; ds++) asm volatile("" : "+v"(qf[qi][ds]));
  store_tile(0, kreg[0], vreg[0]);
  if (!(ABL & 1)) {  // (loads nobody consumes would land in registers the compiler has already handed out again)
    if (nkb > 1) load_tile(1, kreg[1], vreg[1]);   // tile t travels in set t % 3
    if (nkb > 2) load_tile(2, kreg[2], vreg[2]);
    if (nkb > 3) load_tile(3, kreg[0], vreg[0]);
  }
  __syncthreads();

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  unsigned koff[4];
#pragma unroll
  for (int ds = 0; ds < 4; ds++) koff[ds] = (unsigned)(li * 256 + (((ds * 4 + g) ^ li) << 4));
  const unsigned voff = (unsigned)((g * 4 + (li >> 2)) * 32 + (li & 3) * 8);

  auto block = [&](const int kb, i4 (&kr)[NJ], i4 (&vr)[NJ]) {   // kr / vr hold tile kb+1 on entry, tile kb+4 on exit
    f4 st[2][2];  // [query tile][key tile]: st[qi][kt][r] = S[key = kt*16 + g*4 + r][q = qi*16 + li]
    if (ABL & 8) {
#pragma unroll
      for (int qi = 0; qi < 2; qi++)
#pragma unroll
        for (int kt = 0; kt < 2; kt++) st[qi][kt] = __builtin_bit_cast(f4, qf[qi][kt]);
    } else if (active) {
#pragma unroll
      for (int qi = 0; qi < 2; qi++)
#pragma unroll
        for (int kt = 0; kt < 2; kt++) st[qi][kt] = (f4){0.f, 0.f, 0.f, 0.f};
      // all K fragments of the block in one go (one LDS latency, then 16 MFMAs back to back).  The reads are asm statements: hipcc
      // otherwise sinks every read to its first use and waits after each small group
      i4 kf[2][4];
      const unsigned kbase = lds0 + (unsigned)((kb & 1) * BUF);
#pragma unroll
      for (int ds = 0; ds < 4; ds++) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(kf[0][ds]) : "v"(kbase + koff[ds]));
        asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(kf[1][ds]) : "v"(kbase + koff[ds]));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int ds = 0; ds < 4; ds++)
#pragma unroll
          for (int qi = 0; qi < 2; qi++) st[qi][kt] = mfma32<DT>(kf[kt][ds], qf[qi][ds], st[qi][kt]);
    }
    // V^T fragments of this block: requested now, consumed after the softmax (their latency runs under it)
    i2 vlo[8], vhi[8];
    if (active && !(ABL & 4)) {
      const unsigned vbase = lds0 + (unsigned)((kb & 1) * BUF + KB) + voff;
#pragma unroll
      for (int dt = 0; dt < 8; dt++) {
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vlo[dt]) : "v"(vbase), "n"(dt * VSUB));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vhi[dt]) : "v"(vbase), "n"(dt * VSUB + 512));
      }
    }
    // the next tile goes into the other buffer (its last readers passed the barrier that ended the previous iteration)
    if (kb + 1 < nkb && !(ABL & 1)) {
      if (ABL & 32) {
#pragma unroll
        for (int j = 0; j < NJ; j++) asm volatile("" ::"v"(kr[j]), "v"(vr[j]));
      } else {
        wait_tile(ABL & 16 ? 0 : min(2, nkb - 2 - kb), kr, vr);  // tiles kb+2, kb+3 (where they exist) were requested after this one
        store_tile((kb + 1) & 1, kr, vr);
      }
      if (kb + 4 < nkb && !(ABL & 16)) load_tile(kb + 4, kr, vr);
    }
    if (active) {
      i4 pf[2];
      if (ABL & 2) {
#pragma unroll
        for (int qi = 0; qi < 2; qi++) pf[qi] = __builtin_bit_cast(i4, st[qi][0] + st[qi][1]);
      } else
#pragma unroll
      for (int qi = 0; qi < 2; qi++) {
        // softmax in base 2 on the RAW scores: p = exp2(s*c - m*c), c = scale*log2(e); keys past T exist only in the last block
        if (kb == nkb - 1 && (T & 31)) {
#pragma unroll
          for (int kt = 0; kt < 2; kt++)
#pragma unroll
            for (int r = 0; r < 4; r++)
              if (kb * 32 + kt * 16 + g * 4 + r >= T) st[qi][kt][r] = -INFINITY;
        }
        float mx = vmax_f32(vmax_f32(vmax_f32(st[qi][0][0], st[qi][0][1]), vmax_f32(st[qi][0][2], st[qi][0][3])),
                            vmax_f32(vmax_f32(st[qi][1][0], st[qi][1][1]), vmax_f32(st[qi][1][2], st[qi][1][3])));
        mx = rows_max(mx);
        // (ABL 64, no longer instantiated: a LAZY reference -- it only moves when the block maximum exceeds it by more than 2^8, which skips
        // most of the 64-multiply rescales of O^T: 213 -> 204 us per launch.  Not shipped: mathematically the same, but a row whose threshold
        // decision flips under a 1e-3 perturbation of its inputs gets a different f16 rounding of ALL its P values, and the score-net's
        // pooled feature then moves by up to 1.3x the between-hypothesis spread between a shard of 32 and the full batch;
        // with the exact running maximum the rounding pattern is shared and the two agree to 0.12x.)
        const float m_new = (ABL & 64) ? ((mx * sl2e > m_run[qi] * sl2e + 8.0f) ? mx : m_run[qi]) : vmax_f32(m_run[qi], mx);
        const float mc = m_new * sl2e;
        const float alpha = __builtin_amdgcn_exp2f(m_run[qi] * sl2e - mc);  // m_run = -inf on the first block -> 0
        float psum = 0.f;
        E8 pv8;
#pragma unroll
        for (int kt = 0; kt < 2; kt++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qi][kt][r], sl2e, -mc));
            psum += pv;
            pv8[kt * 4 + r] = (E)pv;
          }
        pf[qi] = __builtin_bit_cast(i4, pv8);
        psum = rows_sum(psum);
        l_run[qi] = l_run[qi] * alpha + psum;
        m_run[qi] = m_new;
        // O^T columns of this lane all belong to query li: the rescale is lane-local; x * 1.0f is exact, so it is skipped
        // when no row's running maximum moved (most blocks after the first few)
        if (__any(alpha != 1.0f)) {
#pragma unroll
          for (int dt = 0; dt < 8; dt++)
#pragma unroll
            for (int r = 0; r < 4; r++) o[dt][qi][r] *= alpha;
        }
      }
      // O^T[d][q] += V^T[d][key] P^T[key][q]; k-slot j of lane group g is key (j>>2)*16 + g*4 + (j&3) in both operands
      if (ABL & 4) {
#pragma unroll
        for (int qi = 0; qi < 2; qi++) o[0][qi] += __builtin_bit_cast(f4, pf[qi]);
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
        for (int dt = 0; dt < 8; dt++) {
          const i4 vf = (i4){vlo[dt][0], vlo[dt][1], vhi[dt][0], vhi[dt][1]};
#pragma unroll
          for (int qi = 0; qi < 2; qi++) o[dt][qi] = mfma32<DT>(vf, pf[qi], o[dt][qi]);
        }
        }
    }
    __syncthreads();
  };
  for (int kb = 0; kb < nkb; kb += 3) {
    block(kb, kreg[1], vreg[1]);
    if (kb + 1 < nkb) block(kb + 1, kreg[2], vreg[2]);
    if (kb + 2 < nkb) block(kb + 2, kreg[0], vreg[0]);
  }
  if (!active) return;
  // O tile of the wave through LDS (both buffers are free now; 8 KB per wave) -> whole 256-byte rows
  unsigned char *ob = smem + wave * 8192;
#pragma unroll
  for (int qi = 0; qi < 2; qi++) {
    const float inv = 1.0f / l_run[qi];
    const int row = qi * 16 + li;
#pragma unroll
    for (int dt = 0; dt < 8; dt++) {
      typename ElemT<DT>::v4 ov;
#pragma unroll
      for (int r = 0; r < 4; r++) ov[r] = (E)(o[dt][qi][r] * inv);
      // d = dt*16 + g*4 + r: 16-byte slot dt*2 + (g>>1), swizzled by the row
      *reinterpret_cast<typename ElemT<DT>::v4 *>(ob + row * 256 + (((dt * 2 + (g >> 1)) ^ (row & 15)) << 4) + (g & 1) * 8) = ov;
    }
  }
#pragma unroll
  for (int it = 0; it < 8; it++) {
    const int id = it * 64 + lane, rr = id >> 4, c = id & 15;
    const int row = q0 + rr;
    const i4 v = *reinterpret_cast<const i4 *>(ob + rr * 256 + ((c ^ (rr & 15)) << 4));
    if (row < T) *reinterpret_cast<i4 *>(out + ((size_t)b * tstride + row) * EMBED + h * HDIM + c * 8) = v;
  }
}

// -------------------------------------------------------------------------------------------------
// attention32_skv_kernel [r2]: the same arithmetic for SMALL grids (Track: 2 sequences; the score-net's cross attention: one),
// where a workgroup of attention32_kernel is a latency chain of T/32 key blocks on a mostly idle chip.  One workgroup per 32
// query rows; its four waves split the KEY blocks (wave w takes blocks w, w+4, ...) and run independently -- private LDS
// double buffers filled by LDS-DMA (K rows swizzled on the source side, V in the transpose-read sub-tile layout), no workgroup
// barrier in the loop -- then merge their partial (max, sum, O) through LDS: chain length T/128 blocks, 3.25x more workgroups.
// -------------------------------------------------------------------------------------------------
template <bool REMAP, int DT>
__global__ __launch_bounds__(256, 2) void attention32_skv_kernel(const typename ElemT<DT>::t *__restrict__ qkv, typename ElemT<DT>::t *__restrict__ out, int T, int nq,
                                                                 int tstride, int qkv_ld, int qt0 = 0 /* first 32-row query tile this launch covers */) {
  using E = typename ElemT<DT>::t;
  using E8 = typename ElemT<DT>::v8;
  constexpr int KB = 32 * 256, VSUB = 1056, BUF = KB + 8 * VSUB, WREG = 2 * BUF;  // per wave: two tile buffers (33 280 B)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int logical;
  {
    const int nblk = gridDim.x, bi = blockIdx.x;
    const int xcd = bi & 7, within = bi >> 3, q = nblk >> 3, r = nblk & 7;
    logical = REMAP ? (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within : bi;
  }
  const int qt = logical % nq, h = (logical / nq) % HEADS, b = logical / (nq * HEADS);
  const int g = lane >> 4, li = lane & 15;
  const size_t rowstride = (size_t)qkv_ld;
  const E *base = qkv + (size_t)b * tstride * rowstride + h * HDIM;
  const int q0 = (qt0 + qt) * 32;
  unsigned char *wbuf = smem_dyn + wave * WREG;
  const unsigned wlds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)wbuf;

  i4 qf[2][4];
#pragma unroll
  for (int qi = 0; qi < 2; qi++) {
    const int q_ld = min(q0 + qi * 16 + li, T - 1);
#pragma unroll
    for (int ds = 0; ds < 4; ds++) qf[qi][ds] = *reinterpret_cast<const i4 *>(base + (size_t)q_ld * rowstride + ds * 32 + g * 8);
  }
  f4 o[8][2];
#pragma unroll
  for (int dt = 0; dt < 8; dt++)
#pragma unroll
    for (int qi = 0; qi < 2; qi++) o[dt][qi] = (f4){0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  const float sl2e = 0.08838834764831845f * 1.4426950408889634f;

  const int nkb = (T + 31) / 32;
  // one wave stages a whole tile: 8 LDS-DMA instructions for K (4 keys x 256 B each; the lane at LDS slot s of key k fetches
  // chunk s ^ (k & 15)) and 8 for V (one [32 keys][16 d] sub-tile each: lane -> key lane>>1, 8-d half lane&1)
  auto issue_tile = [&](int kb, int bufi) {
    const unsigned dst = __builtin_amdgcn_readfirstlane(wlds + bufi * BUF);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int key = i * 4 + (lane >> 4);
      const int row = min(kb * 32 + key, T - 1);
      const E *src = base + (size_t)row * rowstride + EMBED + (((lane & 15) ^ (key & 15)) * 8);
      glds16_asm(src, dst + i * 1024);
    }
#pragma unroll
    for (int dt = 0; dt < 8; dt++) {
      const int row = min(kb * 32 + (lane >> 1), T - 1);
      const E *src = base + (size_t)row * rowstride + 2 * EMBED + dt * 16 + (lane & 1) * 8;
      glds16_asm(src, dst + KB + dt * VSUB);
    }
  };
  unsigned koff[4];
#pragma unroll
  for (int ds = 0; ds < 4; ds++) koff[ds] = (unsigned)(li * 256 + (((ds * 4 + g) ^ li) << 4));
  const unsigned voff = (unsigned)((g * 4 + (li >> 2)) * 32 + (li & 3) * 8);

  int bufi = 0;
  if (wave < nkb) issue_tile(wave, 0);
  for (int kb = wave; kb < nkb; kb += 4, bufi ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's tile kb has landed (only this wave reads it)
    if (kb + 4 < nkb) issue_tile(kb + 4, bufi ^ 1);    // (its last reads finished an iteration ago: lgkmcnt(0) below)
    f4 st[2][2];
#pragma unroll
    for (int qi = 0; qi < 2; qi++)
#pragma unroll
      for (int kt = 0; kt < 2; kt++) st[qi][kt] = (f4){0.f, 0.f, 0.f, 0.f};
    i4 kf[2][4];
    const unsigned kbase = wlds + (unsigned)(bufi * BUF);
#pragma unroll
    for (int ds = 0; ds < 4; ds++) {
      asm volatile("ds_read_b128 %0, %1" : "=v"(kf[0][ds]) : "v"(kbase + koff[ds]));
      asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(kf[1][ds]) : "v"(kbase + koff[ds]));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
      for (int ds = 0; ds < 4; ds++)
#pragma unroll
        for (int qi = 0; qi < 2; qi++) st[qi][kt] = mfma32<DT>(kf[kt][ds], qf[qi][ds], st[qi][kt]);
    i2 vlo[8], vhi[8];
    {
      const unsigned vbase = kbase + KB + voff;
#pragma unroll
      for (int dt = 0; dt < 8; dt++) {
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vlo[dt]) : "v"(vbase), "n"(dt * VSUB));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vhi[dt]) : "v"(vbase), "n"(dt * VSUB + 512));
      }
    }
    i4 pf[2];
#pragma unroll
    for (int qi = 0; qi < 2; qi++) {
      if (kb == nkb - 1 && (T & 31)) {
#pragma unroll
        for (int kt = 0; kt < 2; kt++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (kb * 32 + kt * 16 + g * 4 + r >= T) st[qi][kt][r] = -INFINITY;
      }
      float mx = vmax_f32(vmax_f32(vmax_f32(st[qi][0][0], st[qi][0][1]), vmax_f32(st[qi][0][2], st[qi][0][3])),
                          vmax_f32(vmax_f32(st[qi][1][0], st[qi][1][1]), vmax_f32(st[qi][1][2], st[qi][1][3])));
      mx = rows_max(mx);
      const float m_new = vmax_f32(m_run[qi], mx);
      const float mc = m_new * sl2e;
      const float alpha = __builtin_amdgcn_exp2f(m_run[qi] * sl2e - mc);
      float psum = 0.f;
      E8 pv8;
#pragma unroll
      for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qi][kt][r], sl2e, -mc));
          psum += pv;
          pv8[kt * 4 + r] = (E)pv;
        }
      pf[qi] = __builtin_bit_cast(i4, pv8);
      psum = rows_sum(psum);
      l_run[qi] = l_run[qi] * alpha + psum;
      m_run[qi] = m_new;
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int dt = 0; dt < 8; dt++)
#pragma unroll
          for (int r = 0; r < 4; r++) o[dt][qi][r] *= alpha;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < 8; dt++) {
      const i4 vf = (i4){vlo[dt][0], vlo[dt][1], vhi[dt][0], vhi[dt][1]};
#pragma unroll
      for (int qi = 0; qi < 2; qi++) o[dt][qi] = mfma32<DT>(vf, pf[qi], o[dt][qi]);
    }
  }
  // ---- merge the four partial results: O = sum_v O_v 2^((m_v - M) c) / sum_v l_v 2^((m_v - M) c)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float *po = reinterpret_cast<float *>(wbuf);                  // [32 q][128 d] f32, 16-byte slots XOR-swizzled by the row
  float *pml = reinterpret_cast<float *>(wbuf + 32 * 512);      // [2][32]: m, l
#pragma unroll
  for (int qi = 0; qi < 2; qi++) {
    const int q = qi * 16 + li;
#pragma unroll
    for (int dt = 0; dt < 8; dt++)
      *reinterpret_cast<f4 *>(reinterpret_cast<unsigned char *>(po) + q * 512 + (((dt * 4 + g) ^ (q & 31)) << 4)) = o[dt][qi];
    if (g == 0) { pml[q] = m_run[qi]; pml[32 + q] = l_run[qi]; }
  }
  __syncthreads();
  {
    const int r8 = lane >> 3, c = lane & 7;     // this wave merges query rows wave*8 .. wave*8+7; a lane: one row, 16 d
    const int q = wave * 8 + r8;
    float mv[4], lv[4], M = -INFINITY;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const float *ml = reinterpret_cast<const float *>(smem_dyn + v * WREG + 32 * 512);
      mv[v] = ml[q]; lv[v] = ml[32 + q];
      M = fmaxf(M, mv[v]);
    }
    float L = 0.f, acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.f;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const float w = __builtin_amdgcn_exp2f((mv[v] - M) * sl2e);   // a wave without key blocks: m = -inf -> weight 0
      L += lv[v] * w;
      const unsigned char *pv = smem_dyn + v * WREG + q * 512;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const f4 x = *reinterpret_cast<const f4 *>(pv + (((c * 4 + j) ^ (q & 31)) << 4));
#pragma unroll
        for (int e = 0; e < 4; e++) acc[j * 4 + e] += x[e] * w;
      }
    }
    const float inv = 1.0f / L;
    const int row = q0 + q;
    if (row < T) {
      E8 o0, o1;
#pragma unroll
      for (int e = 0; e < 8; e++) { o0[e] = (E)(acc[e] * inv); o1[e] = (E)(acc[8 + e] * inv); }
      E *dst = out + ((size_t)b * tstride + row) * EMBED + h * HDIM + c * 16;
      *reinterpret_cast<E8 *>(dst) = o0;
      *reinterpret_cast<E8 *>(dst + 8) = o1;
    }
  }
}

