// fp_nn_conv_kernels.inc -- the convolution / Linear schedules (device code) of the refine-net and score-net
// Part of the fp_nn.hip translation unit (included there, inside namespace fp unless stated): kernel templates must be visible
// where they are launched, so this is a textual split, not a separate compilation unit.

// =================================================================================================
// implicit-GEMM convolution
// =================================================================================================

// LDS-DMA issued from inline asm: hipcc neither counts these loads nor inserts its conservative `s_waitcnt vmcnt(0)`
// in front of a new LDS-DMA while an older one is in flight (it cannot tell the LDS stages apart), so the counted
// waits in the hand-scheduled kernels are authoritative.  M0 (LDS destination base) is saved and restored inside the statement
// (cdna_hip_programming.md §5.7).  lds_addr must be wave-uniform; the 16 bytes land at lds_addr + lane*16.
__device__ __forceinline__ void glds16_asm(const void *gsrc, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}
// FOUR consecutive 1 KB pieces with ONE M0 set-up: the instruction's immediate offset is added to the global address AND to the
// LDS address, so a source that is stored in LDS order (pack_gemm_w) needs no per-piece address arithmetic and no per-piece
// M0 save / set / restore.  The 4 KB land at lds_addr + lane*16 + {0, 1024, 2048, 3072}.
__device__ __forceinline__ void glds16x2_asm(const void *gsrc, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}
__device__ __forceinline__ void glds16x4_asm(const void *gsrc, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\t"
               "global_load_lds_dwordx4 %1, off offset:2048\n\tglobal_load_lds_dwordx4 %1, off offset:3072\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}
// the same with the non-temporal cache policy, for the input tiles of the resident-halo kernels (each tile is staged once per
// 64-channel chunk by at most two workgroups).  A/B build switch FP_X_NT (tools/ab_xnt.sh), OFF: measured [r3] the halo layers move
// by -4...+1 %, inside the run-to-run noise of a box (+-3 %); the same policy on the X tiles of conv_big_pp / gemm_k32, which other
// n-tiles re-read from L2, costs +4 % / +17 %.
#ifndef FP_X_NT
#define FP_X_NT 0
#endif
__device__ __forceinline__ void glds16_asm_x(const void *gsrc, unsigned lds_addr) {
#if FP_X_NT
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
#else
  glds16_asm(gsrc, lds_addr);
#endif
}

struct ConvParams {
  const unsigned char *in;   // [NB, H+2*ipad, W+2*ipad, Cin]  (zero border of width ipad >= pad is physically present)
  const unsigned char *w;    // [Cout][K] in kernel K order (relayout_k), element type = the kernel's DT
  const unsigned char *wfrag;  // the same weights in MFMA-fragment order (fragment_order; conv_smallm_kernel only), or null
  const unsigned char *wpack;  // the same weights in the LDS-stage order of gemm_k32_kernel (1x1 layers) / conv_halo_kernel (3x3) (pack_stage_w), or null
  const unsigned char *wpack128;  // ... in conv_big_pp_kernel's stage order (pack_stage_w128), or null
  const unsigned char *wdeep;     // ... in conv_deep_kernel's stage order (pack_stage_w128 with 128-row tiles, 4 waves), or null
  const float *bias;         // [Cout]
  const float *bias_img;     // INT8 layers [r5]: per-IMAGE bias [NB][Cout] = bias - the first-order compensation of the weights' rounding error
                             // for that image's channel means (q8_img_bias_kernel); null = the shared bias
  const float *cscale;       // FP8 input: [Cout] activation scale * weight scale of the channel; null otherwise
  const unsigned char *res;  // optional residual [NB, OH+2*rpad, OW+2*rpad, res_ld], element type res_dt
  unsigned char *out;        // [NB', OH+2*opad, OW+2*opad, out_ld], element type out_dt
  unsigned char *out2;       // DT_DUAL_* outputs: the 8-bit copy (same shape, 1 byte per element); null otherwise
  const float *rscale;       // DT_QSR_I8 / DT_F16RQ_I8: [res_ld] per-channel scale of the 8-bit residual tensor (value = (byte ^ 0x80) * rscale[c])
  const float *oinv;         // DT_DUAL_* outputs: [out_ld channels... indexed by the layer's OUTPUT channel] 1 / scale of the 8-bit copy
  int NB, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
  int ipad, opad, rpad;
  int M, Ktot, relu, out_ld, res_ld, split_imgs;
  int cin_b;      // bytes per input pixel  (Cin  * element size)
  int krow_b;     // bytes per weight row   (Ktot * element size); K-steps of 128 bytes: krow_b >> 7, of 64 bytes: krow_b >> 6
  int out_dt, res_dt;          // DT_* of the output / residual tensors
  int ntaps;  // KH*KW; for Cin >= 64 the K order is (128-byte channel chunk outer, tap inner) so the taps of a chunk
              // are consecutive K-steps and their overlapping input pixels are re-read while still L2-resident
  // byte offset of K-step kt's X slab relative to a row's (tap 0, channel 0) address; host-filled, read with s_load
  unsigned koff[80];
  unsigned koff32[160];  // same per 64-byte K-step (conv_pp32_kernel)
  int m_begin;            // first output row handled by this launch (hybrid 256^2 + 128^2 launches)
  int n_tall;             // conv_big_pp_kernel: row tiles that are 288 rows tall instead of 256 (the ragged rounds), 0 = none
  int ksplit, kt_per;     // split-K (small problems): K-steps [split*kt_per, ...) per workgroup, fp32 partial slabs
  float *partial;         // [ksplit][M - m_begin][Cout]
  // weight groups along M (the refiner's two heads in ONE launch at small N, conv_igemm_kernel only): rows
  // [g*grp_rows, (g+1)*grp_rows) use weights w + g*grp_w_bytes and bias + g*Cout; grp_rows % 128 == 0, 0 = off.
  // in_shared / res_shared: the input / residual tensor has only the first group's rows and is read by every group.
  int grp_rows, in_shared, res_shared;
  unsigned grp_w_bytes;
  unsigned long long *clk;  // optional clock probe: per block {cycles0, realtime0, cycles1, realtime1}
  // positional table [OH*OW][Cout] (element type out_dt) added to the ROUNDED output (exactly what add_pos_embed_kernel
  // computes on the stored tensor); only conv_splitk_reduce_kernel implements it (Track: one launch less)
  const unsigned char *post;
};

// Epilogue shared by every conv schedule.
// Weight rows are PERMUTED on the host inside each block of 16*NI output channels (permute_rows): MFMA tile ni, row
// i = 4g + j (g = lane>>4, j = accumulator register) computes channel
//     NI == 4:  32*(j>>1) + 8*g + 4*(j&1) + ni        NI == 2:  8*g + 2*j + ni
// so a lane's accumulators hold 8 CONSECUTIVE channels per store and the four lane groups of a store
// instruction cover 64 contiguous channels of one pixel (the natural D^T layout gives 4 channels per store and
// twice the store instructions; the 256x256 kernel spent 13 us of a 70 us workgroup in its store burst).
// All bias and residual loads are issued BEFORE the first store: on CDNA4 stores also count in vmcnt, so a load issued
// behind a store cannot be waited for without draining the store.
// DT = the kernel's operand type.  8-bit kernels (DT_FP8 / DT_I8) [r4]: acc (float, or int32 bits for DT_I8) * cscale[c] + bias[c]
// -- cscale = the weight row's scale; the per-INPUT-channel activation scales are folded into the weights before they are quantised
// (net_apply_q8) -- and the residual is ALWAYS f16 (the skip path of the 8-bit networks is never re-quantised).
// ODT = what is written (fp_nn.h):
//   2-byte type            p.out, as before;
//   DT_FP8 / DT_I8         p.out only, no scaling here: the consumer's per-channel scales are folded into this layer's cscale / bias
//                          on the host (legal because these layers have no residual and end in a ReLU);
//   DT_DUAL_FP8 / _I8      an f16 tensor at p.out (the residual stream) AND its 8-bit copy at p.out2 = value * oinv[c] (the next
//                          convolution's operand); both tensors have the same shape / border, so one element offset serves both.
//   DT_QS_FP8 / _I8        the 8-bit copy alone, value * oinv[c], at p.out (a layer WITH a residual whose f16 output nobody reads:
//                          the consumer's scales cannot be folded into the tables then)
// The epilogue covers channel tiles [NI0, NI0 + NI) of an accumulator array of NIT tiles (the stem: two 32-channel passes
// over its 4 tiles; the array is passed whole so that it stays in registers).
__device__ __forceinline__ int pack4_fp8(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(a), sat_fp8(b), 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(c), sat_fp8(d), w, true);
}
// unsigned 8-bit activations (round to nearest even, saturating to [0, 255]) stored with an offset of -128 (x ^ 0x80) so that the
// signed-integer MFMA can consume them; the offset's contribution, 128 * sum_k w, is folded into the consumer's bias on the host
__device__ __forceinline__ int pack4_u8(float a, float b, float c, float d) {
  unsigned w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(a), 0, 0u);
  w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(b), 1, w);
  w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(c), 2, w);
  w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(d), 3, w);
  return (int)(w ^ 0x80808080u);
}
// EABL: 1 = no stores, 2 = no residual loads (timing ablations / layers without residual), 4 = add ConvParams::post, 8 = pass 1 ends before
// the pixel groups begin (below)
template <int MI, int NI, int DT, int ODT, int EABL = 0, int NIT = NI, int NI0 = 0, class PixFn>
__device__ __forceinline__ void conv_epilogue_px(const ConvParams &p, f4 (&acc)[NIT][MI], int n_base, int lane, PixFn pix,
                                                 int bias_off = 0, int res_img_off = 0) {
  static_assert(NI == 4 || NI == 2, "wave covers 64 or 32 channels");
  constexpr int NS = NI / 2;  // 8-channel stores per pixel per lane
  constexpr int O16 = odt_16(ODT), OQ = odt_q(ODT);
  constexpr bool DUAL = odt_dual(ODT), SCALED = odt_dual(ODT) || odt_qs(ODT), RQ = odt_rq(ODT);
  constexpr int RDT = RQ ? DT_I8 : is_q8(DT) ? DT_F16 : DT;
  const int OHp = p.OH + 2 * p.opad, OWp = p.OW + 2 * p.opad;
  const int RHp = p.OH + 2 * p.rpad, RWp = p.OW + 2 * p.rpad;
  const int g = lane >> 4;
  const int nl = n_base + 8 * g;  // store k covers channels nl + 32*k .. +7
  constexpr int res_es = elem_bytes(RDT);
  // pass 1, in place: acc = acc [* dequantisation scale] + bias (8 channels of bias / scale live at a time)
#pragma unroll
  for (int k = 0; k < NS; k++) {
    float bv[8], sc[8];
    float4 b0 = *reinterpret_cast<const float4 *>(p.bias + bias_off + nl + 32 * k), b1 = *reinterpret_cast<const float4 *>(p.bias + bias_off + nl + 32 * k + 4);
    bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
    if constexpr (DT == DT_I8) {
      if (p.bias_img) {   // (wave-uniform) the bias comes per image, in pass 2
#pragma unroll
        for (int e = 0; e < 8; e++) bv[e] = 0.f;
      }
    }
    if constexpr (is_q8(DT)) {
      float4 s0 = *reinterpret_cast<const float4 *>(p.cscale + bias_off + nl + 32 * k), s1 = *reinterpret_cast<const float4 *>(p.cscale + bias_off + nl + 32 * k + 4);
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w; sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int jj = (NI == 4) ? 2 * k + (e >> 2) : (e >> 1);
      const int ni = (NI == 4) ? (e & 3) : (e & 1);
#pragma unroll
      for (int mi = 0; mi < MI; mi++) {
        // (__float_as_int takes the element BY VALUE: __builtin_bit_cast on a vector-element lvalue reads element 0 of the vector)
        if constexpr (DT == DT_I8) acc[NI0 + ni][mi][jj] = __builtin_fmaf((float)__float_as_int(acc[NI0 + ni][mi][jj]), sc[e], bv[e]);
        else if constexpr (DT == DT_FP8) acc[NI0 + ni][mi][jj] = __builtin_fmaf(acc[NI0 + ni][mi][jj], sc[e], bv[e]);
        else acc[NI0 + ni][mi][jj] += bv[e];
      }
    }
  }
  // EABL & 8 (conv_big_pp_kernel with its two tile heights): every accumulator is final here, so no bias value stays live into the pixel
  // groups.  Without it the compiler interleaves the bias pass with the groups' residual loads and, in the kernel that holds both bodies,
  // runs out of its 256 registers (16 spilled, 36 bytes of scratch); with it 241 and none.  Same operations, same values.
  if constexpr ((EABL & 8) != 0) {
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) asm volatile("" : "+v"(acc[NI0 + a][b]));
  }
  float oi[SCALED ? NS : 1][8];  // 1 / (scale of output channel c in the 8-bit copy)
  if constexpr (SCALED) {
#pragma unroll
    for (int k = 0; k < NS; k++) {
      float4 s0 = *reinterpret_cast<const float4 *>(p.oinv + nl + 32 * k), s1 = *reinterpret_cast<const float4 *>(p.oinv + nl + 32 * k + 4);
      oi[k][0] = s0.x; oi[k][1] = s0.y; oi[k][2] = s0.z; oi[k][3] = s0.w; oi[k][4] = s1.x; oi[k][5] = s1.y; oi[k][6] = s1.z; oi[k][7] = s1.w;
    }
  }
  float rs[RQ ? NS : 1][8];    // RQ: scale of channel c of the 8-bit residual tensor
  if constexpr (RQ) {
#pragma unroll
    for (int k = 0; k < NS; k++) {
      float4 s0 = *reinterpret_cast<const float4 *>(p.rscale + nl + 32 * k), s1 = *reinterpret_cast<const float4 *>(p.rscale + nl + 32 * k + 4);
      rs[k][0] = s0.x; rs[k][1] = s0.y; rs[k][2] = s0.z; rs[k][3] = s0.w; rs[k][4] = s1.x; rs[k][5] = s1.y; rs[k][6] = s1.z; rs[k][7] = s1.w;
    }
  }
  // pixels in groups of at most 8 fragments (4 with a positional table): a group's residual / table values stay in registers
  constexpr bool POST = (EABL & 4) != 0;
  static_assert(!POST || (O16 >= 0 && !DUAL), "the positional table is added to plain 2-byte outputs");
  // (8-bit kernels: groups of 4 -- their f16 residual values are twice the bytes of the operands and the FP8 instantiations sit at the register limit)
  constexpr int GB = (POST || is_q8(DT)) ? (MI > 4 ? 4 : MI) : (MI > 8 ? (MI + 1) / 2 : MI);
#pragma unroll
  for (int g0 = 0; g0 < MI; g0 += GB) {
  size_t oofs[GB];
  bool ok[GB];
  int bimg_row[DT == DT_I8 ? GB : 1];   // image of the fragment's pixel (per-image bias)
  i4 rv[NS][GB], pv[NS][POST ? GB : 1];
#pragma unroll
  for (int gi = 0; gi < GB; gi++) {
    const int mi = g0 + gi;
    if (mi >= MI) break;
    int img, oh, ow;
    ok[gi] = pix(mi, img, oh, ow);  // (img, oh, ow) must be a valid address even when !ok
    if constexpr (DT == DT_I8) bimg_row[gi] = img;
    if constexpr (POST) {
      const size_t tok = (size_t)oh * p.OW + ow;
#pragma unroll
      for (int k = 0; k < NS; k++) pv[k][gi] = *reinterpret_cast<const i4 *>(p.post + (tok * p.Cout + nl + 32 * k) * 2);
    }
    int choff = 0, oimg = img;
    if (p.split_imgs > 0 && img >= p.split_imgs) { oimg = img - p.split_imgs; choff = p.Cout; }
    oofs[gi] = (((size_t)oimg * OHp + oh + p.opad) * OWp + ow + p.opad) * p.out_ld + choff;
    if (p.res && !(EABL & 2)) {
      size_t rpix = ((size_t)(img - res_img_off) * RHp + oh + p.rpad) * RWp + ow + p.rpad;
#pragma unroll
      for (int k = 0; k < NS; k++)
        rv[k][gi] = ok[gi] ? load8_raw(p.res + (rpix * p.res_ld + nl + 32 * k) * res_es, RDT) : (i4){0, 0, 0, 0};
    }
  }
#pragma unroll
  for (int gi = 0; gi < GB; gi++) {
    const int mi = g0 + gi;
    if (mi >= MI) break;
    if (!ok[gi]) continue;
#pragma unroll
    for (int k = 0; k < NS; k++) {
      i4 ov = {0, 0, 0, 0};  // packed 2-byte output: 8 values
      i2 oq = {0, 0};        // packed 8-bit output: 8 bytes
      float bi[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (DT == DT_I8) {
        if (p.bias_img) {
          const float *bp = p.bias_img + (size_t)bimg_row[gi] * p.Cout + nl + 32 * k;
          const float4 b0 = *reinterpret_cast<const float4 *>(bp), b1 = *reinterpret_cast<const float4 *>(bp + 4);
          bi[0] = b0.x; bi[1] = b0.y; bi[2] = b0.z; bi[3] = b0.w; bi[4] = b1.x; bi[5] = b1.y; bi[6] = b1.z; bi[7] = b1.w;
        }
      }
#pragma unroll
      for (int e4 = 0; e4 < 8; e4 += 4) {
        float v4[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const int e = e4 + h;
          const int jj = (NI == 4) ? 2 * k + (e >> 2) : (e >> 1);
          const int ni = (NI == 4) ? (e & 3) : (e & 1);
          float v = acc[NI0 + ni][mi][jj];
          if constexpr (DT == DT_I8) v += bi[e];
          if (p.res && !(EABL & 2)) {
            if constexpr (RQ) v = __builtin_fmaf((float)((((unsigned)rv[k][gi][e >> 2] >> ((e & 3) * 8)) & 0xffu) ^ 0x80u), rs[k][e], v);
            else v += raw_elem<RDT>(rv[k][gi], e);
          }
          if (p.relu) v = fmaxf(v, 0.f);
          if constexpr (POST) v = (float)(typename ElemT<O16 < 0 ? DT_F16 : O16>::t)v + raw_elem<O16 < 0 ? DT_F16 : O16>(pv[k][gi], e);  // = add_pos_embed_kernel on the stored value
          v4[h] = v;
        }
        if constexpr (O16 >= 0) {
          typedef typename ElemT<O16 < 0 ? DT_F16 : O16>::t OE;
          typedef OE oe2 __attribute__((ext_vector_type(2)));
          const oe2 p0 = {(OE)v4[0], (OE)v4[1]}, p1 = {(OE)v4[2], (OE)v4[3]};
          ov[e4 >> 1] = __builtin_bit_cast(int, p0);
          ov[(e4 >> 1) + 1] = __builtin_bit_cast(int, p1);
        }
        if constexpr (OQ >= 0) {
          if constexpr (SCALED) {
#pragma unroll
            for (int h = 0; h < 4; h++) v4[h] *= oi[k][e4 + h];
          }
          if constexpr (OQ == DT_FP8) oq[e4 >> 2] = pack4_fp8(v4[0], v4[1], v4[2], v4[3]);
          else oq[e4 >> 2] = pack4_u8(v4[0], v4[1], v4[2], v4[3]);
        }
      }
      if (EABL & 1) { asm volatile("" ::"v"(ov)); asm volatile("" ::"v"(oq)); continue; }
      if constexpr (O16 >= 0) *reinterpret_cast<i4 *>(p.out + (oofs[gi] + nl + 32 * k) * 2) = ov;
      if constexpr (OQ >= 0) *reinterpret_cast<i2 *>((DUAL ? p.out2 : p.out) + (oofs[gi] + nl + 32 * k)) = oq;
    }
  }
  }
}

// the implicit-GEMM schedules: output row m = m_base + mi*16 + (lane&15) in (image, oh, ow) raster order
template <int MI, int NI, int DT, int ODT, int EABL = 0>
__device__ __forceinline__ void conv_epilogue(const ConvParams &p, f4 (&acc)[NI][MI], int m_base, int n_base, int lane) {
  const int ohw = p.OH * p.OW;
  const int grp = p.grp_rows ? m_base / p.grp_rows : 0;  // tile-uniform (grp_rows is a multiple of the tile height)
  conv_epilogue_px<MI, NI, DT, ODT, EABL>(p, acc, n_base, lane, [&](int mi, int &img, int &oh, int &ow) {
    int m = m_base + mi * 16 + (lane & 15);
    const bool ok = m < p.M;
    int mm = ok ? m : 0;
    img = mm / ohw;
    int rem = mm - img * ohw;
    oh = rem / p.OW;
    ow = rem - oh * p.OW;
    return ok;
  }, grp * p.Cout, p.res_shared ? grp * p.grp_rows : 0);
}

// [r3] The same epilogue with the stores staged through LDS.  conv_epilogue's store instruction covers 16 pixels x 64 bytes: 16 cache
// lines, half of each, and the vector memory path retires lines, not bytes (DESIGN.md section 4.5).  Here a wave writes its finished
// 2-byte outputs to a private LDS tile ([rows][NI*32 bytes], 16-byte chunk c of row r at c ^ (r & 7)) together with each row's
// output offset, and copies them out as whole NI*32-byte runs, 8 rows (NI = 4: 8 full lines) per instruction.  Values are
// identical to conv_epilogue's (same operations in the same order).  `tile`: wave-private, HM*16*(NI*32) + HM*64 bytes; the MI
// fragments go through it in groups of HM.  2-byte output types, no positional table.
template <int MI, int NI, int DT, int ODT, int HM>
__device__ __forceinline__ void conv_epilogue_lds(const ConvParams &p, f4 (&acc)[NI][MI], int m_base, int n_base, int lane, unsigned char *tile) {
  static_assert(NI == 4 && !is_q8(DT) && odt_q(ODT) < 0 && MI % HM == 0, "64-channel wave tiles, 2-byte operands and outputs");
  constexpr int RB = NI * 32;                 // bytes per pixel row of the tile (64 channels x 2 B)
  constexpr int res_es = elem_bytes(DT);
  const int OHp = p.OH + 2 * p.opad, OWp = p.OW + 2 * p.opad;
  const int RHp = p.OH + 2 * p.rpad, RWp = p.OW + 2 * p.rpad;
  const int g = lane >> 4, li = lane & 15;
  const int nl = n_base + 8 * g;
  const int ohw = p.OH * p.OW;
  unsigned *otab = reinterpret_cast<unsigned *>(tile + HM * 16 * RB);
  float bv[2][8];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float4 b0 = *reinterpret_cast<const float4 *>(p.bias + nl + 32 * k), b1 = *reinterpret_cast<const float4 *>(p.bias + nl + 32 * k + 4);
    bv[k][0] = b0.x; bv[k][1] = b0.y; bv[k][2] = b0.z; bv[k][3] = b0.w; bv[k][4] = b1.x; bv[k][5] = b1.y; bv[k][6] = b1.z; bv[k][7] = b1.w;
  }
#pragma unroll
  for (int h0 = 0; h0 < MI; h0 += HM) {
    // residual loads of the group first (stores count in vmcnt on CDNA4: nothing is stored before they are all issued)
    i4 rv[HM][2];
    bool ok[HM];
    unsigned oo[HM];
#pragma unroll
    for (int q = 0; q < HM; q++) {
      const int m = m_base + (h0 + q) * 16 + li;
      ok[q] = m < p.M;
      const int mm = ok[q] ? m : 0;
      const int img = mm / ohw, rem = mm - img * ohw;
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      int choff = 0, oimg = img;
      if (p.split_imgs > 0 && img >= p.split_imgs) { oimg = img - p.split_imgs; choff = p.Cout; }
      oo[q] = ok[q] ? (unsigned)((((size_t)oimg * OHp + oh + p.opad) * OWp + ow + p.opad) * p.out_ld + choff) : 0xFFFFFFFFu;
      if (p.res) {
        const size_t rpix = ((size_t)img * RHp + oh + p.rpad) * RWp + ow + p.rpad;
#pragma unroll
        for (int k = 0; k < 2; k++) rv[q][k] = ok[q] ? load8_raw(p.res + (rpix * p.res_ld + nl + 32 * k) * res_es, DT) : (i4){0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int q = 0; q < HM; q++) {
      const int mi = h0 + q, row = q * 16 + li;
      if (g == 0) otab[row] = oo[q];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        i4 ov = {0, 0, 0, 0};
#pragma unroll
        for (int e2 = 0; e2 < 8; e2 += 2) {
          float v2[2];
#pragma unroll
          for (int hh = 0; hh < 2; hh++) {
            const int e = e2 + hh, jj = 2 * k + (e >> 2), ni = e & 3;
            float v = acc[ni][mi][jj];
            v += bv[k][e];
            if (p.res) v += raw_elem<DT>(rv[q][k], e);
            if (p.relu) v = fmaxf(v, 0.f);
            v2[hh] = v;
          }
          typedef typename ElemT<ODT>::t OE;
          typedef OE oe2 __attribute__((ext_vector_type(2)));
          const oe2 pr = {(OE)v2[0], (OE)v2[1]};
          ov[e2 >> 1] = __builtin_bit_cast(int, pr);
        }
        const int c = k * 4 + g;
        *reinterpret_cast<i4 *>(tile + row * RB + ((c ^ (row & 7)) << 4)) = ov;
      }
    }
    // copy-out (same wave wrote the tile: program order suffices): lane -> (row = it*8 + lane/8, chunk = lane%8)
#pragma unroll
    for (int it = 0; it < HM * 2; it++) {
      const int row = it * 8 + (lane >> 3), c = lane & 7;
      const unsigned off = otab[row];
      const i4 v = *reinterpret_cast<const i4 *>(tile + row * RB + ((c ^ (row & 7)) << 4));
      if (off != 0xFFFFFFFFu) *reinterpret_cast<i4 *>(p.out + ((size_t)off + n_base + c * 8) * 2) = v;
    }
  }
}

// split-K partial slab (true channel order): per accumulator register j a lane owns NI consecutive channels
template <int MI, int NI>
__device__ __forceinline__ void conv_store_partial(const ConvParams &p, f4 (&acc)[NI][MI], int split, int m_base, int n_base, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < MI; mi++) {
    int m = m_base + mi * 16 + (lane & 15);
    if (m >= p.M) continue;
    float *dst = p.partial + ((size_t)split * (p.M - p.m_begin) + (m - p.m_begin)) * p.Cout + n_base;
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      if (NI == 4) {
        f4 v = {acc[0][mi][jj], acc[1][mi][jj], acc[2][mi][jj], acc[3][mi][jj]};
        *reinterpret_cast<f4 *>(dst + 32 * (jj >> 1) + 8 * g + 4 * (jj & 1)) = v;
      } else {
        float2 v = make_float2(acc[0][mi][jj], acc[1][mi][jj]);
        *reinterpret_cast<float2 *>(dst + 8 * g + 2 * jj) = v;
      }
    }
  }
}

// Activations carry a physical zero border, so the K loop has no bounds checks, no selects and no divergent
// branches: a tap's operand address is (wave-uniform tap/chunk offset in SGPRs) + (per-lane row offset fixed for the
// whole kernel), which is exactly the saddr + voffset form of global_load_lds.
template <int BN, int VAR, int DT, int ODT = DT>
__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BM = 128;
  constexpr int XB = BM * 128;  // bytes per X stage (128 rows x 64 halfs)
  constexpr int WB = BN * 128;
  constexpr int STAGE = XB + WB;
  constexpr int NREP = BN / 32;     // 16-channel tiles per wave (wave tile = 64 pixels x BN/2 channels)
  constexpr int WPIECES = BN / 32;  // 8-row pieces of the W tile per wave

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 1] = wall_clock64(); }
  const int n_tiles = p.Cout / BN;
  // XCD-aware tile order: hardware places workgroup b on XCD b%8 (speed-only assumption).  Remap so each XCD walks a
  // contiguous range of logical tiles: the n-tiles of one m-tile (same X rows) and neighbouring m-tiles (shared halo
  // rows) hit the same private L2.  Bijective for any grid size.
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int split = logical % p.ksplit;
  logical /= p.ksplit;
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int m0 = p.m_begin + mt * BM, n0 = nt * BN;
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;

  // ---- staging roles: piece = 8 rows x 128 B; lane -> row (lane>>3), slot (lane&7); source chunk is swizzled
  const int srow = lane >> 3;
  const int g = (lane & 7) ^ srow;  // source 16-B chunk within the 64-wide K step
  unsigned xoff[4];                 // byte offset of (row's input pixel at tap (0,0), chunk 0) + g*16
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int m = min(m0 + (wave * 4 + i) * 8 + srow, p.M - 1);  // rows past M re-read the last pixel (never stored)
    if (p.in_shared) m -= (m0 / p.grp_rows) * p.grp_rows;   // every weight group reads the first group's rows
    int img = m / ohw;
    int rem = m - img * ohw;
    int oh = rem / p.OW, ow = rem - oh * p.OW;
    int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
    xoff[i] = (unsigned)(((img * IHp + ih0) * IWp + iw0) * p.cin_b + g * 16);
  }
  unsigned woffv[WPIECES];
#pragma unroll
  for (int i = 0; i < WPIECES; i++) {
    int row = (wave * WPIECES + i) * 8 + srow;
    woffv[i] = (unsigned)((n0 + row) * p.krow_b + g * 16);
  }
  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w + (p.grp_rows ? (size_t)(m0 / p.grp_rows) * p.grp_w_bytes : 0);

  auto stage = [&](int kt, int buf) {
    unsigned char *xs = smem + buf * STAGE;
    unsigned char *ws = xs + XB;
    const unsigned char *xb = in_b + p.koff[kt];
    const unsigned char *wb = w_b + (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; i++)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(xb + xoff[i]),
                                       (__attribute__((address_space(3))) void *)(xs + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < WPIECES; i++)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wb + woffv[i]),
                                       (__attribute__((address_space(3))) void *)(ws + (wave * WPIECES + i) * 1024), 16, 0, 0);
  };

  f4 acc[NREP][4];
#pragma unroll
  for (int a = 0; a < NREP; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (bytes) inside a stage; slot = chunk ^ (row&7), row&7 == lane&7
  const int frow = lane & 15, fk = lane >> 4;
  int xfo[2], wfo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    int slot = (ks * 4 + fk) ^ (lane & 7);
    xfo[ks] = (wm * 64 + frow) * 128 + slot * 16;
    wfo[ks] = XB + (wn * (BN / 2) + frow) * 128 + slot * 16;
  }

  auto compute = [&](int buf) {
    const unsigned char *sb = smem + buf * STAGE;
    if (VAR & 2) {
      // all 16 fragment reads of the K-step are issued up front: only the first LDS round trip is exposed
      i4 xf[2][4], wf[2][NREP];
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
#pragma unroll
        for (int mi = 0; mi < 4; mi++) xf[ks][mi] = *reinterpret_cast<const i4 *>(sb + xfo[ks] + mi * 16 * 128);
#pragma unroll
        for (int ni = 0; ni < NREP; ni++) wf[ks][ni] = *reinterpret_cast<const i4 *>(sb + wfo[ks] + ni * 16 * 128);
      }
      if (VAR & 8) {  // ablation: no MFMAs, fragments kept live
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
#pragma unroll
          for (int mi = 0; mi < 4; mi++) asm volatile("" ::"v"(xf[ks][mi]));
#pragma unroll
          for (int ni = 0; ni < NREP; ni++) asm volatile("" ::"v"(wf[ks][ni]));
        }
        return;
      }
      if (VAR & 1) __builtin_amdgcn_s_setprio(1);
      mma_kstep<DT, NREP, 4>(acc, wf, xf);
      if (VAR & 1) __builtin_amdgcn_s_setprio(0);
      return;
    }
    if constexpr (!is_q8(DT)) {
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      i4 xf[4], wf[NREP];
#pragma unroll
      for (int mi = 0; mi < 4; mi++) xf[mi] = *reinterpret_cast<const i4 *>(sb + xfo[ks] + mi * 16 * 128);
#pragma unroll
      for (int ni = 0; ni < NREP; ni++) wf[ni] = *reinterpret_cast<const i4 *>(sb + wfo[ks] + ni * 16 * 128);
      if (VAR & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ni = 0; ni < NREP; ni++)
#pragma unroll
        for (int mi = 0; mi < 4; mi++)
          acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
      if (VAR & 1) __builtin_amdgcn_s_setprio(0);
    }
    }
  };

  const int k_begin = split * p.kt_per, k_end = min(p.krow_b >> 7, k_begin + p.kt_per);
  stage(k_begin, 0);
  __syncthreads();
  // steady state is branch-free (stage next tile, compute current tile, one barrier); the last tile is peeled
  int buf = 0;
  for (int kt = k_begin; kt < k_end - 1; kt++) {
    if (!(VAR & 4)) stage(kt + 1, buf ^ 1);  // VAR&4: ablation (stale LDS, timing only)
    compute(buf);
    __syncthreads();
    buf ^= 1;
  }
  compute(buf);

  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4 + 2] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 3] = wall_clock64(); }
  if (p.ksplit > 1) {  // split-K: raw fp32 partial slab, reduced (+ bias / residual / ReLU) by conv_splitk_reduce_kernel
    conv_store_partial<4, NREP>(p, acc, split, m0 + wm * 64, n0 + wn * (BN / 2), lane);
    return;
  }
  // ---- epilogue: lane owns channels cb..cb+3 (cb = 4*(lane>>4)) of pixel (lane&15) in each 16x16 tile
  conv_epilogue<4, NREP, DT, ODT>(p, acc, m0 + wm * 64, n0 + wn * (BN / 2), lane);
}

// -------------------------------------------------------------------------------------------------
// conv_smallm_kernel [r3]: SMALL problems (Track: 1-2 images, a handful of objects) where every other schedule is a latency
// chain.  At N = 1 a layer is a weight-streaming problem -- conv_512 is 1.9 GFLOP on 4.7 MB of weights, 400 output pixels -- and
// the split-K schedules paid for their parallelism with an fp32 slab round trip and a SECOND launch per layer (9 reduce launches
// = 47 us of a 335 us Track).  Here a workgroup owns 16*MI pixels x 64 channels and its four waves split the K-STEPS (wave w
// takes steps w, w+4, ...): operands go global -> registers directly (no LDS staging, no barriers in the loop; three steps in
// flight per wave), the four partial accumulators are summed through LDS in a fixed order (w0+w1+w2+w3) and wave 0 runs the usual
// epilogue (bias, residual, ReLU, channel-concat addressing, positional table).  One launch per layer, every tensor written once.
// Generic over the conv shapes of both networks (3x3 s1 / s2, the 4x4 space-to-depth stem, 1x1 Linear layers incl. the two weight
// groups of the refiner heads): addressing is the implicit-GEMM one (ConvParams::koff + a per-lane row offset).
// -------------------------------------------------------------------------------------------------
// DEEP: the layer has at least 8 * PF K-steps, i.e. every wave at least 2 * PF: the prologue loads are then UNCONDITIONAL, which
// is what lets the compiler prove how many loads are in flight at the head of the steady-state loop (s_waitcnt vmcnt(10 * (PF-1) + 1)
// instead of vmcnt(1): with conditional prologue loads the in-order counter has to assume the shortest path).
template <int MI, int NI, int DT, int ODT, bool POST, bool DEEP>  // NI = 4: 64 channels per workgroup (Cout % 128 == 0); NI = 2: 32 (the row permutation of Cout == 64 layers)
__global__ __launch_bounds__(256, 2) void conv_smallm_kernel(const ConvParams p) {
  static_assert(!is_q8(DT), "2-byte operand types");
  constexpr int PF = MI == 1 ? 4 : 3;         // K-steps in flight per wave (register budget: (2*NI + 2*MI) * 4 VGPRs per step)
  extern __shared__ __attribute__((aligned(16))) unsigned char red[];  // 3 * NI * MI KB (dynamic, like every kernel launched through FP_LAUNCH)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_tiles = p.Cout / (16 * NI);
  // XCD placement for a WEIGHT-bound layer: hardware puts workgroup b on XCD b % 8, every XCD has its own L2, and at this size
  // the weights (4.7 MB for conv_512) are the traffic.  All workgroups of one channel tile go to ONE XCD (or to 8 / n_tiles XCDs
  // when the layer has fewer than 8 channel tiles), so each L2 pulls its 1/8 of the weights once instead of every L2 pulling all
  // of them (the m-tile-major order of the big schedules would cost 8 x 4.7 MB of fabric traffic per layer here).
  int mt, nt;
  {
    const int b = blockIdx.x, xcd = b & 7, within = b >> 3;
    if (n_tiles >= 8) {              // n_tiles % 8 == 0 (checked by the launcher)
      const int per = n_tiles >> 3;
      nt = xcd + 8 * (within % per);
      mt = within / per;
    } else {                         // 1, 2 or 4 channel tiles: 8 / n_tiles XCDs share one
      const int share = 8 / n_tiles;
      nt = xcd / share;
      mt = within * share + (xcd % share);
    }
  }
  if (mt * (16 * MI) >= p.M) return;   // (grid padded to a multiple of 8)
  const int m0 = mt * (16 * MI), n0 = nt * (16 * NI);
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;
  const int frow = lane & 15, fk = lane >> 4;
  const int grp = p.grp_rows ? m0 / p.grp_rows : 0;
  // per-lane operand addresses: X row of pixel fragment mi (rows past M re-read the last pixel, never stored), W row of tile ni
  const unsigned char *xrow[MI];
#pragma unroll
  for (int mi = 0; mi < MI; mi++) {
    int m = min(m0 + mi * 16 + frow, p.M - 1);
    if (p.in_shared) m -= grp * p.grp_rows;
    const int img = m / ohw, rem = m - img * ohw;
    const int oh = rem / p.OW, ow = rem - oh * p.OW;
    const int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
    xrow[mi] = p.in + ((size_t)(img * IHp + ih0) * IWp + iw0) * p.cin_b + fk * 16;
  }
  // weights in fragment order (fragment_order): one wave instruction = 1 KB of consecutive bytes = 8 whole cache lines
  const unsigned char *wrow = p.wfrag + (p.grp_rows ? (size_t)grp * p.grp_w_bytes : 0) + (size_t)(n0 >> 4) * ((size_t)16 * p.krow_b) + lane * 16;
  const size_t wtile = (size_t)16 * p.krow_b;

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int KT = p.krow_b >> 7;
  const int n_my = (KT - wave + 3) >> 2;      // steps wave, wave+4, ...
  i4 wf[PF][2][NI], xf[PF][2][MI];
  auto load = [&](i4 (&w)[2][NI], i4 (&x)[2][MI], int kt) {
    const unsigned ko = p.koff[kt];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
#pragma unroll
      for (int ni = 0; ni < NI; ni++) w[ks][ni] = *reinterpret_cast<const i4 *>(wrow + ni * wtile + (size_t)kt * 2048 + ks * 1024);
#pragma unroll
      for (int mi = 0; mi < MI; mi++) x[ks][mi] = *reinterpret_cast<const i4 *>(xrow[mi] + ko + ks * 64);
    }
  };
#pragma unroll
  for (int s = 0; s < PF; s++)
    if (DEEP || s < n_my) load(wf[s], xf[s], wave + 4 * s);
  // steady state WITHOUT conditions (every step has a successor PF steps ahead): the compiler's vmcnt bookkeeping stays exact, so
  // PF - 1 steps of loads really are in flight under each step's MFMAs (with the conditions inside, every step waited for
  // vmcnt(0): 21 us per conv_512 launch instead of the ~6 the L1 rate allows)
  int i = 0;
  for (; i + 2 * PF <= n_my; i += PF) {
#pragma unroll
    for (int s = 0; s < PF; s++) {
      // (scheduling fences: hipcc otherwise gathers the loads of all slots at the end of the iteration, and the in-order vmcnt
      // at the loop head then has to wait for nearly all of them -- s_waitcnt vmcnt(1) instead of vmcnt(10 * (PF - 1)))
      __builtin_amdgcn_sched_barrier(0);
      mma_kstep<DT, NI, MI>(acc, wf[s], xf[s]);
      __builtin_amdgcn_sched_barrier(0);
      load(wf[s], xf[s], wave + 4 * (i + s + PF));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // tail: at most 2*PF - 1 steps
#pragma unroll
  for (int s = 0; s < PF; s++) {
    if (i + s < n_my) {
      mma_kstep<DT, NI, MI>(acc, wf[s], xf[s]);
      if (i + s + PF < n_my) load(wf[s], xf[s], wave + 4 * (i + s + PF));
    }
  }
#pragma unroll
  for (int s = 0; s < PF; s++)
    if (i + PF + s < n_my) mma_kstep<DT, NI, MI>(acc, wf[s], xf[s]);
  // ---- fixed-order reduction of the four partial sums: waves 1..3 publish, wave 0 adds them in order and stores
  if (wave > 0) {
    f4 *dst = reinterpret_cast<f4 *>(red + (wave - 1) * (NI * MI * 1024)) + lane;
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) dst[(a * MI + b) * 64] = acc[a][b];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; w++) {
    const f4 *src = reinterpret_cast<const f4 *>(red + w * (NI * MI * 1024)) + lane;
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) {
        const f4 v = src[(a * MI + b) * 64];
        // component-wise on purpose: a float4 add is legalised to v_pk_add_f32, which this library must not contain (DESIGN.md section 9)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[a][b][r] = acc[a][b][r] + v[r];
      }
  }
  conv_epilogue<MI, NI, DT, ODT, POST ? 4 : 0>(p, acc, m0, n0, lane);
}

// -------------------------------------------------------------------------------------------------
// conv_smallx_kernel [r3]: conv_smallm_kernel with BOTH operands in the shape the vector L1 likes (tools/bench_tcp.hip: the L1
// serves a wave's 16-byte loads four lanes at a time, one clock per distinct cache line in the four -- 64 clocks for a load in
// MFMA-operand shape, 18 for 1 KB of consecutive bytes or for 8 pixel rows of 128 bytes):
//   * weights: global -> registers from the fragment-order copy (fragment_order), 1 KB of consecutive bytes per instruction;
//   * input pixels: LDS-DMA into a ring PRIVATE to the wave (8 pixels x 128 bytes per instruction, the 16-byte chunks XOR-swizzled
//     by the pixel on the source side), fragments read back with ds_read_b128 -- no workgroup barrier, the wave waits for its own
//     DMA with the in-order vmcnt.
// Every vector-memory instruction in the loop is an asm statement and the waits are counted by hand: L = 2 MI + 2 NI instructions
// per K-step, PF steps in flight, step s is complete when at most (steps issued after s) * L are outstanding.  Same tiles, same
// K split over the four waves, same fixed-order reduction and epilogue as conv_smallm_kernel: results are bit-identical.
// -------------------------------------------------------------------------------------------------
template <int MI, int NI, int DT, int ODT, bool POST, int PFO = 0>
__global__ __launch_bounds__(256, 2) void conv_smallx_kernel(const ConvParams p) {
  // (every element type: operands travel as raw 16-byte pieces, a 128-byte K-step is 64 two-byte or 128 one-byte channels; mma_kstep
  // picks the MFMA.  FP8 layers: Track / a few objects in FP8 mode no longer fall back to the split-K schedules)
  constexpr int PF = PFO ? PFO : (MI == 1 ? 4 : 3);        // K-steps in flight per wave
  constexpr int L = 2 * MI + 2 * NI;         // vector-memory instructions per K-step
  constexpr int STAGE = MI * 2048, RING = PF * STAGE;
  static_assert((PF - 1) * L <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [4 waves][PF stages][MI][16 pixels][128 B], then 3 * NI * MI KB for the reduction
  unsigned char *red = smem + 4 * RING;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_tiles = p.Cout / (16 * NI);
  int mt, nt;  // XCD placement by channel tile, as in conv_smallm_kernel
  {
    const int b = blockIdx.x, xcd = b & 7, within = b >> 3;
    if (n_tiles >= 8) {
      const int per = n_tiles >> 3;
      nt = xcd + 8 * (within % per);
      mt = within / per;
    } else {
      const int share = 8 / n_tiles;
      nt = xcd / share;
      mt = within * share + (xcd % share);
    }
  }
  if (mt * (16 * MI) >= p.M) return;
  const int m0 = mt * (16 * MI), n0 = nt * (16 * NI);
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;
  const int grp = p.grp_rows ? m0 / p.grp_rows : 0;
  // DMA sources: instruction (mi, j) stages pixels j*8 .. j*8+7 of fragment mi, lane -> (pixel = lane >> 3, chunk = (lane & 7) ^ pixel)
  const unsigned char *xsrc[MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; mi++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      int m = min(m0 + mi * 16 + j * 8 + (lane >> 3), p.M - 1);   // rows past M re-read the last pixel, never stored
      if (p.in_shared) m -= grp * p.grp_rows;
      const int img = m / ohw, rem = m - img * ohw;
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      const int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
      xsrc[mi][j] = p.in + ((size_t)(img * IHp + ih0) * IWp + iw0) * p.cin_b + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
    }
  const unsigned char *wrow = p.wfrag + (p.grp_rows ? (size_t)grp * p.grp_w_bytes : 0) + (size_t)(n0 >> 4) * ((size_t)16 * p.krow_b) + lane * 16;
  const size_t wtile = (size_t)16 * p.krow_b;
  const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem + wave * RING;
  const int li = lane & 15, g = lane >> 4;
  const unsigned char *xrd = smem + wave * RING + li * 128;
  const int xsl[2] = {(g ^ (li & 7)) << 4, ((4 + g) ^ (li & 7)) << 4};

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int KT = p.krow_b >> 7;
  const int n_my = (KT - wave + 3) >> 2;      // steps wave, wave+4, ...
  i4 wf[PF][2][NI];
  auto issue = [&](const int slot, i4 (&w)[2][NI], int kt) {
    const unsigned ko = p.koff[kt];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
      for (int j = 0; j < 2; j++) glds16_asm(xsrc[mi][j] + ko, ring_lds + slot * STAGE + mi * 2048 + j * 1024);
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      const unsigned char *wp = wrow + ni * wtile + (size_t)kt * 2048;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(w[0][ni]) : "v"(wp) : "memory");
      asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(w[1][ni]) : "v"(wp) : "memory");
    }
  };
  auto wait_steps = [&](int later) {  // wave-uniform: the number of K-steps issued after the one about to be consumed
    if (later >= PF - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PF - 1) * L) : "memory");
    else if (later == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * L <= 63 ? 3 * L : 63) : "memory");
    else if (later == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  auto consume = [&](const int slot, i4 (&w)[2][NI]) {
    // (the weight registers are asm outputs: tie them to this point so that no MFMA is scheduled above the wait)
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
      for (int ni = 0; ni < NI; ni++) asm volatile("" : "+v"(w[ks][ni]));
    __builtin_amdgcn_sched_barrier(0);
    i4 x[2][MI];
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
      for (int mi = 0; mi < MI; mi++) x[ks][mi] = *reinterpret_cast<const i4 *>(xrd + slot * STAGE + mi * 2048 + xsl[ks]);
    mma_kstep<DT, NI, MI>(acc, w, x);
    __builtin_amdgcn_sched_barrier(0);
  };
  int issued = 0;
#pragma unroll
  for (int s = 0; s < PF; s++)
    if (s < n_my) { issue(s, wf[s], wave + 4 * s); issued++; }
  for (int base = 0; base < n_my; base += PF) {
#pragma unroll
    for (int s = 0; s < PF; s++) {
      const int step = base + s;
      if (step < n_my) {
        wait_steps(issued - step - 1);
        consume(s, wf[s]);
        if (issued < n_my) { issue(s, wf[s], wave + 4 * issued); issued++; }   // (issued == step + PF here)
      }
    }
  }
  // ---- fixed-order reduction of the four partial sums: waves 1..3 publish, wave 0 adds them in order and stores
  if (wave > 0) {
    f4 *dst = reinterpret_cast<f4 *>(red + (wave - 1) * (NI * MI * 1024)) + lane;
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) dst[(a * MI + b) * 64] = acc[a][b];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; w++) {
    const f4 *src = reinterpret_cast<const f4 *>(red + w * (NI * MI * 1024)) + lane;
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) {
        const f4 v = src[(a * MI + b) * 64];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if constexpr (DT == DT_I8) acc[a][b][r] = __int_as_float(__float_as_int(acc[a][b][r]) + __float_as_int(v[r]));   // int32 partial sums
          else acc[a][b][r] = acc[a][b][r] + v[r];   // (component-wise: no v_pk_add_f32, DESIGN.md section 9)
        }
      }
  }
  conv_epilogue<MI, NI, DT, ODT, POST ? 4 : 0>(p, acc, m0, n0, lane);
}

// -------------------------------------------------------------------------------------------------
// Ping-pong variant: 256 pixels x BN channels per workgroup, 8 waves = two groups of 4 (each group owns 128 pixel
// rows with the usual 2x2 arrangement of 64 x BN/2 wave tiles, the W tile is shared).  The groups run in strict
// anti-phase: while group 0 pulls its 16 operand fragments of K-step kt from LDS into registers and issues the LDS-DMA
// for K-step kt+2, group 1 issues the 32 MFMAs of K-step kt-1 from registers only, and vice versa.  Each SIMD hosts one
// wave of either group, so its matrix pipe always has a pure-MFMA wave to run.  Three LDS stages; loads stay in
// flight across the barriers (counted vmcnt, raw s_barrier); two barriers per K-step.
// -------------------------------------------------------------------------------------------------
template <int BN, int DT, int ODT = DT>
__global__ __launch_bounds__(512, 2) void conv_pp_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BM = 256;
  constexpr int XB = BM * 128;
  constexpr int WB = BN * 128;
  constexpr int STAGE = XB + WB;
  constexpr int NREP = BN / 32;
  constexpr int WPIECES = BN / 64;
  constexpr int G = 4 + WPIECES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;                 // 0 / 1: pixel rows [grp*128, +128)
  const int wq = wave & 3, wm = wq & 1, wn = wq >> 1;
  const int n_tiles = p.Cout / BN;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int m0 = p.m_begin + mt * BM, n0 = nt * BN;
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;

  const int srow = lane >> 3;
  const int g = (lane & 7) ^ srow;
  unsigned xoff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int m = min(m0 + (wave * 4 + i) * 8 + srow, p.M - 1);
    int img = m / ohw;
    int rem = m - img * ohw;
    int oh = rem / p.OW, ow = rem - oh * p.OW;
    int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
    xoff[i] = (unsigned)(((img * IHp + ih0) * IWp + iw0) * p.cin_b + g * 16);
  }
  unsigned woffv[WPIECES];
#pragma unroll
  for (int i = 0; i < WPIECES; i++) {
    int row = (wave * WPIECES + i) * 8 + srow;
    woffv[i] = (unsigned)((n0 + row) * p.krow_b + g * 16);
  }
  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

  // (ConvParams::wdeep: the 16 pieces of a 128-row x 128-byte stage in piece order -- this wave's two are one 2 KB run)
  const bool packed = BN == 128 && p.wdeep != nullptr;   // (wave-uniform: a scalar branch)
  const unsigned char *wpk = p.wdeep + ((size_t)nt * (p.krow_b >> 7) * 16 + wave * 2) * 1024 + lane * 16;
  auto stage = [&](int kt, int buf) {
    const unsigned xs = lds_base + buf * STAGE;
    const unsigned ws = xs + XB;
    const unsigned char *xb = in_b + p.koff[kt];
    const unsigned char *wb = w_b + (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; i++) glds16_asm(xb + xoff[i], xs + (wave * 4 + i) * 1024);
    if (packed) { glds16x2_asm(wpk + (size_t)kt * 16384, ws + wave * 2048); return; }
#pragma unroll
    for (int i = 0; i < WPIECES; i++) glds16_asm(wb + woffv[i], ws + (wave * WPIECES + i) * 1024);
  };

  f4 acc[NREP][4];
#pragma unroll
  for (int a = 0; a < NREP; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fk = lane >> 4;
  int xfo[2], wfo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    int slot = (ks * 4 + fk) ^ (lane & 7);
    xfo[ks] = (grp * 128 + wm * 64 + frow) * 128 + slot * 16;
    wfo[ks] = XB + (wn * (BN / 2) + frow) * 128 + slot * 16;
  }

  i4 xf[2][4], wf[2][NREP];
  auto ldfrags = [&](int buf) {
    const unsigned char *sb = smem + buf * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
#pragma unroll
      for (int mi = 0; mi < 4; mi++) xf[ks][mi] = *reinterpret_cast<const i4 *>(sb + xfo[ks] + mi * 16 * 128);
#pragma unroll
      for (int ni = 0; ni < NREP; ni++) wf[ks][ni] = *reinterpret_cast<const i4 *>(sb + wfo[ks] + ni * 16 * 128);
    }
  };
  auto mfmas = [&]() {
    __builtin_amdgcn_s_setprio(1);
    mma_kstep<DT, NREP, 4>(acc, wf, xf);
    __builtin_amdgcn_s_setprio(0);
  };
#define FP_PP_BARRIER()                  \
  do {                                   \
    __builtin_amdgcn_s_barrier();        \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)

  const int KT = p.krow_b >> 7;  // >= 8
  stage(0, 0);
  stage(1, 1);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");  // tile 0 landed (this wave's pieces)
  FP_PP_BARRIER();
  int rb = 0, wb3 = 2;
  if (grp == 0) {
    for (int kt = 0; kt < KT; kt++) {
      // even slot: LDS -> registers for K-step kt, prefetch K-step kt+2
      ldfrags(rb);
      if (kt + 2 < KT) stage(kt + 2, wb3);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      FP_PP_BARRIER();
      // odd slot: MFMAs from registers
      mfmas();
      if (kt + 2 < KT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");  // tile kt+1 landed, kt+2 in flight
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      FP_PP_BARRIER();
      rb = (rb == 2) ? 0 : rb + 1;
      wb3 = (wb3 == 2) ? 0 : wb3 + 1;
    }
  } else {
    for (int kt = 0; kt < KT; kt++) {
      // even slot: MFMAs of K-step kt-1
      if (kt > 0) mfmas();
      FP_PP_BARRIER();
      // odd slot: LDS -> registers for K-step kt, prefetch K-step kt+2
      ldfrags(rb);
      if (kt + 2 < KT) {
        stage(kt + 2, wb3);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      FP_PP_BARRIER();
      rb = (rb == 2) ? 0 : rb + 1;
      wb3 = (wb3 == 2) ? 0 : wb3 + 1;
    }
    mfmas();
  }
#undef FP_PP_BARRIER

  conv_epilogue<4, NREP, DT, ODT>(p, acc, m0 + grp * 128 + wm * 64, n0 + wn * (BN / 2), lane);
}

// -------------------------------------------------------------------------------------------------
// 256 x 256 tile.  Ablation of the 128 x 128 kernel (tools/bench_conv.py variants 17/21/25) shows its K-step is bound
// by the global -> LDS path, not by the matrix pipe: with the MFMAs removed a K-step still takes ~1360 cycles against
// ~1050 with the loads removed, i.e. the two co-resident workgroups pull 64 KB per K-step at ~47 B/clk/CU, the L2 ->
// CU ceiling.  A 256 x 256 tile moves the same 64 KB per K-step for TWICE the MFMA work, which puts the K-step back
// under the matrix pipe.  8 waves (2 along pixels x 4 along channels), wave tile 128 x 64 (32 accumulators), BK = 64,
// two 64-KB LDS stages, one workgroup per CU.  Needs Cout % 256 == 0.
// -------------------------------------------------------------------------------------------------
// Ping-pong schedule of the 256 x 256 tile (see the slot comment inside), as a device function of the pixel fragments per wave:
// MI = 8 is the 256-row tile, MI = 9 the 288-row tile of the ragged rounds (two ping-pong groups of 144 rows; the weight side -- BN,
// NI, wpack128, stage_w -- is the same, an LDS stage is 288 * 128 + 256 * 128 bytes).  m0 / nt: first output row / channel tile.
template <int MI, int ABL, int DT, int ODT, bool POST, bool LSTORE>
__device__ __forceinline__ void conv_big_pp_body(const ConvParams &p, unsigned char *smem, const int m0, const int nt) {
  constexpr int BM = MI * 32, BN = 256;
  constexpr int XB = BM * 128, WB = BN * 128, STAGE = XB + WB;
  constexpr int NI = 4;
  // the X tile is BM / 8 pieces of 8 rows x 128 bytes: every wave stages PLO of them, the first PREM waves one more (288 rows: 36
  // pieces, waves 0-3 five, waves 4-7 four).  The loop only ever waits with vmcnt(0), so the uneven counts need no re-counted waits.
  constexpr int NPX = BM / 8, PLO = NPX / 8, PREM = NPX % 8, PHI = PLO + (PREM ? 1 : 0);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;  // wm doubles as the ping-pong group: waves w and w+4 share a SIMD
  const int n0 = nt * BN;
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;

  const int srow = lane >> 3;
  const int g = (lane & 7) ^ srow;
  const int px0 = wave * PLO + min(wave, PREM);   // the wave's first X piece
  unsigned xoff[PHI], woffv[4];
#pragma unroll
  for (int i = 0; i < PHI; i++) {
    int m = min(m0 + (px0 + i) * 8 + srow, p.M - 1);
    int img = m / ohw;
    int rem = m - img * ohw;
    int oh = rem / p.OW, ow = rem - oh * p.OW;
    int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
    xoff[i] = (unsigned)(((img * IHp + ih0) * IWp + iw0) * p.cin_b + g * 16);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int row = (wave * 4 + i) * 8 + srow;
    woffv[i] = (unsigned)((n0 + row) * p.krow_b + g * 16);
  }
  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

  // the 8 (9) LDS-DMA instructions of a K-step are issued in two halves (X pieces in the wave's L0 slot, W pieces at the
  // head of its M0 slot) so the address path (64 B/clk/CU) sees them spread over three slots instead of bunched in two
  auto stage_x = [&](int kt, int buf) {
    const unsigned xs = lds_base + buf * STAGE;
    const unsigned char *xb = in_b + p.koff[kt];
#pragma unroll
    for (int i = 0; i < PHI; i++)
      if (i < PLO || wave < PREM) glds16_asm(xb + xoff[i], xs + (px0 + i) * 1024);   // (wave-uniform)
  };
  // (ConvParams::wpack128, pack_stage_w128) this wave's 4 KB of every K-step as one run: one address + one M0 per stage
  const bool packed = p.wpack128 != nullptr;   // (wave-uniform: a scalar branch)
  const unsigned char *wpk = p.wpack128 + ((size_t)nt * (p.krow_b >> 7) * 8 + wave) * 4096 + lane * 16;
  auto stage_w = [&](int kt, int buf) {
    const unsigned ws = lds_base + buf * STAGE + XB;
    if (packed) { glds16x4_asm(wpk + (size_t)kt * 32768, ws + wave * 4096); return; }
    const unsigned char *wb = w_b + (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; i++) glds16_asm(wb + woffv[i], ws + (wave * 4 + i) * 1024);
  };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fk = lane >> 4;
  int xfo[2], wfo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    int slot = (ks * 4 + fk) ^ (lane & 7);
    xfo[ks] = (wm * (MI * 16) + frow) * 128 + slot * 16;   // (MI * 16 is a multiple of 8: row & 7 == lane & 7 in both groups)
    wfo[ks] = XB + (wn * 64 + frow) * 128 + slot * 16;
  }

#define FP_BAR()                         \
  do {                                   \
    __builtin_amdgcn_s_barrier();        \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
#define FP_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define FP_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
  // Slots of ~32 MFMAs (16 for FP8, each twice as long): group 0 runs L0 M0 L1 M1 per K-step, group 1 the same one slot later,
  // so on every SIMD one wave issues MFMAs from registers while its partner refills fragments from LDS / issues the next
  // tile's LDS-DMA.  The slot sequence is the same for every element type (FP_PP_LOOP); what a half-slot reads and
  // multiplies differs:
  //   2-byte types: half h = the 32-wide k-step h over all MI pixel fragments (8 + 4 fragment reads, 32 MFMAs; the 288-row tile 9 + 4, 36);
  //   FP8: one 128-wide MFMA consumes the whole 128-byte row, so the halves split the PIXEL fragments instead: half 0 reads
  //        the 4 weight operands (kept for both halves) + pixel fragments 0..3, half 1 pixel fragments 4..7.
#define FP_PP_LOOP(LD0, LD1, MF0, MF1)                                   \
  do {                                                                   \
    const int KT = p.krow_b >> 7;                                        \
    stage_x(0, 0);                                                       \
    stage_w(0, 0);                                                       \
    FP_VM0();                                                            \
    FP_BAR();                                                            \
    if (p.clk && tid == 0) { p.clk[blockIdx.x * 4] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 1] = wall_clock64(); } \
    int buf = 0;                                                         \
    if (wm == 0) {                                                       \
      for (int kt = 0; kt < KT; kt++) {                                  \
        LD0(buf);                                                        \
        if (kt + 1 < KT && !(ABL & 1)) stage_x(kt + 1, buf ^ 1);         \
        FP_LGKM0(); FP_BAR();                                            \
        if (kt + 1 < KT && !(ABL & 1)) stage_w(kt + 1, buf ^ 1);         \
        MF0(); FP_BAR();                                                 \
        LD1(buf); FP_LGKM0(); FP_BAR();                                  \
        MF1(); FP_VM0(); FP_BAR();                                       \
        buf ^= 1;                                                        \
      }                                                                  \
      FP_BAR();                                                          \
    } else {                                                             \
      FP_BAR();                                                          \
      for (int kt = 0; kt < KT; kt++) {                                  \
        LD0(buf);                                                        \
        if (kt + 1 < KT && !(ABL & 1)) stage_x(kt + 1, buf ^ 1);         \
        FP_LGKM0(); FP_BAR();                                            \
        if (kt + 1 < KT && !(ABL & 1)) stage_w(kt + 1, buf ^ 1);         \
        MF0(); FP_BAR();                                                 \
        LD1(buf); FP_LGKM0(); FP_VM0(); FP_BAR();                        \
        MF1(); FP_BAR();                                                 \
        buf ^= 1;                                                        \
      }                                                                  \
    }                                                                    \
  } while (0)

  if constexpr (is_q8(DT)) {
    i8 xv[MI / 2], wv[NI];
    auto ld0 = [&](int buf) {
      const unsigned char *sb = smem + buf * STAGE;
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
        wv[ni] = __builtin_shufflevector(*reinterpret_cast<const i4 *>(sb + wfo[0] + ni * 16 * 128),
                                         *reinterpret_cast<const i4 *>(sb + wfo[1] + ni * 16 * 128), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int j = 0; j < MI / 2; j++)
        xv[j] = __builtin_shufflevector(*reinterpret_cast<const i4 *>(sb + xfo[0] + j * 16 * 128),
                                        *reinterpret_cast<const i4 *>(sb + xfo[1] + j * 16 * 128), 0, 1, 2, 3, 4, 5, 6, 7);
    };
    auto ld1 = [&](int buf) {
      const unsigned char *sb = smem + buf * STAGE;
#pragma unroll
      for (int j = 0; j < MI / 2; j++)
        xv[j] = __builtin_shufflevector(*reinterpret_cast<const i4 *>(sb + xfo[0] + (MI / 2 + j) * 16 * 128),
                                        *reinterpret_cast<const i4 *>(sb + xfo[1] + (MI / 2 + j) * 16 * 128), 0, 1, 2, 3, 4, 5, 6, 7);
    };
    auto mf0 = [&]() {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
#pragma unroll
        for (int j = 0; j < MI / 2; j++) acc[ni][j] = mfma8<DT>(wv[ni], xv[j], acc[ni][j]);
      __builtin_amdgcn_s_setprio(0);
    };
    auto mf1 = [&]() {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
#pragma unroll
        for (int j = 0; j < MI / 2; j++) acc[ni][MI / 2 + j] = mfma8<DT>(wv[ni], xv[j], acc[ni][MI / 2 + j]);
      __builtin_amdgcn_s_setprio(0);
    };
    FP_PP_LOOP(ld0, ld1, mf0, mf1);
  } else {
    i4 xf[MI], wf[NI];
    auto ldk = [&](int buf, int ks) {
      const unsigned char *sb = smem + buf * STAGE;
#pragma unroll
      for (int mi = 0; mi < MI; mi++) xf[mi] = *reinterpret_cast<const i4 *>(sb + xfo[ks] + mi * 16 * 128);
#pragma unroll
      for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(sb + wfo[ks] + ni * 16 * 128);
    };
    auto ld0 = [&](int buf) { ldk(buf, 0); };
    auto ld1 = [&](int buf) { ldk(buf, 1); };
    auto mf = [&]() {
      if (ABL & 2) {  // ablation: keep fragments live, no MFMAs
#pragma unroll
        for (int mi = 0; mi < MI; mi++) asm volatile("" ::"v"(xf[mi]));
#pragma unroll
        for (int ni = 0; ni < NI; ni++) asm volatile("" ::"v"(wf[ni]));
        return;
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
          acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
      __builtin_amdgcn_s_setprio(0);
    };
    FP_PP_LOOP(ld0, ld1, mf, mf);
  }
#undef FP_PP_LOOP
#undef FP_BAR
#undef FP_LGKM0
#undef FP_VM0
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4 + 2] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 3] = wall_clock64(); }

  if (ABL & 4) {  // ablation: no epilogue (keep the accumulators live)
#pragma unroll
    for (int a = 0; a < NI; a++)
#pragma unroll
      for (int b = 0; b < MI; b++) asm volatile("" ::"v"(acc[a][b]));
    return;
  }
  if constexpr (LSTORE && MI == 8 && ABL == 0 && !POST && !is_q8(DT) && odt_q(ODT) < 0) {
    __syncthreads();   // both ping-pong groups are done with the ring: 8 x (8 KB tile + 256 B offsets) of it become the staging area
    conv_epilogue_lds<MI, NI, DT, ODT, 4>(p, acc, m0 + wm * 128, n0 + wn * 64, lane, smem + wave * (4 * 16 * 128 + 4 * 64));
    return;
  }
  constexpr bool RAGGED = ABL == 0 && !POST && !LSTORE && !is_q8(DT) && odt_q(ODT) < 0;   // the kernel holds this body at both heights
  conv_epilogue<MI, NI, DT, ODT, ((ABL >> 3) & 3) | (POST ? 4 : 0) | (RAGGED ? 8 : 0)>(p, acc, m0 + wm * (MI * 16), n0 + wn * 64, lane);
}

// The launch: workgroup -> (row tile, channel tile).  `logical` hands each XCD a contiguous chunk of tiles (the two channel tiles of a
// row tile are neighbours on one XCD and share the X tile in its L2).
// Ragged rounds (ConvParams::n_tall > 0; plan_conv): the grid is whole rounds of the 256 CUs and n_tall of its row tiles are 288 rows
// tall instead of 256, so that the rounds cover [m_begin, M) without a left-over launch.  The hardware dispatches workgroups in
// blockIdx order, round-robin over the XCDs, so the first round is the workgroups with blockIdx.x >> 3 < 32: the tall row tiles are the
// FIRST t_x row tiles of each XCD's chunk (t_x = n_tall / 8, one more on the first n_tall % 8 XCDs; t_x * n_tiles <= 32), all in the
// first round -- in the last they would be its tail.  Row tiles stay in row order, each 32 rows further down per tall tile in front of
// it: an exact partition of [m_begin, m_begin + 256 * row tiles + 32 * n_tall), which reaches M; rows >= M are clamped on load and
// masked in the epilogue.  A wave-uniform branch picks the body.  The 8-bit, POST, LSTORE and ablation instantiations have no tall body.
template <int ABL, int DT, int ODT = DT, bool POST = false, bool LSTORE = false>  // LSTORE: epilogue stores staged through LDS (conv_epilogue_lds)
__global__ __launch_bounds__(512, 2) void conv_big_pp_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool RAGGED = ABL == 0 && !POST && !LSTORE && !is_q8(DT) && odt_q(ODT) < 0;
  const int n_tiles = p.Cout / 256;
  const int nblk = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
  const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  int m0 = p.m_begin + mt * 256;
  if constexpr (RAGGED) {
    if (p.n_tall > 0) {   // (nblk % 256 == 0 and 256 % n_tiles == 0: r == 0, an XCD's chunk is q / n_tiles whole row tiles)
      const int tq = p.n_tall >> 3, tr = p.n_tall & 7;
      const int t_x = tq + (xcd < tr ? 1 : 0);   // tall row tiles of this XCD
      const int lt = within / n_tiles;           // row tile within the XCD's chunk: mt == xcd * (q / n_tiles) + lt
      m0 += 32 * (xcd * tq + min(xcd, tr) + min(lt, t_x));
      if (lt < t_x) {
        conv_big_pp_body<9, ABL, DT, ODT, POST, LSTORE>(p, smem, m0, nt);
        return;
      }
    }
  }
  conv_big_pp_body<8, ABL, DT, ODT, POST, LSTORE>(p, smem, m0, nt);
}

// -------------------------------------------------------------------------------------------------
// conv_pp32_kernel<BM,BN>: the ping-pong schedule on 32-wide K-steps with a ring of FOUR LDS stages.
// Ablation of conv_big_pp_kernel (64-wide K-steps, 2 stages) shows it is bound by the latency of the global -> LDS
// path: with the MFMAs removed a K-step still takes ~2190 cycles (64 KB in flight per CU), against ~1970 with the loads
// removed.  Halving the K-step and doubling the ring keeps the same 128 KB of LDS but lets three K-steps (96 KB) be in
// flight, with ~5 slots between issue and first use instead of ~3.
//   tile BM x BN, 8 waves = (BM/128) x (BN/64), wave tile 128 px x 64 ch (32 accumulators); (256,256) and (512,128).
//   stage = [BM + BN rows][64 B]; a DMA piece is 16 rows x 64 B; slot = chunk ^ G[(row>>2)&3], G = {0,2,3,1}, is
//   conflict-free for the four 16-lane groups of ds_read_b128 with 64-byte rows (checked by enumeration).
// -------------------------------------------------------------------------------------------------
template <int BM, int BN, int DT, int ODT = DT>
__global__ __launch_bounds__(512, 2) void conv_pp32_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int WM = BM / 128, WN = BN / 64;
  static_assert(WM * WN == 8, "8 waves");
  constexpr int XP = BM / 16, WP = BN / 16, PER = (XP + WP) / 8;  // DMA pieces per stage / per wave
  constexpr int XB = XP * 1024, STAGE = (XP + WP) * 1024;
  constexpr int MI = 8, NI = 4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;  // waves w and w+4 share a SIMD: the two ping-pong groups
  const int wm = wave / WN, wn = wave - wm * WN;
  const int n_tiles = p.Cout / BN;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int m0 = mt * BM, n0 = nt * BN;
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;

  // DMA roles: piece = wave + 8*i; lane -> (row = lane>>2, slot = lane&3); source chunk = slot ^ G[(row>>2)&3]
  const int prow = lane >> 2;
  const int gsel = (prow >> 2) & 3;
  const int gch = (lane & 3) ^ ((0x78 >> (gsel * 2)) & 3);  // G = {0,2,3,1} packed two bits each = 0x78
  unsigned poff[PER];
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int piece = wave + 8 * i;
    if (piece < XP) {
      int m = min(m0 + piece * 16 + prow, p.M - 1);
      int img = m / ohw;
      int rem = m - img * ohw;
      int oh = rem / p.OW, ow = rem - oh * p.OW;
      int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
      poff[i] = (unsigned)(((img * IHp + ih0) * IWp + iw0) * p.cin_b + gch * 16);
    } else {
      int row = (piece - XP) * 16 + prow;
      poff[i] = (unsigned)((n0 + row) * p.krow_b + gch * 16);
    }
  }
  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

  auto stage = [&](int st, int buf) {
    const unsigned sb = lds_base + buf * STAGE;
    const unsigned char *xb = in_b + p.koff32[st];
    const unsigned char *wb = w_b + (size_t)st * 64;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int piece = wave + 8 * i;
      glds16_asm((piece < XP ? xb : wb) + poff[i], sb + piece * 1024);
    }
  };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  // fragment addresses: row-in-tile r, chunk kg = lane>>4, slot = kg ^ G[(r>>2)&3]; (r>>2)&3 == ((lane&15)>>2)
  const int fsel = (lane & 15) >> 2;
  const int fslot = (lane >> 4) ^ ((0x78 >> (fsel * 2)) & 3);
  const int xfo = (wm * 128 + (lane & 15)) * 64 + fslot * 16;
  const int wfo = XB + (wn * 64 + (lane & 15)) * 64 + fslot * 16;

  i4 xf[MI], wf[NI];
  auto ld = [&](int buf) {
    const unsigned char *sb = smem + buf * STAGE;
#pragma unroll
    for (int mi = 0; mi < MI; mi++) xf[mi] = *reinterpret_cast<const i4 *>(sb + xfo + mi * 16 * 64);
#pragma unroll
    for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(sb + wfo + ni * 16 * 64);
  };
  auto mfmas = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ni = 0; ni < NI; ni++)
#pragma unroll
      for (int mi = 0; mi < MI; mi++)
        acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
    __builtin_amdgcn_s_setprio(0);
  };
#define FP_BAR()                         \
  do {                                   \
    __builtin_amdgcn_s_barrier();        \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
#define FP_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define FP_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
  // after the (optional) issue for step s+3, make sure this wave's pieces of step s+1 have landed
#define FP_WAIT_NEXT(s)                                  \
  do {                                                   \
    if ((s) + 3 < S) FP_VM(2 * PER);                     \
    else if ((s) + 2 < S) FP_VM(PER);                    \
    else FP_VM(0);                                       \
  } while (0)

  const int S = p.krow_b >> 6;  // 32-wide K-steps, >= 16 for every layer
  stage(0, 0);
  stage(1, 1);
  stage(2, 2);
  FP_VM(2 * PER);
  FP_BAR();
  int rb = 0, wb = 3;
  if (grp == 0) {
    for (int s = 0; s < S; s++) {
      ld(rb);
      if (s + 3 < S) stage(s + 3, wb);
      FP_LGKM0(); FP_BAR();
      mfmas();
      FP_WAIT_NEXT(s);
      FP_BAR();
      rb = (rb + 1) & 3; wb = (wb + 1) & 3;
    }
    FP_BAR();
  } else {
    FP_BAR();
    for (int s = 0; s < S; s++) {
      ld(rb);
      if (s + 3 < S) stage(s + 3, wb);
      FP_LGKM0();
      FP_WAIT_NEXT(s);
      FP_BAR();
      mfmas();
      FP_BAR();
      rb = (rb + 1) & 3; wb = (wb + 1) & 3;
    }
  }
#undef FP_BAR
#undef FP_LGKM0
#undef FP_VM
#undef FP_WAIT_NEXT
  conv_epilogue<MI, NI, DT, ODT>(p, acc, m0 + wm * 128, n0 + wn * 64, lane);
}

// -------------------------------------------------------------------------------------------------
// conv_halo_kernel<TW>: 3x3 / stride 1 convolution with the INPUT TILE + HALO resident in LDS.
// The implicit-GEMM schedules above re-fetch every input pixel once per tap (9x) through the global -> LDS path, which
// is what bounds them (~47 B/clk/CU).  Here a workgroup owns an 8-row x TW-column output tile of one image and stages
// the (8+2) x (TW+2) halo tile of a 64-channel chunk ONCE (the padded image rows are contiguous in memory, so the halo
// tile is one linear run of pixels); the 9 taps are just 9 shifted LDS windows.  Only the weights stream per K-step
// (8 KB per 32-wide step, 3-stage ring).  Global -> LDS traffic per flop is ~2x below the 256x256 tile's, small enough
// that TWO workgroups (4 waves, 160 accumulators each) share a CU: one's prologue / halo reload / epilogue store burst
// overlaps the other's MFMAs, which the one-workgroup-per-CU 256x256 tile cannot do.
//   M fragment = a 4x4 pixel block (lane&15 -> dy = >>2, dx = &3); wave (wm, wn) owns block-row wm (TW/4 blocks) x 64 ch.
//   halo LDS layout: pixel-major 128-byte rows, 16-byte slot = chunk ^ g, g = ((x>>1)&1) | ((y&3)<<1): conflict-free for
//   every tap shift (checked by enumeration); the swizzle is applied by the DMA on the SOURCE chunk.
// -------------------------------------------------------------------------------------------------
template <int TW, int ABL, int DT>  // ABL (timing ablations, wrong results): 1 no per-step barrier, 2 no MFMAs, 4 X fragments read once
__global__ __launch_bounds__(256, 2) void conv_halo_kernel(const ConvParams p) {
  static_assert(!is_q8(DT), "2-byte element types (64-channel chunks); the 8-bit sibling is conv_halo8_kernel");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TH = 8, HC = TW + 2, HPX = (TH + 2) * HC;
  constexpr int HPIECES = (HPX + 7) / 8, HALO_B = HPIECES * 1024;
  constexpr int HPER = (HPIECES + 3) / 4;  // halo DMA pieces per wave
  constexpr int WST = 128 * 64, NWST = 3;  // weight ring: 128 rows x 64 B per 32-wide K-step
  constexpr int MI = TW / 4, NI = 4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int n_tiles = p.Cout / 128;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int tiles_per_img = p.H / TH;
  const int img = mt / tiles_per_img, ty0 = (mt - img * tiles_per_img) * TH;
  const int n0 = nt * 128;
  const int IHp = p.H + 2;

  const unsigned char *in_b = p.in + ((size_t)(img * IHp + ty0) * HC) * p.cin_b;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  const unsigned w_lds = lds_base + HALO_B;

  // halo DMA: piece = wave + 4*i covers halo pixels piece*8 .. +7; lane -> (pixel = lane>>3, slot = lane&7)
  auto issue_halo = [&](int chunk) {
    const unsigned char *src = in_b + chunk * 128;
    int lane8;  // opaque copy of lane>>3: keeps the 14 per-lane offsets from being hoisted out of the chunk loop (VGPRs)
    asm volatile("v_lshrrev_b32 %0, 3, %1" : "=v"(lane8) : "v"(lane));
#pragma unroll
    for (int i = 0; i < HPER; i++) {
      const int piece = wave + 4 * i;
      if (piece < HPIECES) {
        int q = min(piece * 8 + lane8, HPX - 1);
        int hy = q / HC, hx = q - hy * HC;
        int g = ((hx >> 1) & 1) | ((hy & 3) << 1);
        unsigned off = (unsigned)(q * p.cin_b + (((lane & 7) ^ g) << 4));
        glds16_asm_x(src + off, lds_base + piece * 1024);
        __builtin_amdgcn_sched_barrier(0);  // one address at a time: 14 hoisted 64-bit addresses would spill accumulators
      }
    }
  };
  // weight DMA: piece = wave*2 + i (16 rows x 64 B); lane -> (row = lane>>2, slot = lane&3), source chunk = slot ^ G
  const int prow = lane >> 2;
  const int gch = (lane & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
  unsigned woff[2];
#pragma unroll
  for (int i = 0; i < 2; i++) woff[i] = (unsigned)((n0 + (wave * 2 + i) * 16 + prow) * p.krow_b + gch * 16);
  // (ConvParams::wpack, pack_stage_w) this wave's 2 KB of every K-step as one run: one address + one M0 per stage
  const bool packed = p.wpack != nullptr;   // (wave-uniform: a scalar branch)
  const unsigned char *wpk = p.wpack + ((size_t)nt * (p.krow_b >> 6) * 4 + wave) * 2048 + lane * 16;
  auto issue_w = [&](int st) {
    const unsigned dst = w_lds + (st % NWST) * WST;
    if (packed) { glds16x2_asm(wpk + (size_t)st * 8192, dst + wave * 2048); return; }
    const unsigned char *wb = w_b + (size_t)st * 64;
#pragma unroll
    for (int i = 0; i < 2; i++) glds16_asm(wb + woff[i], dst + (wave * 2 + i) * 1024);
  };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, dy = li >> 2, dx = li & 3, kg = lane >> 4;
  const int fslot = kg ^ ((0x78 >> ((li >> 2) * 2)) & 3);
  const int wfo = HALO_B + (wn * 64 + li) * 64 + fslot * 16;

  const int S = p.krow_b >> 6;   // 32-wide K-steps: 18 per 64-channel chunk (9 taps x 2)
  const int nch = p.cin_b >> 7;
  issue_halo(0);
  issue_w(0);
  issue_w(1);
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 1] = wall_clock64(); }
  int s = 0;
  for (int ch = 0; ch < nch; ch++) {
    for (int tap = 0; tap < 9; tap++) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int ty = wm * 4 + dy + ky, tx = dx + kx;
      const int g = ((tx >> 1) & 1) | ((ty & 3) << 1);
      const int pix_off = (ty * HC + tx) * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ks++, s++) {
        // W(s) (and, on a chunk's first step, the halo tile) landed; everyone finished reading step s-1
        if (((tap == 0 && ks == 0) && (!(ABL & 16) || s == 0)) || s == S - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        if (!(ABL & 1) || (tap == 0 && ks == 0)) __builtin_amdgcn_s_barrier();
        // s_barrier is IntrNoMem for the compiler: without this fence the fragment loads below may be placed ABOVE the
        // barrier on the steps that issue no DMA (the last two), reading weight pieces other waves have not landed yet
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < S) issue_w(s + 2);
        const unsigned char *xs = smem + pix_off + (((ks * 4 + kg) ^ g) << 4);
        const unsigned char *ws = smem + wfo + (s % NWST) * WST;
        if constexpr ((ABL & ~16) == 0) {  // (any ablation flag but 16, e.g. 32: the round-1 schedule -- two halves of 5 fragments; 16: the halo tile is never reloaded)
          // X fragments in four groups (3,2,3,2 of MI = 10) through two small register sets: the LDS reads of group q+1 are in
          // flight while the MFMAs of group q issue, so only the first group of a K-step waits for the LDS with the matrix pipe idle
          static_assert(MI == 10, "group split written for 10 pixel fragments");
          i4 wf[NI], xa[3], xb[2];
#pragma unroll
          for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(ws + ni * 16 * 64);
#pragma unroll
          for (int i = 0; i < 3; i++) xa[i] = *reinterpret_cast<const i4 *>(xs + i * 512);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 2; i++) xb[i] = *reinterpret_cast<const i4 *>(xs + (3 + i) * 512);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int i = 0; i < 3; i++) acc[ni][i] = mfma32<DT>(wf[ni], xa[i], acc[ni][i]);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 3; i++) xa[i] = *reinterpret_cast<const i4 *>(xs + (5 + i) * 512);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int i = 0; i < 2; i++) acc[ni][3 + i] = mfma32<DT>(wf[ni], xb[i], acc[ni][3 + i]);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 2; i++) xb[i] = *reinterpret_cast<const i4 *>(xs + (8 + i) * 512);
          __builtin_amdgcn_sched_barrier(0);
          if (tap == 8 && ks == 1 && ch + 1 < nch && !(ABL & 16)) {  // last reads of this chunk's halo tile are issued: refill it under the MFMAs
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            issue_halo(ch + 1);
          }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int i = 0; i < 3; i++) acc[ni][5 + i] = mfma32<DT>(wf[ni], xa[i], acc[ni][5 + i]);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int i = 0; i < 2; i++) acc[ni][8 + i] = mfma32<DT>(wf[ni], xb[i], acc[ni][8 + i]);
          __builtin_amdgcn_s_setprio(0);
        } else {
          // X fragments in two halves of MI/2 (register budget: 160 accumulators + 20 + 16 fragment registers); the
          // second half's LDS reads are issued behind the first half's MFMAs
          constexpr int HM = MI / 2;
          i4 xf[HM], wf[NI];
#pragma unroll
          for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(ws + ni * 16 * 64);
#pragma unroll
          for (int mi = 0; mi < HM; mi++) xf[mi] = *reinterpret_cast<const i4 *>(xs + mi * 512);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (!(ABL & 8)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int mi = 0; mi < HM; mi++) {
              if (ABL & 2) asm volatile("" ::"v"(wf[ni]), "v"(xf[mi]));
              else acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
            }
          if (!(ABL & 8)) __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mi = 0; mi < HM; mi++) xf[mi] = *reinterpret_cast<const i4 *>(xs + (HM + mi) * 512);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (tap == 8 && ks == 1 && ch + 1 < nch) {  // last read of this chunk's halo tile: refill it under the MFMAs
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            issue_halo(ch + 1);
          }
          if (!(ABL & 8)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int mi = 0; mi < HM; mi++) {
              if (ABL & 2) asm volatile("" ::"v"(wf[ni]), "v"(xf[mi]));
              else acc[ni][HM + mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][HM + mi]);
            }
          if (!(ABL & 8)) __builtin_amdgcn_s_setprio(0);
        }
      }
    }
  }
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4 + 2] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 3] = wall_clock64(); }
  conv_epilogue_px<MI, NI, DT, DT>(p, acc, n0 + wn * 64, lane, [&](int mi, int &oimg, int &oh, int &ow) {
    oimg = img;
    oh = ty0 + wm * 4 + dy;
    ow = mi * 4 + dx;
    return true;
  });
}

// -------------------------------------------------------------------------------------------------
// conv_halo8_kernel: the FP8 (e4m3) sibling of conv_halo_kernel<40>: 3x3 / stride 1 on 40x40 maps, input tile + halo of a
// 128-CHANNEL chunk (again 128 bytes per pixel, so the halo layout, its DMA and its swizzle are byte-identical) resident
// in LDS.  One K-step = one tap of the chunk = one v_mfma_f32_16x16x128_f8f6f4 per (pixel block, channel tile): 9
// steps per chunk of 40 MFMAs x 32 cycles per wave -- the same matrix-pipe time per step PAIR as the 2-byte kernel for
// twice the contraction length.
//   Weights: 128 rows x 128 B = 16 KB per step.  Two such stages next to the 53 KB halo would not let two workgroups
//   share a CU (2 x 85 KB > 160 KB), so the weight tile is single-buffered in LDS and double-buffered through
//   REGISTERS: every wave pulls its four 32-byte weight operands first, a second barrier frees the stage, the DMA for
//   the next tap is issued, and the 40 MFMAs (1280 cycles) run from registers while it lands.  LDS: 53 + 16 = 69 KB.
//   X operands are read two pixel blocks at a time under the MFMAs (160 accumulators + 32 + 16 operand registers).
//   Weight stage layout: 128-byte rows, 16-byte slot = chunk ^ (row & 7) (the implicit-GEMM kernels' swizzle).
// -------------------------------------------------------------------------------------------------
template <int DT, int ODT>   // DT = DT_FP8 / DT_I8; ODT = DT (a block's first conv) or DT_DUAL_* (its second: f16 stream + 8-bit copy)
__global__ __launch_bounds__(256, 2) void conv_halo8_kernel(const ConvParams p) {
  static_assert(is_q8(DT), "8-bit operand types (128-channel chunks); the 2-byte sibling is conv_halo_kernel");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TW = 40, TH = 8, HC = TW + 2, HPX = (TH + 2) * HC;
  constexpr int HPIECES = (HPX + 7) / 8, HALO_B = HPIECES * 1024;
  constexpr int HPER = (HPIECES + 3) / 4;  // halo DMA pieces per wave
  constexpr int MI = TW / 4, NI = 4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int n_tiles = p.Cout / 128;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int tiles_per_img = p.H / TH;
  const int img = mt / tiles_per_img, ty0 = (mt - img * tiles_per_img) * TH;
  const int n0 = nt * 128;
  const int IHp = p.H + 2;

  const unsigned char *in_b = p.in + ((size_t)(img * IHp + ty0) * HC) * p.cin_b;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  const unsigned w_lds = lds_base + HALO_B;

  // halo DMA: piece = wave + 4*i covers halo pixels piece*8 .. +7; lane -> (pixel = lane>>3, slot = lane&7)
  auto issue_halo = [&](int chunk) {
    const unsigned char *src = in_b + chunk * 128;
    int lane8;  // opaque copy of lane>>3: keeps the 14 per-lane offsets from being hoisted out of the chunk loop (VGPRs)
    asm volatile("v_lshrrev_b32 %0, 3, %1" : "=v"(lane8) : "v"(lane));
#pragma unroll
    for (int i = 0; i < HPER; i++) {
      const int piece = wave + 4 * i;
      if (piece < HPIECES) {
        int q = min(piece * 8 + lane8, HPX - 1);
        int hy = q / HC, hx = q - hy * HC;
        int g = ((hx >> 1) & 1) | ((hy & 3) << 1);
        unsigned off = (unsigned)(q * p.cin_b + (((lane & 7) ^ g) << 4));
        glds16_asm_x(src + off, lds_base + piece * 1024);
        __builtin_amdgcn_sched_barrier(0);  // one address at a time: hoisted 64-bit addresses would spill accumulators
      }
    }
  };
  // weight DMA: piece = wave*4 + i (8 rows x 128 B); lane -> (row = lane>>3, slot = lane&7), source chunk = slot ^ row
  const int srow = lane >> 3;
  unsigned woff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) woff[i] = (unsigned)((n0 + (wave * 4 + i) * 8 + srow) * p.krow_b + (((lane & 7) ^ srow) << 4));
  // (ConvParams::wpack, pack_stage_w128) this wave's 4 KB of every K-step as one run: one address + one M0 per stage
  const bool packed = p.wpack != nullptr;   // (wave-uniform: a scalar branch)
  const unsigned char *wpk = p.wpack + ((size_t)nt * (p.krow_b >> 7) * 4 + wave) * 4096 + lane * 16;
  auto issue_w = [&](int st) {
    if (packed) { glds16x4_asm(wpk + (size_t)st * 16384, w_lds + wave * 4096); return; }
    const unsigned char *wb = w_b + (size_t)st * 128;
#pragma unroll
    for (int i = 0; i < 4; i++) glds16_asm(wb + woff[i], w_lds + (wave * 4 + i) * 1024);
  };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, dy = li >> 2, dx = li & 3, kg = lane >> 4;
  // weight operand of channel tile ni: row wn*64 + ni*16 + li, chunks kg and 4 + kg
  const int wfo0 = HALO_B + (wn * 64 + li) * 128 + ((kg ^ (li & 7)) << 4);
  const int wfo1 = HALO_B + (wn * 64 + li) * 128 + (((4 + kg) ^ (li & 7)) << 4);

  const int S = p.krow_b >> 7;   // 9 taps per 128-channel chunk
  const int nch = p.cin_b >> 7;
  issue_halo(0);
  issue_w(0);
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 1] = wall_clock64(); }
  int s = 0;
  for (int ch = 0; ch < nch; ch++) {
    for (int tap = 0; tap < 9; tap++, s++) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int ty = wm * 4 + dy + ky, tx = dx + kx;
      const int g = ((tx >> 1) & 1) | ((ty & 3) << 1);
      const unsigned char *xs0 = smem + (ty * HC + tx) * 128 + ((kg ^ g) << 4);
      const unsigned char *xs1 = smem + (ty * HC + tx) * 128 + (((4 + kg) ^ g) << 4);
      // W(s) (and, on a chunk's first tap, the halo tile) landed
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      i8 wv[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
        wv[ni] = __builtin_shufflevector(*reinterpret_cast<const i4 *>(smem + wfo0 + ni * 16 * 128),
                                         *reinterpret_cast<const i4 *>(smem + wfo1 + ni * 16 * 128), 0, 1, 2, 3, 4, 5, 6, 7);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave holds W(s) in registers: the stage is free
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < S) issue_w(s + 1);
      // pixel fragments one at a time through two register sets: the reads of fragment m+1 are in flight while the four MFMAs of
      // fragment m issue (the round-1 schedule read two fragments, waited, issued eight MFMAs, five times per tap)
      auto read_x = [&](int m) {
        return __builtin_shufflevector(*reinterpret_cast<const i4 *>(xs0 + m * 512), *reinterpret_cast<const i4 *>(xs1 + m * 512), 0, 1, 2, 3, 4, 5, 6, 7);
      };
      i8 xv[2];
      xv[0] = read_x(0);
#pragma unroll
      for (int m = 0; m < MI; m++) {
        if (m + 1 < MI) {
          xv[(m + 1) & 1] = read_x(m + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (m == MI - 2 && tap == 8 && ch + 1 < nch) {  // the last read of this chunk's halo tile is issued: refill it under the MFMAs
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          issue_halo(ch + 1);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < NI; ni++) acc[ni][m] = mfma8<DT>(wv[ni], xv[m & 1], acc[ni][m]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if (p.clk && tid == 0) { p.clk[blockIdx.x * 4 + 2] = __builtin_readcyclecounter(); p.clk[blockIdx.x * 4 + 3] = wall_clock64(); }
  conv_epilogue_px<MI, NI, DT, ODT>(p, acc, n0 + wn * 64, lane, [&](int mi, int &oimg, int &oh, int &ow) {
    oimg = img;
    oh = ty0 + wm * 4 + dy;
    ow = mi * 4 + dx;
    return true;
  });
}

// -------------------------------------------------------------------------------------------------
// conv_stem_halo_kernel: the space-to-depth stem (4x4 taps, stride 1, 32 -> 64 channels, 84x84 padded input -> 80x80)
// with the same resident-halo scheme as conv_halo_kernel.  The implicit-GEMM stem re-fetched every 64-byte input pixel
// once per tap (16x) for a 128x64 tile and ran at ~365 TFLOP/s of padded work, bound by the global -> LDS path.
//   tile = 8 rows x 80 cols (640 px) x all 64 channels; 4 waves split the pixels (block-row x column half), 160
//   accumulators each; halo tile = (8+3) padded rows x 84 px x 64 B = one linear run of 59 KB staged once; 16 K-steps
//   (one tap each, 32 channels); weights 4 KB per step through a 3-stage ring; two workgroups per CU.
//   64-byte pixel rows: 16-byte slot = chunk ^ (y & 3); conflict-free because the pitch (84) is a multiple of 4.
// -------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256, 2) void conv_stem_halo_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TW = 80, TH = 8, HC = 84, HPX = (TH + 3) * HC;
  constexpr int HPIECES = (HPX + 15) / 16, HALO_B = HPIECES * 1024;
  constexpr int HPER = (HPIECES + 3) / 4;
  constexpr int WST = 64 * 64, NWST = 3;
  constexpr int MI = TW / 8, NI = 4, HM = MI / 2;  // 10 fragments (4x4 pixel blocks) per wave, in two halves
  constexpr int S = 16;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int brow = wave >> 1, chalf = wave & 1;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int tiles_per_img = p.H / TH;
  const int img = logical / tiles_per_img, ty0 = (logical - img * tiles_per_img) * TH;

  const unsigned char *in_b = p.in + ((size_t)(img * HC + ty0) * HC) * 64;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  const unsigned w_lds = lds_base + HALO_B;

  {  // halo DMA: piece = wave + 4*i covers 16 halo pixels; lane -> (pixel = lane>>2, slot = lane&3)
#pragma unroll
    for (int i = 0; i < HPER; i++) {
      const int piece = wave + 4 * i;
      if (piece < HPIECES) {
        int q = min(piece * 16 + (lane >> 2), HPX - 1);
        int hy = q / HC;
        unsigned off = (unsigned)(q * 64 + (((lane & 3) ^ (hy & 3)) << 4));
        glds16_asm(in_b + off, lds_base + piece * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  const int prow = lane >> 2;
  const int gch = (lane & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
  const unsigned woff = (unsigned)((wave * 16 + prow) * p.krow_b + gch * 16);
  auto issue_w = [&](int st) { glds16_asm(w_b + (size_t)st * 64 + woff, w_lds + (st % NWST) * WST + wave * 1024); };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, dy = li >> 2, dx = li & 3, kg = lane >> 4;
  const int fslot = kg ^ ((0x78 >> ((li >> 2) * 2)) & 3);
  const int wfo = HALO_B + li * 64 + fslot * 16;

  issue_w(0);
  issue_w(1);
#pragma unroll 1
  for (int s = 0; s < S; s++) {
    const int ky = s >> 2, kx = s & 3;
    const int ty = brow * 4 + dy + ky, tx = chalf * (TW / 2) + dx + kx;
    if (s == 0 || s == S - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (s + 2 < S) issue_w(s + 2);
    const unsigned char *xs = smem + (ty * HC + tx) * 64 + ((kg ^ (ty & 3)) << 4);
    const unsigned char *ws = smem + wfo + (s % NWST) * WST;
    i4 xf[HM], wf[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(ws + ni * 16 * 64);
#pragma unroll
    for (int mi = 0; mi < HM; mi++) xf[mi] = *reinterpret_cast<const i4 *>(xs + mi * 256);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ni = 0; ni < NI; ni++)
#pragma unroll
      for (int mi = 0; mi < HM; mi++)
        acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mi = 0; mi < HM; mi++) xf[mi] = *reinterpret_cast<const i4 *>(xs + (HM + mi) * 256);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ni = 0; ni < NI; ni++)
#pragma unroll
      for (int mi = 0; mi < HM; mi++)
        acc[ni][HM + mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][HM + mi]);
  }
  // Cout = 64: weight rows are permuted in 32-channel blocks (NI = 2 form), so the epilogue runs once per block
  auto pix = [&](int mi, int &oimg, int &oh, int &ow) {
    oimg = img;
    oh = ty0 + brow * 4 + dy;
    ow = chalf * (TW / 2) + mi * 4 + dx;
    return true;
  };
  // EABL = 2: this layer never has a residual (the dispatcher requires it), so the residual path is compiled out
  conv_epilogue_px<MI, 2, DT, DT, 2, 4, 0>(p, acc, 0, lane, pix);
  conv_epilogue_px<MI, 2, DT, DT, 2, 4, 2>(p, acc, 32, lane, pix);
}

// -------------------------------------------------------------------------------------------------
// conv_s2_halo_kernel: the 3x3 / stride-2 convolution 64 -> 128 channels on the 80x80 stem output (encodeA.1), again
// with the input tile resident in LDS.
//   tile = 4 output rows x 40 cols (160 px) x 128 channels; 4 waves = 2 (column halves) x 2 (64 channels), 80
//   accumulators each; 2 workgroups per CU.
//   Stride 2: a tap (ky,kx) reads input columns 2*ox + kx, i.e. one column-PARITY plane at consecutive positions --
//   exactly like a stride-1 tap.  The tile's 9 input rows are therefore staged one parity plane at a time (9 x 41 px x
//   128 B = 47 KB; every fetched 128-byte line is used whole): plane 0 serves the six taps with kx in {0,2} (12
//   32-channel K-steps), plane 1 the three taps with kx = 1 (6 K-steps).  Weights: 8 KB per step, 3-stage ring.
//   16-byte slot of an LDS pixel = chunk ^ (((row>>1)&3) | (((x>>1)&1)<<2)): conflict-free fragment reads.
// -------------------------------------------------------------------------------------------------
template <int DT, int ODT = DT>
__global__ __launch_bounds__(256, 2) void conv_s2_halo_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int IC = 82, HR = 9, PW = 41, HPX = HR * PW;  // 4 output rows need 9 input rows; 41 columns per parity plane
  constexpr int HPIECES = (HPX + 7) / 8, HALO_B = HPIECES * 1024;
  constexpr int HPER = (HPIECES + 3) / 4;
  constexpr int WST = 128 * 64, NWST = 3;
  constexpr int MI = 5, NI = 4, S = 18, SA = 12;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chalf = wave >> 1, wn = wave & 1;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int img = logical / 10, oy0 = (logical - img * 10) * 4;

  // input image: [82][82][64] halfs (border 1); the tile's first input row is 2*oy0 (padded coordinates)
  const unsigned char *in_b = p.in + ((size_t)(img * IC + 2 * oy0) * IC) * 128;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  const unsigned w_lds = lds_base + HALO_B;

  auto issue_halo = [&](int plane) {  // columns of one parity, all 64 channels
    int lane8;
    asm volatile("v_lshrrev_b32 %0, 3, %1" : "=v"(lane8) : "v"(lane));  // opaque: keeps the offsets out of long live ranges
#pragma unroll
    for (int i = 0; i < HPER; i++) {
      const int piece = wave + 4 * i;
      if (piece < HPIECES) {
        int q = min(piece * 8 + lane8, HPX - 1);
        int r = q / PW, xp = q - r * PW;
        int c = min(2 * xp + plane, IC - 1);
        int g = ((r >> 1) & 3) | (((xp >> 1) & 1) << 2);
        unsigned off = (unsigned)((r * IC + c) * 128 + (((lane & 7) ^ g) << 4));
        glds16_asm(in_b + off, __builtin_amdgcn_readfirstlane(lds_base + piece * 1024));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  const int prow = lane >> 2;
  const int gch = (lane & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
  unsigned woff[2];
#pragma unroll
  for (int i = 0; i < 2; i++) woff[i] = (unsigned)(((wave * 2 + i) * 16 + prow) * p.krow_b + gch * 16);
  // step -> (tap, 32-channel half): steps 0..11 walk the kx in {0,2} taps, 12..17 the kx = 1 taps
  auto step_tap = [&](int st, int &ky, int &kx) {
    if (st < SA) { const int t = st >> 1; ky = t >> 1; kx = (t & 1) * 2; }
    else { ky = (st - SA) >> 1; kx = 1; }
  };
  auto issue_w = [&](int st) {
    int ky, kx;
    step_tap(st, ky, kx);
    const unsigned char *wb = w_b + (size_t)((ky * 3 + kx) * 128 + (st & 1) * 64);
    const unsigned dst = __builtin_amdgcn_readfirstlane(w_lds + (st % NWST) * WST);
#pragma unroll
    for (int i = 0; i < 2; i++) glds16_asm(wb + woff[i], dst + (wave * 2 + i) * 1024);
  };

  f4 acc[NI][MI];
#pragma unroll
  for (int a = 0; a < NI; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, dy = li >> 2, dx = li & 3, kg = lane >> 4;
  const int fslot = kg ^ ((0x78 >> ((li >> 2) * 2)) & 3);
  const int wfo = HALO_B + (wn * 64 + li) * 64 + fslot * 16;

  issue_halo(0);
  issue_w(0);
  issue_w(1);
#pragma unroll 1
  for (int s = 0; s < S; s++) {
    int ky, kx;
    step_tap(s, ky, kx);
    if (s == 0 || s == SA || s == S - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (s + 2 < S) issue_w(s + 2);
    const int r = 2 * dy + ky;                         // input row inside the tile
    const int xp = chalf * 20 + dx + (kx >> 1);        // + mi*4 per fragment (keeps (xp>>1)&1 of the lane)
    const int g = ((r >> 1) & 3) | (((xp >> 1) & 1) << 2);
    const unsigned char *xs = smem + (r * PW + xp) * 128 + (((((s & 1) << 2) | kg) ^ g) << 4);
    const unsigned char *ws = smem + wfo + (s % NWST) * WST;
    i4 xf[MI], wf[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ni++) wf[ni] = *reinterpret_cast<const i4 *>(ws + ni * 16 * 64);
#pragma unroll
    for (int mi = 0; mi < MI; mi++) xf[mi] = *reinterpret_cast<const i4 *>(xs + mi * 512);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (s == SA - 1) {  // last read of plane 0: stage plane 1 under this step's MFMAs
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      issue_halo(1);
    }
#pragma unroll
    for (int ni = 0; ni < NI; ni++)
#pragma unroll
      for (int mi = 0; mi < MI; mi++)
        acc[ni][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni][mi]);
  }
  conv_epilogue_px<MI, NI, DT, ODT, 2>(p, acc, wn * 64, lane, [&](int mi, int &oimg, int &oh, int &ow) {  // 2: no residual in this layer
    oimg = img;
    oh = oy0 + dy;
    ow = chalf * 20 + mi * 4 + dx;
    return true;
  });
}

// -------------------------------------------------------------------------------------------------
// gemm_k32_kernel: the Linear layers (QKV, out_proj, FFN; K = 512, 100 800 rows at N = 252).  With only 8 64-wide
// K-steps a 256x256 tile that owns its CU spends as long in its prologue (two stages of loads with nothing to overlap)
// and in its 128 KB store burst as in the K loop (~720 TFLOP/s).  Here: 128 rows x 256 channels, 4 waves = 2 (64 rows)
// x 2 (128 channels), 128 accumulators, 32-wide K-steps of 24 KB through a 3-stage LDS-DMA ring (72 KB), TWO
// workgroups per CU so one's prologue / epilogue runs under the other's MFMAs.  LDS rows are 64 bytes; the 16-byte
// slot of (row, chunk) is chunk ^ f((row>>2)&3), f = {0,2,3,1} (conflict-free ds_read_b128 fragments).
// -------------------------------------------------------------------------------------------------
template <int ABL, int DT, bool LSTORE = false, bool WPACK = false>  // timing ablations: 1 = no MFMAs, 2 = no loads after the first stage, 4 = no stores; LSTORE: epilogue through LDS; WPACK: weights from the stage-order copy (ConvParams::wpack)
__global__ __launch_bounds__(256, 2) void gemm_k32_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BM = 128, BN = 256;
  constexpr int XST = BM * 64, WST = BN * 64, STAGE = XST + WST, NST = 3;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int n_tiles = p.Cout / BN;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int m0 = p.m_begin + mt * BM, n0 = nt * BN;
  const int S = p.krow_b >> 6;

  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

  // staging: a wave-instruction moves 16 rows x 64 B; lane -> (row = lane>>2, slot = lane&3), source chunk swizzled
  const int prow = lane >> 2;
  const int gch = (lane & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
  unsigned xoff[2], woff[4];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int m = min(m0 + (wave * 2 + i) * 16 + prow, p.M - 1);  // rows past M re-read the last row (never stored)
    xoff[i] = (unsigned)(m * p.krow_b + gch * 16);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) woff[i] = (unsigned)((n0 + (wave * 4 + i) * 16 + prow) * p.krow_b + gch * 16);
  // (WPACK) this wave's 4 KB of K-step 0; a K-step is 4 waves x 4 KB further
  const unsigned char *wpk = WPACK ? p.wpack + ((size_t)nt * S * 4 + wave) * 4096 + lane * 16 : nullptr;
  auto issue = [&](int st) {
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (st % NST) * STAGE);
    const unsigned char *xb = in_b + (size_t)st * 64, *wb = w_b + (size_t)st * 64;
#pragma unroll
    for (int i = 0; i < 2; i++) glds16_asm(xb + xoff[i], dst + (wave * 2 + i) * 1024);
    if constexpr (WPACK) {
      glds16x4_asm(wpk + (size_t)st * 16384, dst + XST + wave * 4096);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) glds16_asm(wb + woff[i], dst + XST + (wave * 4 + i) * 1024);
    }
  };

  f4 acc[2][4][4];  // [64-channel block][16-channel tile][16-row tile]
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[h][a][b] = (f4){0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, kg = lane >> 4;
  const int fslot = kg ^ ((0x78 >> ((li >> 2) * 2)) & 3);
  const int xfo = (wm * 64 + li) * 64 + fslot * 16;
  const int wfo = XST + (wn * 128 + li) * 64 + fslot * 16;

  issue(0);
  if (S > 1 && !(ABL & 2)) issue(1);
#pragma unroll 1
  for (int s = 0; s < S; s++) {
    if (s == S - 1 || (ABL & 2)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (s + 2 < S && !(ABL & 2)) issue(s + 2);
    const unsigned char *sb = smem + ((ABL & 2) ? 0 : (s % NST)) * STAGE;
    i4 xf[4], wf[8];
#pragma unroll
    for (int mi = 0; mi < 4; mi++) xf[mi] = *reinterpret_cast<const i4 *>(sb + xfo + mi * 1024);
#pragma unroll
    for (int ni = 0; ni < 8; ni++) wf[ni] = *reinterpret_cast<const i4 *>(sb + wfo + ni * 1024);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (ABL & 1) {
#pragma unroll
      for (int ni = 0; ni < 8; ni++) asm volatile("" ::"v"(wf[ni]));
#pragma unroll
      for (int mi = 0; mi < 4; mi++) asm volatile("" ::"v"(xf[mi]));
      continue;
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ni = 0; ni < 8; ni++)
#pragma unroll
      for (int mi = 0; mi < 4; mi++)
        acc[ni >> 2][ni & 3][mi] = mfma32<DT>(wf[ni], xf[mi], acc[ni >> 2][ni & 3][mi]);
    __builtin_amdgcn_s_setprio(0);
  }
  if constexpr (ABL == 0 && LSTORE) {
    // [r3] epilogue through LDS: the accumulator layout gives every store instruction 16 rows x 64 bytes -- 16 cache lines, half
    // of each -- and the vector memory path retires lines, not bytes (section 4.5 of DESIGN.md).  The wave's 64 x 128 tile is
    // written to its own 16 KB of the (now idle) ring as finished output rows and leaves as 4 rows x 256 contiguous bytes per
    // instruction.  Values are identical to conv_epilogue's (same operations in the same order).
    __syncthreads();                                   // every wave is done reading the ring
    unsigned char *tile = smem + wave * 16384;         // [64 rows][256 B], 16-byte chunk c stored at c ^ (row & 15)
    const int g = lane >> 4, li = lane & 15;
    const int mb = m0 + wm * 64, nb = n0 + wn * 128;
    float bv[2][2][8];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float4 b0 = *reinterpret_cast<const float4 *>(p.bias + nb + h * 64 + 8 * g + 32 * k), b1 = *reinterpret_cast<const float4 *>(p.bias + nb + h * 64 + 8 * g + 32 * k + 4);
        bv[h][k][0] = b0.x; bv[h][k][1] = b0.y; bv[h][k][2] = b0.z; bv[h][k][3] = b0.w; bv[h][k][4] = b1.x; bv[h][k][5] = b1.y; bv[h][k][6] = b1.z; bv[h][k][7] = b1.w;
      }
#pragma unroll
    for (int mi = 0; mi < 4; mi++) {
      const int row = mi * 16 + li, m = mb + row;
      const bool ok = m < p.M;
      i4 rv[2][2];
      if (p.res) {
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
          for (int k = 0; k < 2; k++)
            rv[h][k] = ok ? *reinterpret_cast<const i4 *>(p.res + ((size_t)m * p.res_ld + nb + h * 64 + 8 * g + 32 * k) * 2) : (i4){0, 0, 0, 0};
      }
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
          typename ElemT<DT>::v8 ov;
#pragma unroll
          for (int e = 0; e < 8; e++) {
            float v = acc[h][e & 3][mi][2 * k + (e >> 2)] + bv[h][k][e];
            if (p.res) v += raw_elem<DT>(rv[h][k], e);
            if (p.relu) v = fmaxf(v, 0.f);
            ov[e] = (typename ElemT<DT>::t)v;
          }
          const int c = h * 8 + k * 4 + g;
          *reinterpret_cast<typename ElemT<DT>::v8 *>(tile + row * 256 + ((c ^ (row & 15)) << 4)) = ov;
        }
    }
    // (same-wave LDS write -> read: program order suffices, no barrier)
#pragma unroll
    for (int it = 0; it < 16; it++) {
      const int row = it * 4 + (lane >> 4), c = lane & 15, m = mb + row;
      const i4 v = *reinterpret_cast<const i4 *>(tile + row * 256 + ((c ^ (row & 15)) << 4));
      if (m < p.M) *reinterpret_cast<i4 *>(p.out + ((size_t)m * p.out_ld + nb + c * 8) * 2) = v;
    }
    return;
  }
  conv_epilogue<4, 4, DT, DT, (ABL >> 2) & 1>(p, acc[0], m0 + wm * 64, n0 + wn * 128, lane);
  conv_epilogue<4, 4, DT, DT, (ABL >> 2) & 1>(p, acc[1], m0 + wm * 64, n0 + wn * 128 + 64, lane);
}

// -------------------------------------------------------------------------------------------------
// conv_deep_kernel: the rows the full 256x256 rounds of a long-K layer leave over (2.5 % of conv_512 at N = 252) run on
// an otherwise idle chip, one workgroup per CU walking all 72 K-steps: that chain is latency-bound, not bandwidth- or
// MFMA-bound.  So: small tiles (BM x 128, more CUs in use), the whole LDS as a deep LDS-DMA ring (6 x 24 KB stages at
// BM = 64: five K-steps in flight, counted vmcnt, one barrier per step) and the next step's fragments read under the
// current step's MFMAs (two register sets).  Same K order / accumulation order as every
// other schedule, so a row's value does not depend on which kernel computed it.
// -------------------------------------------------------------------------------------------------
template <int BM, int DT, int ODT = DT, bool POST = false>
__global__ __launch_bounds__(256, 2) void conv_deep_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BN = 128;
  constexpr int XB = BM * 128, WB = BN * 128, STAGE = XB + WB;
  constexpr int NST = BM == 64 ? 6 : 4, D = NST - 1;  // D stages in flight
  constexpr int XP = BM / 32, WP = 4, LPS = XP + WP;  // 1-KB pieces (8 rows x 128 B) per wave per stage
  constexpr int MI = BM / 32;                         // wave tile = BM/2 rows x 64 channels

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int n_tiles = p.Cout / BN;
  int logical;
  {
    const int nblk = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, within = b >> 3, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int split = logical % p.ksplit;  // split-K (small problems): this workgroup walks K-steps [K0, KT) into an fp32 partial slab
  logical /= p.ksplit;
  const int mt = logical / n_tiles, nt = logical - mt * n_tiles;
  const int m0 = p.m_begin + mt * BM, n0 = nt * BN;
  const int ohw = p.OH * p.OW;
  const int IHp = p.H + 2 * p.ipad, IWp = p.W + 2 * p.ipad;
  const int K0 = split * p.kt_per, KT = min(p.krow_b >> 7, K0 + p.kt_per);

  const int srow = lane >> 3;
  const int g = (lane & 7) ^ srow;
  unsigned xoff[XP], woff[WP];
#pragma unroll
  for (int i = 0; i < XP; i++) {
    int m = min(m0 + (wave * XP + i) * 8 + srow, p.M - 1);  // rows past M re-read the last pixel (never stored)
    if (p.in_shared) m -= (m0 / p.grp_rows) * p.grp_rows;   // weight groups along M: every group reads the first group's rows
    int img = m / ohw;
    int rem = m - img * ohw;
    int oh = rem / p.OW, ow = rem - oh * p.OW;
    int ih0 = oh * p.stride - p.pad + p.ipad, iw0 = ow * p.stride - p.pad + p.ipad;
    xoff[i] = (unsigned)(((img * IHp + ih0) * IWp + iw0) * p.cin_b + g * 16);
  }
#pragma unroll
  for (int i = 0; i < WP; i++) woff[i] = (unsigned)((n0 + (wave * WP + i) * 8 + srow) * p.krow_b + g * 16);
  const unsigned char *in_b = p.in;
  const unsigned char *w_b = p.w + (p.grp_rows ? (size_t)(m0 / p.grp_rows) * p.grp_w_bytes : 0);
  // (ConvParams::wdeep, pack_stage_w128) this wave's 4 KB of every K-step as one run: one address + one M0 per stage -- in this
  // kernel (8 MFMAs per wave and K-step at BM = 64) the LDS-DMA issue IS the K-step time
  const bool packed = p.wdeep != nullptr;   // (wave-uniform: a scalar branch)
  const unsigned char *wpk = p.wdeep + (p.grp_rows ? (size_t)(m0 / p.grp_rows) * p.grp_w_bytes : 0) + ((size_t)nt * (p.krow_b >> 7) * 4 + wave) * 4096 + lane * 16;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  auto issue = [&](int kt) {
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (kt % NST) * STAGE);
    const unsigned char *xb = in_b + p.koff[kt];
    const unsigned char *wb = w_b + (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < XP; i++) glds16_asm(xb + xoff[i], dst + (wave * XP + i) * 1024);
    if (packed) { glds16x4_asm(wpk + (size_t)kt * 16384, dst + XB + wave * 4096); return; }
#pragma unroll
    for (int i = 0; i < WP; i++) glds16_asm(wb + woff[i], dst + XB + (wave * WP + i) * 1024);
  };

  f4 acc[4][MI];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < MI; b++) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fk = lane >> 4;
  int xfo[2], wfo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    int slot = (ks * 4 + fk) ^ (lane & 7);
    xfo[ks] = (wm * (BM / 2) + frow) * 128 + slot * 16;
    wfo[ks] = XB + (wn * 64 + frow) * 128 + slot * 16;
  }

  // wait until stage `st` has landed: at most min(max_younger, KT-1-st) younger stages may still be in flight
  auto wait_stage = [&](int st, int max_younger) {
    const int younger = min(max_younger, KT - 1 - st);
    if (younger >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPS) : "memory");
    else if (younger == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPS) : "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 * LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  struct Frags { i4 x[2][MI], w[2][4]; };
  auto read_frags = [&](int kt, Frags &f) {
    const unsigned char *sb = smem + (kt % NST) * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
#pragma unroll
      for (int mi = 0; mi < MI; mi++) f.x[ks][mi] = *reinterpret_cast<const i4 *>(sb + xfo[ks] + mi * 16 * 128);
#pragma unroll
      for (int ni = 0; ni < 4; ni++) f.w[ks][ni] = *reinterpret_cast<const i4 *>(sb + wfo[ks] + ni * 16 * 128);
    }
  };
  // one K-step: the fragments of stage kt are already in `cur`; stage kt+1's are read into `nxt` under this step's MFMAs
  auto step = [&](int kt, const Frags &cur, Frags &nxt) {
    if (kt + 1 < KT) {
      wait_stage(kt + 1, D - 2);
      __builtin_amdgcn_s_barrier();  // every wave has finished reading stages <= kt (read one step ahead)
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if (kt + D < KT) issue(kt + D);  // reuses the buffer of stage kt-1
      read_frags(kt + 1, nxt);
    }
    mma_kstep<DT, 4, MI>(acc, cur.w, cur.x);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

#pragma unroll
  for (int s = 0; s < D; s++)
    if (K0 + s < KT) issue(K0 + s);
  Frags fa, fb;
  wait_stage(K0, D - 1);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read_frags(K0, fa);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int kt = K0;
#pragma unroll 1
  for (; kt + 1 < KT; kt += 2) {
    step(kt, fa, fb);
    step(kt + 1, fb, fa);
  }
  if (kt < KT) step(kt, fa, fb);
  if (p.ksplit > 1) {
    conv_store_partial<MI, 4>(p, acc, split, m0 + wm * (BM / 2), n0 + wn * 64, lane);
    return;
  }
  conv_epilogue<MI, 4, DT, ODT, POST ? 4 : 0>(p, acc, m0 + wm * (BM / 2), n0 + wn * 64, lane);
}

// split-K reduction + the conv epilogue: out = relu(sum_s partial[s] + bias + res); thread = (pixel, 8 channels).  2-byte networks
// only: the 8-bit layers never split K across workgroups (plan_conv).
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvParams p) {
  const int nq = p.Cout / 8;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int rows = p.M - p.m_begin;
  if (i >= (size_t)rows * nq) return;
  const int mr = (int)(i / nq), n = (int)(i - (size_t)mr * nq) * 8;
  const int m = p.m_begin + mr;
  float v[8];
  {
    const f4 a0 = *reinterpret_cast<const f4 *>(p.partial + (size_t)mr * p.Cout + n), a1 = *reinterpret_cast<const f4 *>(p.partial + (size_t)mr * p.Cout + n + 4);
#pragma unroll
    for (int e = 0; e < 4; e++) { v[e] = a0[e]; v[4 + e] = a1[e]; }
  }
  for (int sp = 1; sp < p.ksplit; sp++) {  // component-wise: no packed-f32 VALU ops in this library (DESIGN.md section 9)
    const float *src = p.partial + ((size_t)sp * rows + mr) * p.Cout + n;
    const f4 b0 = *reinterpret_cast<const f4 *>(src), b1 = *reinterpret_cast<const f4 *>(src + 4);
#pragma unroll
    for (int e = 0; e < 4; e++) { v[e] += b0[e]; v[4 + e] += b1[e]; }
  }
  const int grp = p.grp_rows ? m / p.grp_rows : 0;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    v[e] += p.bias[grp * p.Cout + n + e];
  }
  const int ohw = p.OH * p.OW;
  int img = m / ohw;
  int rem = m - img * ohw;
  int oh = rem / p.OW, ow = rem - oh * p.OW;
  const int OHp = p.OH + 2 * p.opad, OWp = p.OW + 2 * p.opad;
  const int RHp = p.OH + 2 * p.rpad, RWp = p.OW + 2 * p.rpad;
  if (p.res) {
    size_t rpix = ((size_t)(img - (p.res_shared ? grp * p.grp_rows : 0)) * RHp + oh + p.rpad) * RWp + ow + p.rpad;
    float r[8];
    decode8(load8_raw(p.res + (rpix * p.res_ld + n) * elem_bytes(p.res_dt), p.res_dt), p.res_dt, r);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] += r[e];
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    if (p.relu) v[e] = fmaxf(v[e], 0.f);
  }
  if (p.post) {  // (2-byte output types only)
    float pe[8];
    decode8(load8_raw(p.post + ((size_t)rem * p.Cout + n) * 2, p.out_dt), p.out_dt, pe);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (p.out_dt == DT_BF16 ? (float)(__bf16)v[e] : (float)(_Float16)v[e]) + pe[e];
  }
  int choff = 0, oimg = img;
  if (p.split_imgs > 0 && img >= p.split_imgs) { oimg = img - p.split_imgs; choff = p.Cout; }
  size_t opix = ((size_t)oimg * OHp + oh + p.opad) * OWp + ow + p.opad;
  store8(p.out + (opix * p.out_ld + choff + n) * elem_bytes(p.out_dt), p.out_dt, v);
}

