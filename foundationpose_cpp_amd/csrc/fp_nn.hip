// fp_nn.hip -- refine-net and score-net as hand-written CDNA4 (gfx950) kernels: fp16 storage, fp32 accumulate.
//
// Replaces the two opaque TensorRT fp16 engines of the reference (refiner_core_->SyncInfer / scorer_core_->SyncInfer,
// detection_6d_foundationpose/src/foundationpose.cpp:206-208,218-220,254-256; I/O blobs :78-83; shapes
// simple_tests/src/test_foundationpose.cpp:24-35).  The architecture is the published NVlabs FoundationPose one
// (SURVEY.md Appendix B [EXT]); the arithmetic oracle is oracle/nets_torch.py.
//
// Source layout [r4]: one translation unit (kernel templates must be visible where they are launched), four textual parts --
//   fp_nn_conv_kernels.inc       the convolution / Linear schedules        fp_nn_attention_kernels.inc   attention
//   fp_nn_small_kernels.inc      LayerNorm, token mean, small Linear ...   fp_nn_test_hooks.inc          fpt_* hooks (test build only)
// and this file: element types and helpers, weights (loading, layouts, 8-bit quantisation), scratch, the convolution / Linear schedule
// (plan_conv: pure host arithmetic, which kernels run a layer over which rows; run_conv: executes the plan's steps), the two forward passes.
//
// Kernels (DESIGN.md section 4.2 has the why and the measurements)
//   All convolution / Linear schedules are the same contraction D^T[channel][pixel] = W * X^T on
//   v_mfma_f32_16x16x32_f16 over NHWC activations that carry a physical zero border: operand tiles are staged with
//   global_load_lds_dwordx4 (16 B/lane LDS-DMA, no VGPR round trip), LDS stays lane-linear and the XOR swizzle is applied
//   to the per-lane SOURCE chunk and to the ds_read_b128 fragment address (conflict-free); im2col never touches HBM.
//   Weight rows are permuted on the host so a lane's accumulators are 8 consecutive channels: bias + residual + ReLU (+
//   the a|b channel concat as an addressing mode) fuse into an epilogue of 16-byte stores (conv_epilogue_px).
//     conv_halo_kernel<40>      3x3/s1 on 40x40 maps: the (8+2)x(40+2) input tile of a 64-channel chunk resident in LDS,
//                               the 9 taps are shifted LDS windows, only weights stream; 2 workgroups per CU.
//     conv_stem_halo_kernel     the 7x7/s2 stem as a 4x4/s1 conv over the space-to-depth input, same resident-halo scheme.
//     conv_big_pp_kernel        256x256 implicit-GEMM tile, 8 waves in two ping-pong groups, hand-counted s_waitcnt /
//                               raw s_barrier; conv_512, the stride-2 convs, Linear layers (full rounds of the 256 CUs).  Ragged
//                               rounds: some row tiles of the launch are 288 rows tall and absorb a small left-over (plan_conv).
//     conv_s2_halo_kernel       the 3x3/s2 conv 64->128 on the 80x80 stem output: the input tile staged one column-parity
//                               plane at a time (a stride-2 tap is a stride-1 window of one plane).  HBM-bound layer.
//     conv_pp32_kernel<512,128> 32-wide K-steps, 4-stage ring; the same stride-2 conv below ~30 hypotheses.
//     conv_igemm_kernel<BN>     128 x BN tile, 2 workgroups per CU, optional split-K (+ conv_splitk_reduce_kernel) and
//                               weight groups along M: left-over rows, small batches (Track).
//     conv_smallx_kernel [r3]   small problems (Track, a few objects): one launch per layer, K split over the waves of a workgroup;
//                               weights global -> registers from a copy in MFMA-fragment order, pixels through a per-wave LDS-DMA
//                               ring -- both in the one address shape the vector L1 serves at full rate (tools/bench_tcp.hip).
//     conv_pp / conv_smallm kernels: earlier schedules kept behind fpt_set_conv_variant / fpt_set_smallm for A/B.
//     Which of them runs where is plan_conv's decision alone; fpt_plan_conv asks it without a GPU (tests/test_conv_plan_cpu.py).
//   Weight layouts [r3]: besides the row-major [Cout][K] copy every layer carries the copies its schedules stream from -- fragment
//   order (conv_smallx), LDS-stage order for gemm_k32 / conv_halo / conv_halo8 / conv_big_pp / conv_deep + conv_pp (pack_stage_w,
//   pack_stage_w128): a wave's 2-4 LDS-DMA pieces of a stage are ONE contiguous run, so one address and one M0 serve them (the
//   instruction's immediate offset moves the global AND the LDS address) and every fetched cache line is used whole.
//   attention_kernel       softmax(QK^T/sqrt(d))V for 4 heads x 128, any sequence length (400 tokens per hypothesis, or
//                          the N hypotheses of the score-net's cross attention): S^T = K Q^T on MFMA so a softmax row is
//                          lane-local, P feeds the PV MFMA straight from registers (k-slot permutation shared with V^T).
//   layernorm / add_pos_embed / token_mean / small_linear / cast: bandwidth-trivial helpers.
#include "fp_nn.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <atomic>
#include <memory>
#include <thread>
#include <utility>

namespace fp {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i2 __attribute__((ext_vector_type(2)));
typedef int i4 __attribute__((ext_vector_type(4)));  // 16 raw bytes: one ds_read_b128 / one LDS-DMA lane
typedef int i8 __attribute__((ext_vector_type(8)));  // 32 raw bytes: one fp8 operand of v_mfma_f32_16x16x128_f8f6f4

static constexpr int EMBED = 512, HEADS = 4, HDIM = 128;

// ---- element types ------------------------------------------------------------------------------
// DT_F16 / DT_BF16: 2-byte storage, v_mfma_f32_16x16x32_{f16,bf16}; a 128-byte LDS row holds 64 elements = two MFMA k-steps.
// DT_FP8 (OCP e4m3, BASELINE configs[4]): 1-byte storage, v_mfma_f32_16x16x128_f8f6f4 (unscaled form: both block
//   scales are the literal 0, which selects the instruction without the scale prefix); a 128-byte row holds 128 elements = ONE
//   MFMA k-step whose 32-byte operand is the concatenation of the two 16-byte reads the 2-byte types feed to their two
//   MFMAs (lane group kg owns chunks kg and 4+kg of the row: W and X use the same assignment, so the contraction is
//   unchanged and the LDS swizzles / bank-conflict analysis carry over).  Quantisation: per-output-channel weight scale,
//   per-tensor activation scale (static, from fp_calibrate_fp8), folded into the epilogue.
template <int DT> struct ElemT { using t = _Float16; using v8 = h8; using v4 = h4; };
template <> struct ElemT<DT_BF16> { using t = __bf16; using v8 = b8; using v4 = b4; };

template <int DT>
__device__ __forceinline__ f4 mfma32(i4 a, i4 b, f4 c) {  // one 16x16x32 step on 2-byte operands
  static_assert(DT == DT_F16 || DT == DT_BF16, "32-wide MFMA steps exist for the 2-byte types only");
  if constexpr (DT == DT_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f4 mfma128_fp8(i8 a, i8 b, f4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0 /*A: fp8 e4m3*/, 0 /*B: fp8 e4m3*/, 0, 0, 0, 0);
}
// 8-bit operand types: DT_FP8 and DT_I8 share the byte geometry (a 128-byte LDS row = 128 channels = one 32-byte operand per lane
// group: chunks kg and 4+kg) and differ only in the matrix instruction.  DT_I8: the same 32 bytes feed TWO
// v_mfma_i32_16x16x64_i8 (16 cycles each = the 32 cycles of the one 128-wide FP8 instruction); the int32 accumulators live in
// the same f4 registers as raw bits (float 0.0 == int 0), the epilogue converts.
__host__ __device__ constexpr bool is_q8(int dt) { return dt == DT_FP8 || dt == DT_I8; }
template <int DT>
__device__ __forceinline__ f4 mfma8(i8 a, i8 b, f4 c) {
  static_assert(is_q8(DT), "8-bit operand types");
  if constexpr (DT == DT_FP8) return mfma128_fp8(a, b, c);
  else {
    i4 ci = __builtin_bit_cast(i4, c);
    ci = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_shufflevector(a, a, 0, 1, 2, 3), __builtin_shufflevector(b, b, 0, 1, 2, 3), ci, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_shufflevector(a, a, 4, 5, 6, 7), __builtin_shufflevector(b, b, 4, 5, 6, 7), ci, 0, 0, 0);
    return __builtin_bit_cast(f4, ci);
  }
}
// output-type codes (fp_nn.h): which tensors an epilogue writes
__host__ __device__ constexpr bool odt_dual(int odt) { return odt == DT_DUAL_FP8 || odt == DT_DUAL_I8; }
__host__ __device__ constexpr bool odt_qs(int odt) { return odt == DT_QS_FP8 || odt == DT_QS_I8 || odt == DT_QSR_I8; }
__host__ __device__ constexpr bool odt_rq(int odt) { return odt == DT_QSR_I8 || odt == DT_F16RQ_I8; }   // the residual operand is an 8-bit tensor
__host__ __device__ constexpr int odt_q(int odt) { return (odt == DT_DUAL_FP8 || odt == DT_QS_FP8) ? DT_FP8 : (odt == DT_DUAL_I8 || odt == DT_QS_I8 || odt == DT_QSR_I8) ? DT_I8 : is_q8(odt) ? odt : -1; }   // 8-bit type written, or -1
__host__ __device__ constexpr int odt_16(int odt) { return (odt_dual(odt) || odt == DT_F16RQ_I8) ? DT_F16 : (is_q8(odt) || odt_qs(odt)) ? -1 : odt; }   // 2-byte type written, or -1
// all MFMAs of one 128-byte K-step: w[ks][ni] / x[ks][mi] are the two 16-byte fragment reads of each row
template <int DT, int NI, int MI>
__device__ __forceinline__ void mma_kstep(f4 (&acc)[NI][MI], const i4 (&w)[2][NI], const i4 (&x)[2][MI]) {
  if constexpr (is_q8(DT)) {
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      const i8 wv = __builtin_shufflevector(w[0][ni], w[1][ni], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int mi = 0; mi < MI; mi++)
        acc[ni][mi] = mfma8<DT>(wv, __builtin_shufflevector(x[0][mi], x[1][mi], 0, 1, 2, 3, 4, 5, 6, 7), acc[ni][mi]);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
#pragma unroll
        for (int mi = 0; mi < MI; mi++) acc[ni][mi] = mfma32<DT>(w[ks][ni], x[ks][mi], acc[ni][mi]);
  }
}

// 8 consecutive channels <-> float; FP8 values are stored SCALED (real = stored * scale).  The raw form (16 bytes, or 8
// for FP8) is what stays in registers between the load and its use.
__device__ __forceinline__ i4 load8_raw(const unsigned char *ptr, int dt) {
  if (dt == DT_FP8 || dt == DT_I8) {
    const i2 v = *reinterpret_cast<const i2 *>(ptr);
    return (i4){v[0], v[1], 0, 0};
  }
  return *reinterpret_cast<const i4 *>(ptr);
}
__device__ __forceinline__ void decode8(i4 raw, int dt, float (&f)[8]) {
  if (dt == DT_FP8) {
    f[0] = __builtin_amdgcn_cvt_f32_fp8(raw[0], 0); f[1] = __builtin_amdgcn_cvt_f32_fp8(raw[0], 1);
    f[2] = __builtin_amdgcn_cvt_f32_fp8(raw[0], 2); f[3] = __builtin_amdgcn_cvt_f32_fp8(raw[0], 3);
    f[4] = __builtin_amdgcn_cvt_f32_fp8(raw[1], 0); f[5] = __builtin_amdgcn_cvt_f32_fp8(raw[1], 1);
    f[6] = __builtin_amdgcn_cvt_f32_fp8(raw[1], 2); f[7] = __builtin_amdgcn_cvt_f32_fp8(raw[1], 3);
  } else if (dt == DT_BF16) {
    const b8 v = __builtin_bit_cast(b8, raw);
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = (float)v[e];
  } else {
    const h8 v = __builtin_bit_cast(h8, raw);
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = (float)v[e];
  }
}
// element e (0..7) of a raw 8-channel group, as float (e is a constant once the caller's loop is unrolled)
template <int DT>
__device__ __forceinline__ float raw_elem(const i4 &raw, int e) {
  if constexpr (DT == DT_FP8) {
    const int w = raw[e >> 2];
    switch (e & 3) {
      case 0: return __builtin_amdgcn_cvt_f32_fp8(w, 0);
      case 1: return __builtin_amdgcn_cvt_f32_fp8(w, 1);
      case 2: return __builtin_amdgcn_cvt_f32_fp8(w, 2);
      default: return __builtin_amdgcn_cvt_f32_fp8(w, 3);
    }
  } else if constexpr (DT == DT_BF16) return (float)__builtin_bit_cast(b8, raw)[e];
  else return (float)__builtin_bit_cast(h8, raw)[e];
}
__device__ __forceinline__ float sat_fp8(float v) { return __builtin_amdgcn_fmed3f(v, -448.f, 448.f); }  // e4m3 finite range
__device__ __forceinline__ void store8(unsigned char *ptr, int dt, const float (&f)[8]) {
  if (dt == DT_FP8) {
    i2 v = {0, 0};
    v[0] = __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(f[0]), sat_fp8(f[1]), v[0], false);
    v[0] = __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(f[2]), sat_fp8(f[3]), v[0], true);
    v[1] = __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(f[4]), sat_fp8(f[5]), v[1], false);
    v[1] = __builtin_amdgcn_cvt_pk_fp8_f32(sat_fp8(f[6]), sat_fp8(f[7]), v[1], true);
    *reinterpret_cast<i2 *>(ptr) = v;
  } else if (dt == DT_BF16) {
    b8 v;
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (__bf16)f[e];
    *reinterpret_cast<b8 *>(ptr) = v;
  } else {
    h8 v;
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (_Float16)f[e];
    *reinterpret_cast<h8 *>(ptr) = v;
  }
}
__host__ __device__ constexpr int elem_bytes(int dt) { return (dt == DT_FP8 || dt == DT_I8) ? 1 : 2; }

#include "fp_nn_conv_kernels.inc"
#include "fp_nn_attention_kernels.inc"
#include "fp_nn_small_kernels.inc"
#include "fp_nn_enc_kernels.inc"

// =================================================================================================
// weights
// =================================================================================================

struct HostTensor {
  std::vector<int> shape;
  std::vector<float> data;
};

static bool read_fpw(const char *path, std::map<std::string, HostTensor> &out, std::string *err) {
  FILE *f = std::fopen(path, "rb");
  if (!f) { *err = std::string("cannot open ") + path; return false; }
  char magic[4];
  uint32_t n = 0;
  bool ok = std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "FPW1", 4) == 0 && std::fread(&n, 4, 1, f) == 1 && n <= 4096;
  for (uint32_t i = 0; ok && i < n; i++) {
    uint32_t ln = 0, nd = 0;
    ok = std::fread(&ln, 4, 1, f) == 1 && ln < 4096;
    std::string name(ok ? ln : 0, '\0');
    ok = ok && std::fread(&name[0], 1, ln, f) == ln && std::fread(&nd, 4, 1, f) == 1 && nd <= 8;
    HostTensor t;
    size_t cnt = 1;
    for (uint32_t d = 0; ok && d < nd; d++) {
      uint32_t s = 0;
      ok = std::fread(&s, 4, 1, f) == 1 && s <= (1u << 24);
      t.shape.push_back((int)s);
      cnt *= s;
      ok = ok && cnt <= ((size_t)1 << 28);  // no tensor of these networks exceeds 2^28 elements: a corrupt header must not drive a huge allocation
    }
    uint64_t nbytes = 0;
    ok = ok && std::fread(&nbytes, 8, 1, f) == 1 && nbytes == cnt * 4;
    if (ok) {
      t.data.resize(cnt);
      ok = std::fread(t.data.data(), 4, cnt, f) == cnt;
      out[name] = std::move(t);
    }
  }
  std::fclose(f);
  if (!ok) *err = std::string("malformed FPW1 file ") + path;
  return ok;
}

struct ConvLayer {
  unsigned char *w = nullptr;  // kernel layout, element type dt
  unsigned char *wfrag = nullptr;  // 2-byte types: a second copy in MFMA-fragment order for conv_smallm_kernel (fragment_order)
  unsigned char *wstep = nullptr;  // Linear layers: the fragment-order copy with the K-step OUTER (fragment_order_step_major; enc_tail_kernel, qkv_tile_kernel)
  unsigned char *wpack = nullptr;  // a copy in the LDS-stage order of gemm_k32_kernel (Linear layers) / conv_halo_kernel (3x3 layers) (pack_stage_w)
  unsigned char *wpack128 = nullptr;  // 3x3 layers with Cout % 256 == 0: a copy in conv_big_pp_kernel's stage order (pack_stage_w128)
  unsigned char *wdeep = nullptr;     // Cout % 128 == 0, 128-byte K-steps: a copy in conv_deep_kernel's stage order (FP8 3x3 layers: = wpack, the same order)
  float *bias = nullptr;
  float *cscale = nullptr;     // 8-bit layers: [Cout] dequantisation scale of the accumulator (weight-row scale, times the consumer's
                               // inverse activation scale when the output is 8-bit only: net_apply_q8)
  int dt = DT_F16;
  // 8-bit layers keep what net_apply_q8 needs to (re-)quantise them at calibration time: f32 rows [Cout][tap][Cin] and bias
  std::vector<float> rows_f32, bias_f32;
  std::vector<float> q_sw;     // per-row weight scale of the current quantisation
  std::vector<double> q_sum;   // DT_I8: per-row sum of the quantised weights
  float *tmat_t = nullptr;     // DT_I8 [r5]: [Cin][Cout] tap sums of the weights' rounding errors, T[co][c] = sum_taps (q - v), transposed (q8_img_bias_kernel)
  int ntaps = 0;
  int Cin = 0, Cout = 0, KH = 0, KW = 0, stride = 1, pad = 0;
  int algo_K = 0;  // algorithmic reduction length for FLOP accounting (the s2d stem pads 7x7x6=294 to 512)
};
struct LinearF32 {
  float *w = nullptr, *b = nullptr;
  int out = 0, in = 0;
};
struct LNParams {
  float *g = nullptr, *b = nullptr;
};
struct MHA {
  ConvLayer in_proj, out_proj;
  LinearF32 out_proj_f32;  // same weights in f32 for the "mean first" shortcut
};
struct EncLayer {  // transformer encoder layer (refiner heads)
  MHA att;
  ConvLayer lin1, lin2;
  LNParams ln1, ln2;
  LinearF32 head;
};

// trunk activation ids (FP8 scales / calibration): 0 stem, 1 a1, 2..5 encodeA blocks, 6..9 encodeAB 256 blocks, 10 b2,
// 11..14 encodeAB 512 blocks (14 = the token tensor, never quantised)
static constexpr int N_TRUNK_ACT = 15;

struct Net {
  bool scorer = false;
  int prec = PREC_F16;
  int act_dt = DT_F16;               // element type of nn_in, of the token path and (non-FP8) of the trunk activations
  ConvLayer a0, a1, ra[2][2];        // encodeA
  ConvLayer rb[2][2], b2, rc[2][2];  // encodeAB
  EncLayer trans, rot;               // refiner
  // the two heads' QKV projections stored back to back ([2][Cout][K], [2][Cout]) for Track's grouped launch
  ConvLayer g_in_proj;
#ifdef FP_TEST_HOOKS
  ConvLayer g_out_proj, g_lin1, g_lin2;   // the same for the Linear layers of Track's launch chain (TAIL_GROUPED_CHAIN, test build)
#endif
  MHA att, att_cross;                // scorer
  LinearF32 score_lin;
  unsigned char *pe = nullptr;       // [400,512], act_dt
  // 8-bit networks (PREC_FP8 / PREC_INT8), set by net_apply_q8: per-CHANNEL activation scales of the trunk tensors that feed an
  // 8-bit convolution (real = stored * scale, DT_I8: real = (stored + 128) * scale); act_oinv = 1 / scale on the device for the
  // producers that write an f16 stream tensor together with its 8-bit copy (DT_DUAL_*); bias_fix / tok_fix = the bias correction
  // solved by the calibration sweeps (fp_api.hip: fp_calibrate)
  bool q8_ready = false;
  int qdt = DT_FP8;                                  // element type of the 8-bit layers
  int q8_blocks = 0;                                 // [r6] stages on 8-bit operands (bits: TrunkRow::stage); 0 for the 2-byte networks
  // [r6] INT8: the per-image first-order compensation (plan_trunk: img_bias) belongs to records whose corrections were SOLVED with it on,
  // i.e. records that carry frame means (version 2, fp_calibrate_*).  A round-4 record or fp_set_calibration's per-tensor scales
  // (no frame means) were solved without it: compensating on top would subtract the same term twice.
  bool q8_img_comp = false;
  bool q8_on(int layer) const;                       // 8-bit layer 0..12 (TRUNK row layer + 2): its stage is in the mask
  std::vector<float> act_scale[N_TRUNK_ACT];         // host, [channels of the activation]
  float *act_oinv[N_TRUNK_ACT] = {nullptr};          // device
  float *act_scale_dev[N_TRUNK_ACT] = {nullptr};     // device copy of act_scale (calibration statistics of 8-bit tensors)
  std::vector<float> bias_fix[13], tok_fix;          // host
  std::vector<float> out_bias0, out_fix;             // output-layer biases as loaded (refiner: trans 3 | rot 3; scorer: att.out_proj 512) and their correction
  std::vector<float> pe_host;                        // the positional table in f32 (tok_fix is added to the device copy)
  // calibration: per-channel |max| and sum of the 15 trunk activations collected on the device while the trunk runs
  // ([N_TRUNK_ACT][512] each); calib_mode 1 = |max| + sum (2-byte networks), 2 = sum only (8-bit networks, dequantised)
  float *calib_amax = nullptr;
  long long *calib_sum = nullptr;   // fixed point (2^-20): integer atomics are order-independent, so a calibration is reproducible bit for bit
  int calib_mode = 0;
  int calib_only = -1;                               // >= 0: record this activation only (the sequential correction sweeps)
  mutable double calib_count[N_TRUNK_ACT] = {0};     // interior pixels summed per activation (host side)
  std::vector<void *> allocs;
  // Two-phase loading [r5]: net_prepare reads the file and builds every layout on the HOST (no HIP call: it runs outside the
  // process-wide exclusive section); each device buffer it wants is recorded here as (address of the pointer field, bytes) and the
  // field holds a placeholder until net_commit carves one arena, uploads, and patches the fields.
  struct Pending {
    void **slot;
    std::vector<unsigned char> bytes;
  };
  std::vector<Pending> pending;
  bool deferred = false;
  const std::vector<unsigned char> *pending_bytes(const void *slot) const {
    for (const Pending &q : pending)
      if ((const void *)q.slot == slot) return &q.bytes;
    return nullptr;
  }
  ~Net() {
    for (void *p : allocs) (void)hipFree(p);
  }
};
static unsigned char g_placeholder;   // what a deferred pointer field holds between net_prepare and net_commit (never dereferenced)

// The shared CNN trunk, described once: the table of its 15 convolutions, what follows from the table alone, and plan_trunk, which
// adds the precision policy.  run_trunk walks the plan and decides nothing.
// Buffer slots of the trunk (Arena): the 2-byte tensor and, in an 8-bit network, its 1-byte operand copy
enum TrunkSlot { TS_NONE = -1, TS_NN_IN = 0, TS_STEM = 1, TS_X128 = 2, TS_X256 = 5, TS_X512 = 8, TS_TOKENS = 11, TS_COUNT = 12 };
struct TrunkRow {
  const char *tag;                // the profiler's name
  ConvLayer &(*layer)(Net &);
  int in, out, res;               // TrunkSlot; res = the skip operand (TS_NONE: no residual)
  bool ab;                        // runs over the N rendered + n_b observed images (otherwise over the N concatenated ones)
  int HW;                         // input map size
  int ipad, opad, rpad;           // zero borders of the input, output and residual tensors
  bool concat;                    // the output is the a|b channel concat: image N + i lands in channels [C/2, C) of image i (split_imgs = N)
  bool pe;                        // the layer is offered the positional table
  int act, C;                     // the output's trunk activation id (= the row's index) and channel count
  int stage;                      // bit of Net::q8_blocks; 0: 2-byte operands in every precision
  int tap;                        // TapPoint of the output (test build)
};
#define FP_TL(m) [](Net &n) -> ConvLayer & { return n.m; }
static constexpr int N_TRUNK = 15, Q8_FIRST_ROW = 2;   // rows 2..14 are the 13 layers an 8-bit network may quantise (its "layer" 0..12)
static constexpr TrunkRow TRUNK[N_TRUNK] = {
    {"conv_stem", FP_TL(a0),       TS_NN_IN,    TS_STEM,     TS_NONE,     true,  80, 2, 1, 0, false, false, 0,  64,  0, TAP_STEM},
    {"conv_a1",   FP_TL(a1),       TS_STEM,     TS_X128 + 0, TS_NONE,     true,  80, 1, 1, 0, false, false, 1,  128, 0, TAP_ACT + 1},
    // encodeA residual blocks @40x40x128; the last one writes the a|b concat directly
    {"conv_128",  FP_TL(ra[0][0]), TS_X128 + 0, TS_X128 + 1, TS_NONE,     true,  40, 1, 1, 0, false, false, 2,  128, 1, TAP_ACT + 2},
    {"conv_128",  FP_TL(ra[0][1]), TS_X128 + 1, TS_X128 + 2, TS_X128 + 0, true,  40, 1, 1, 1, false, false, 3,  128, 1, TAP_ACT + 3},
    {"conv_128",  FP_TL(ra[1][0]), TS_X128 + 2, TS_X128 + 1, TS_NONE,     true,  40, 1, 1, 0, false, false, 4,  128, 1, TAP_ACT + 4},
    {"conv_128",  FP_TL(ra[1][1]), TS_X128 + 1, TS_X256 + 0, TS_X128 + 2, true,  40, 1, 1, 1, true,  false, 5,  256, 1, TAP_ACT + 5},
    // encodeAB @40x40x256, encodeAB.2 (stride 2), @20x20x512; the last conv writes the un-bordered token tensor [N,400,512]
    {"conv_256",  FP_TL(rb[0][0]), TS_X256 + 0, TS_X256 + 1, TS_NONE,     false, 40, 1, 1, 0, false, false, 6,  256, 2, TAP_ACT + 6},
    {"conv_256",  FP_TL(rb[0][1]), TS_X256 + 1, TS_X256 + 2, TS_X256 + 0, false, 40, 1, 1, 1, false, false, 7,  256, 2, TAP_ACT + 7},
    {"conv_256",  FP_TL(rb[1][0]), TS_X256 + 2, TS_X256 + 1, TS_NONE,     false, 40, 1, 1, 0, false, false, 8,  256, 2, TAP_ACT + 8},
    {"conv_256",  FP_TL(rb[1][1]), TS_X256 + 1, TS_X256 + 0, TS_X256 + 2, false, 40, 1, 1, 1, false, false, 9,  256, 2, TAP_ACT + 9},
    {"conv_b2",   FP_TL(b2),       TS_X256 + 0, TS_X512 + 0, TS_NONE,     false, 40, 1, 1, 0, false, false, 10, 512, 4, TAP_ACT + 10},
    {"conv_512",  FP_TL(rc[0][0]), TS_X512 + 0, TS_X512 + 1, TS_NONE,     false, 20, 1, 1, 0, false, false, 11, 512, 8, TAP_ACT + 11},
    {"conv_512",  FP_TL(rc[0][1]), TS_X512 + 1, TS_X512 + 2, TS_X512 + 0, false, 20, 1, 1, 1, false, false, 12, 512, 8, TAP_ACT + 12},
    {"conv_512",  FP_TL(rc[1][0]), TS_X512 + 2, TS_X512 + 1, TS_NONE,     false, 20, 1, 1, 0, false, false, 13, 512, 8, TAP_ACT + 13},
    {"conv_512",  FP_TL(rc[1][1]), TS_X512 + 1, TS_TOKENS,   TS_X512 + 2, false, 20, 1, 0, 1, false, true,  14, 512, 8, TAP_ACT + 14},
};
#undef FP_TL
static constexpr bool trunk_is_chain() {   // what plan_trunk relies on: row r writes activation r and row r + 1 reads it
  for (int r = 0; r < N_TRUNK; r++)
    if (TRUNK[r].act != r || (r + 1 < N_TRUNK && TRUNK[r + 1].in != TRUNK[r].out)) return false;
  return N_TRUNK == N_TRUNK_ACT;
}
static_assert(trunk_is_chain(), "TRUNK: not a chain of the 15 trunk activations");
static constexpr int trunk_writer(int r, int s) {   // the row that wrote slot s last in front of row r
  for (int i = r - 1; i >= 0; i--)
    if (TRUNK[i].out == s) return i;
  return -1;
}
// row r starts or continues a residual stream: a later row reads its output as the skip operand
static constexpr bool trunk_out_is_skip(int r) {
  for (int i = r + 1; i < N_TRUNK; i++) {
    if (TRUNK[i].res == TRUNK[r].out) return true;
    if (TRUNK[i].out == TRUNK[r].out) return false;
  }
  return false;
}
// a block's first conv: no residual, and nobody but the next 8-bit convolution reads its output -- the consumer's scales fold into
// cscale / bias (legal: no residual, ReLU)
static constexpr bool trunk_folded_out(int r) { return TRUNK[r].stage != 0 && TRUNK[r].res == TS_NONE && !trunk_out_is_skip(r); }
inline bool Net::q8_on(int layer) const { return (q8_blocks & TRUNK[Q8_FIRST_ROW + layer].stage) != 0; }
static const ConvLayer &trunk_layer(const Net &n, int r) { return TRUNK[r].layer(const_cast<Net &>(n)); }
static constexpr int trunk_layer_cout(int r) { return TRUNK[r].concat ? TRUNK[r].C / 2 : TRUNK[r].C; }   // (the concat row writes one half per image group)
static constexpr int Q8_IMG_BIAS_MIN_N = 16;   // INT8: passes of fewer hypotheses run without the per-image compensation (plan_trunk)

struct TrunkQuery {
  int dt = DT_F16;          // the 2-byte element type: every tensor of a 2-byte network; nn_in, the stem, the residual stream and the tokens of an 8-bit one
  int qdt = -1;             // DT_FP8 / DT_I8: an 8-bit network; -1: a 2-byte network
  int mask = 0;             // 8-bit network: the stages on 8-bit operands (TrunkRow::stage bits)
  bool i8_stream = false;   // test build, DT_I8: the residual stream itself is 8-bit
  bool img_comp = false;    // INT8: the per-image compensation is available in this call (a record solved with it, its buffers, its switch) ...
  unsigned comp_rows = 0;   // ... and bit r: row r's layer carries the tap sums of its rounding errors (ConvLayer::tmat_t)
  int N = 1, n_b = 1;       // hypotheses; observed crops behind them (N, or 1 = shared)
};
// What one row does, in this order: per-image bias, convolution, 2-byte broadcast, 8-bit broadcast, q8_copy, calibration record, tap.
// Slots are TrunkSlot, activation indices select a row of Net::act_oinv / act_scale_dev; TS_NONE / -1 = none.
struct TrunkStep {
  int op_dt = DT_F16;                           // element type of the weights and the input
  int in = TS_NONE;   bool in_q = false;        // the input: the slot's 2-byte tensor or its 8-bit copy
  int res = TS_NONE;  bool res_q = false;       // the skip operand, likewise ...
  int rscale = -1;                              // ... and the activation whose scales de-quantise an 8-bit one in the epilogue
  int out16 = TS_NONE, outq = TS_NONE;          // the epilogue writes the 2-byte tensor / the 8-bit copy (both: DT_DUAL_*) ...
  int oinv = -1;                                // ... the copy scaled by this activation's inverse scales (-1: folded into the layer's tables)
  bool img_bias = false;                        // INT8: the bias comes per image from q8_img_bias_fused_kernel on the 8-bit input
  bool bcast16 = false, bcastq = false;         // the shared crop's half of the concat is replicated: 2-byte tensor / 8-bit copy
  int qcopy = -1;                               // q8_copy_kernel makes the 8-bit copy from the 2-byte output, with this activation's inverse scales
  int rec = TS_NONE;  bool rec_q = false;       // calibration statistics: of this slot's 2-byte tensor or 8-bit copy ...
  int rec_dt = -1, rec_scale = -1;              // ... of this element type, de-quantised with this activation's scales
};
struct TrunkPlan { TrunkStep step[N_TRUNK]; };
// The precision policy of the trunk: pure, no HIP call, no decision outside its arguments.
//   2-byte network: every row on q.dt.
//   8-bit network [r4, r6]: a stage in the mask reads 8-bit operands, the others keep their 2-byte weights and kernels.  The RESIDUAL
//   STREAM stays f16, so the skip path is never re-quantised and the tensor a stage hands over always exists in f16 unless nobody reads
//   it.  An 8-bit row's producer leaves the 8-bit copy as well: from its own epilogue when it is an 8-bit layer or one of the two
//   2-byte rows in front of the stages (their kernels have the f16 -> dual-output form), through q8_copy_kernel when it is a 2-byte
//   layer of a stage outside the mask (the resident-halo and 256x256 schedules have no such form).
//   i8_stream [r4, test build: tools/q8_cross.py]: no f16 stream at all -- a block's second conv reads its skip operand from the 8-bit
//   copy and writes only the new one (DT_QSR_I8); every stage is 8-bit whatever the mask says.  Not shipped: DESIGN.md section 4.4.
static int plan_trunk(const TrunkQuery &q, TrunkPlan *plan) {
  *plan = TrunkPlan{};
  const bool q8 = q.qdt >= 0;
  FP_CHECK(q.dt == DT_F16 || q.dt == DT_BF16, "plan_trunk: the stem and the token path run on 2-byte elements");
  FP_CHECK(!q8 || (is_q8(q.qdt) && q.dt == DT_F16), "plan_trunk: an 8-bit trunk is FP8 or INT8 layers in an f16 network");
  FP_CHECK(q.N >= 1 && (q.n_b == q.N || q.n_b == 1), "plan_trunk: invalid query");
  const bool i8s = q.i8_stream && q.qdt == DT_I8;
  const int mask = !q8 ? 0 : i8s ? ~0 : q.mask;
  const auto on = [&](int r) { return r < N_TRUNK && (mask & TRUNK[r].stage) != 0; };
  // the image's own first-order term of the weights' rounding error [r5, r6].  The decision is per CALL (N), not per layer: a pass of
  // fewer than 16 hypotheses -- Track, small shards -- runs without it (26 more launches would double a Track) and carries that term
  // uncorrected, the record's corrections being solved on full Registers WITH it: on Track 0.24 deg / 0.28 mm against f16
  const bool comp = q.qdt == DT_I8 && !i8s && q.img_comp && q.N >= Q8_IMG_BIAS_MIN_N;
  for (int r = 0; r < N_TRUNK; r++) {
    const TrunkRow &t = TRUNK[r];
    TrunkStep &s = plan->step[r];
    const bool need_q = on(r + 1);                             // the next row reads 8-bit operands
    const bool epi_q = need_q && (on(r) || t.stage == 0);      // ... and this row's epilogue can write them
    // no 2-byte output: nobody reads it (the next row is 8-bit and no later row takes it as its skip operand)
    const bool drop16 = need_q && (i8s || (on(r) && !trunk_out_is_skip(r)));
    s.op_dt = on(r) ? q.qdt : q.dt;
    s.in = t.in; s.in_q = on(r);
    s.res = t.res; s.res_q = i8s && t.res != TS_NONE;
    s.rscale = s.res_q ? TRUNK[trunk_writer(r, t.res)].act : -1;
    s.out16 = drop16 ? TS_NONE : t.out; s.outq = epi_q ? t.out : TS_NONE;
    s.oinv = epi_q && !trunk_folded_out(r) ? t.act : -1;
    s.img_bias = comp && on(r) && ((q.comp_rows >> r) & 1u) != 0;
    const bool bcast = t.concat && q.n_b == 1 && q.N > 1;
    s.bcast16 = bcast && !drop16; s.bcastq = bcast && epi_q;
    s.qcopy = need_q && !epi_q ? t.act : -1;
    // every activation but the stem's is recorded, in the form the trunk keeps it; an f16-stream 8-bit trunk skips encodeA.1's too (a
    // 2-byte layer in front of every stage: the correction sweeps have nothing to solve there)
    if (t.act >= 1 && (t.stage != 0 || !q8 || i8s)) {
      s.rec = t.out; s.rec_q = drop16;
      s.rec_dt = drop16 ? q.qdt : q.dt; s.rec_scale = drop16 ? t.act : -1;
    }
  }
  return 0;
}

template <typename T>
static T *upload(Net *net, const std::vector<T> &h) {
  if (net->deferred) return nullptr;   // (every load-time buffer goes through put(): the field's address is what net_commit patches)
  T *d = nullptr;
  if (hipMalloc((void **)&d, std::max<size_t>(h.size(), 1) * sizeof(T)) != hipSuccess) return nullptr;
  net->allocs.push_back(d);
  if (fp::memcpy_sync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}

// device copy of a host vector: allocated the first time, overwritten in place afterwards (re-calibration of an 8-bit network)
template <typename T>
static bool put(Net *net, T *&dst, const std::vector<T> &h) {
  if (net->deferred) {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(h.data());
    for (Net::Pending &q : net->pending)
      if (q.slot == (void **)&dst) { q.bytes.assign(b, b + h.size() * sizeof(T)); return true; }
    net->pending.push_back({(void **)&dst, std::vector<unsigned char>(b, b + h.size() * sizeof(T))});
    dst = reinterpret_cast<T *>(&g_placeholder);
    return true;
  }
  if (!dst) { dst = upload(net, h); return dst != nullptr; }
  return fp::memcpy_sync(dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}
static bool put_bytes(Net *net, unsigned char *&dst, const std::vector<unsigned char> &h) { return put<unsigned char>(net, dst, h); }

// ---- host-side element conversion (round to nearest even) ----
static uint16_t f32_to_bf16_bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// OCP FP8 e4m3fn: 1-4-3, bias 7, max 448, no infinities; saturating
static uint8_t f32_to_e4m3_bits(float x) {
  const uint8_t sign = std::signbit(x) ? 0x80 : 0;
  const float a = std::fabs(x);
  if (!(a == a)) return (uint8_t)(sign | 0x7f);
  if (a >= 448.f) return (uint8_t)(sign | 0x7e);
  if (a < 0x1p-10f) return sign;  // below half of the smallest subnormal (2^-9)
  int e;
  (void)std::frexp(a, &e);
  int E = e - 1;  // a in [2^E, 2^(E+1))
  if (E < -6) {   // subnormal: quantum 2^-9
    const int r = (int)std::nearbyint(a * 512.f);
    return (uint8_t)(sign | (r >= 8 ? 0x08 : r));
  }
  int r = (int)std::nearbyint(std::ldexp(a, 3 - E));  // 8..16
  if (r == 16) { r = 8; E++; }
  if (E > 8 || (E == 8 && r > 14)) return (uint8_t)(sign | 0x7e);
  return (uint8_t)(sign | ((E + 7) << 3) | (r - 8));
}
// rows of `K` floats -> kernel element bytes (2-byte types; the 8-bit layers go through quantise_q8)
static std::vector<unsigned char> to_elems(const std::vector<float> &w, int rows, int K, int dt, std::vector<float> *row_scale) {
  std::vector<unsigned char> o((size_t)rows * K * 2);
  if (row_scale) row_scale->assign(rows, 1.f);
  for (int r = 0; r < rows; r++) {
    const float *src = &w[(size_t)r * K];
    uint16_t *dst = reinterpret_cast<uint16_t *>(&o[(size_t)r * K * 2]);
    for (int k = 0; k < K; k++) {
      if (dt == DT_BF16) dst[k] = f32_to_bf16_bits(src[k]);
      else { __half h = __float2half(src[k]); std::memcpy(&dst[k], &h, 2); }
    }
  }
  return o;
}

// [a | b] copy of two equally shaped Linear layers (weights already in kernel row order), concatenated on the host from the
// layers' pending uploads (net_prepare)
static bool make_grouped(Net *net, const ConvLayer &a, const ConvLayer &b, ConvLayer *g) {
  if (a.Cin != b.Cin || a.Cout != b.Cout || a.dt != b.dt || !net->deferred) return false;
  auto cat = [&](const void *sa, const void *sb, std::vector<unsigned char> *out) {
    const std::vector<unsigned char> *pa = net->pending_bytes(sa), *pb = net->pending_bytes(sb);
    if (!pa || !pb || pa->size() != pb->size()) return false;
    *out = *pa;
    out->insert(out->end(), pb->begin(), pb->end());
    return true;
  };
  *g = a;
  g->w = nullptr; g->bias = nullptr; g->wfrag = nullptr; g->wpack = nullptr; g->wpack128 = nullptr; g->wdeep = nullptr;   // (the grouped launch never runs on gemm_k32_kernel)
  g->wstep = nullptr; g->tmat_t = nullptr; g->cscale = nullptr;   // (copied as placeholders from `a`: a host address no launch may ever see)
  std::vector<unsigned char> buf;
  if (!cat(&a.w, &b.w, &buf) || !put_bytes(net, g->w, buf)) return false;
  {
    std::vector<unsigned char> bb;
    if (!cat(&a.bias, &b.bias, &bb)) return false;
    std::vector<float> bf(bb.size() / 4);
    std::memcpy(bf.data(), bb.data(), bb.size());
    if (!put(net, g->bias, bf)) return false;
  }
  // (a group's fragment-order / deep-ring copy has the size of its row-major copy: the same group stride serves them)
  if (a.wfrag && b.wfrag && (!cat(&a.wfrag, &b.wfrag, &buf) || !put_bytes(net, g->wfrag, buf))) return false;
  if (a.wdeep && b.wdeep && (!cat(&a.wdeep, &b.wdeep, &buf) || !put_bytes(net, g->wdeep, buf))) return false;
  return true;
}

static bool get(const std::map<std::string, HostTensor> &m, const std::string &name, const HostTensor **t, std::string *err) {
  auto it = m.find(name);
  if (it == m.end()) { *err = "missing tensor " + name; return false; }
  *t = &it->second;
  return true;
}
static bool shape_is(const HostTensor *t, std::initializer_list<int> want) { return t->shape == std::vector<int>(want); }

// [Cout][tap][Cin] -> kernel K order: for Cin >= 64 [Cout][Cin/CH][tap][CH] with CH = the channels of a 128-byte chunk (64
// for the 2-byte types, 128 for FP8), otherwise unchanged.  `es` = element bytes.
static std::vector<unsigned char> relayout_k(const std::vector<unsigned char> &w, int Cout, int ntaps, int Cin, int es) {
  const int CH = 128 / es;
  if (Cin < 64 || ntaps == 1) return w;
  std::vector<unsigned char> o(w.size());
  const int nch = Cin / CH;
  for (int co = 0; co < Cout; co++)
    for (int t = 0; t < ntaps; t++)
      for (int c0 = 0; c0 < nch; c0++)
        std::memcpy(&o[((((size_t)co * nch + c0) * ntaps + t) * CH) * es], &w[(((size_t)co * ntaps + t) * Cin + (size_t)c0 * CH) * es], (size_t)CH * es);
  return o;
}

// Row permutation matching conv_epilogue: inside every block of 16*NI output channels (NI = 4, or 2 when Cout == 64)
// kernel row ni*16 + 4g + j holds the weights of channel 32*(j>>1) + 8g + 4*(j&1) + ni (NI=4) / 8g + 2j + ni (NI=2).
static std::vector<unsigned char> permute_rows(const std::vector<unsigned char> &w, int Cout, size_t row_bytes) {
  const int NI = (Cout % 128 == 0) ? 4 : 2, blk = 16 * NI;
  std::vector<unsigned char> o(w.size());
  for (int b0 = 0; b0 < Cout; b0 += blk)
    for (int ni = 0; ni < NI; ni++)
      for (int g = 0; g < 4; g++)
        for (int j = 0; j < 4; j++) {
          int ch = (NI == 4) ? 32 * (j >> 1) + 8 * g + 4 * (j & 1) + ni : 8 * g + 2 * j + ni;
          std::memcpy(&o[(size_t)(b0 + ni * 16 + 4 * g + j) * row_bytes], &w[(size_t)(b0 + ch) * row_bytes], row_bytes);
        }
  return o;
}

// Fragment order for conv_smallm_kernel, which loads its weight operands global -> registers: the vector L1 serves a wave's
// 16-byte loads four lanes at a time and takes one clock per DISTINCT cache line in each group of four (tools/bench_tcp.hip: a load in
// MFMA-operand shape -- lane -> row lane & 15 -- costs 64 clocks per wave instruction at any row pitch, a load of 1 KB of
// consecutive bytes 18).  So the bytes lane l needs for (16-row tile t, 128-byte K-step kt, half ks) are stored at
//     ((t * KT + kt) * 2 + ks) * 1024 + l * 16       <-  row t*16 + (l & 15), bytes kt*128 + ks*64 + (l >> 4)*16 .. +15
// Same size as the row-major copy; `w` is that copy ([Cout][row_bytes], rows already permuted).
static std::vector<unsigned char> fragment_order(const std::vector<unsigned char> &w, int Cout, size_t row_bytes) {
  const size_t KT = row_bytes / 128;
  std::vector<unsigned char> o(w.size());
  for (size_t t = 0; t < (size_t)Cout / 16; t++)
    for (size_t kt = 0; kt < KT; kt++)
      for (int ks = 0; ks < 2; ks++)
        for (int l = 0; l < 64; l++)
          std::memcpy(&o[((t * KT + kt) * 2 + ks) * 1024 + (size_t)l * 16], &w[(t * 16 + (l & 15)) * row_bytes + kt * 128 + ks * 64 + (size_t)(l >> 4) * 16], 16);
  return o;
}

// The same 1 KB fragments with the 64-byte K-step OUTER: fragment (16-row tile t, K-step s) at (s * Cout / 16 + t) KB.  The tile kernels of the
// Linear layers (enc_tail_kernel, qkv_tile_kernel: eight waves x four row tiles per K-step) read 32 CONSECUTIVE KB per step this way; in
// the tile-outer order the same 32 fragments lie 16 KB apart and fall on a few L2 channels, which every workgroup of an XCD -- they start
// together and stream the same bytes in the same order -- then hammers at the same time.
static std::vector<unsigned char> fragment_order_step_major(const std::vector<unsigned char> &w, int Cout, size_t row_bytes) {
  const size_t S = row_bytes / 64, T = (size_t)Cout / 16;
  std::vector<unsigned char> o(w.size());
  for (size_t t = 0; t < T; t++)
    for (size_t s = 0; s < S; s++)
      for (int l = 0; l < 64; l++)
        std::memcpy(&o[(s * T + t) * 1024 + (size_t)l * 16], &w[(t * 16 + (l & 15)) * row_bytes + s * 64 + (size_t)(l >> 4) * 16], 16);
  return o;
}

// Stage order for the kernels that stream a [TILE rows][64 B] weight stage per K-step through LDS-DMA (gemm_k32_kernel: TILE = 256,
// conv_halo_kernel: TILE = 128): the PW pieces (16 rows x 64 B each; lane -> row = lane >> 2, swizzled 16-byte chunk) wave `w` of a
// workgroup stages for (row tile nt, 64-byte K-step st) are stored as ONE run at ((nt * S + st) * 4 + w) * PW KB -- the DMA then
// needs one address and one M0 per PW pieces (glds16x4_asm / glds16x2_asm), and every fetched cache line is used whole.
static std::vector<unsigned char> pack_stage_w(const std::vector<unsigned char> &w, int Cout, size_t row_bytes, int TILE) {
  const size_t S = row_bytes / 64;
  const int PW = TILE / 64;
  std::vector<unsigned char> o(w.size());
  for (size_t nt = 0; nt < (size_t)Cout / TILE; nt++)
    for (size_t st = 0; st < S; st++)
      for (int wv = 0; wv < 4; wv++)
        for (int i = 0; i < PW; i++)
          for (int l = 0; l < 64; l++) {
            const int prow = l >> 2, gch = (l & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
            std::memcpy(&o[(((nt * S + st) * 4 + wv) * PW + i) * 1024 + (size_t)l * 16],
                        &w[(nt * TILE + (size_t)(wv * PW + i) * 16 + prow) * row_bytes + st * 64 + (size_t)gch * 16], 16);
          }
  return o;
}

// The same for the kernels with 128-byte K-steps: conv_big_pp_kernel (TILE = 256 rows, NW = 8 waves) and the FP8 conv_halo8_kernel
// (TILE = 128, NW = 4); 4 pieces of 8 rows x 128 B per wave, lane -> row = lane >> 3, 16-byte chunk (lane & 7) ^ row: wave `w`'s 4 KB
// of (row tile nt, K-step kt) at ((nt * KT + kt) * NW + w) * 4096.  Byte-level, so it serves every element type.
static std::vector<unsigned char> pack_stage_w128(const std::vector<unsigned char> &w, int Cout, size_t row_bytes, int TILE, int NW) {
  const size_t KT = row_bytes / 128;
  std::vector<unsigned char> o(w.size());
  for (size_t nt = 0; nt < (size_t)Cout / TILE; nt++)
    for (size_t kt = 0; kt < KT; kt++)
      for (int wv = 0; wv < NW; wv++)
        for (int i = 0; i < 4; i++)
          for (int l = 0; l < 64; l++) {
            const int srow = l >> 3, g = (l & 7) ^ srow;
            std::memcpy(&o[(((nt * KT + kt) * NW + wv) * 4 + i) * 1024 + (size_t)l * 16],
                        &w[(nt * TILE + (size_t)(wv * 4 + i) * 8 + srow) * row_bytes + kt * 128 + (size_t)g * 16], 16);
          }
  return o;
}

// element bytes [Cout][tap][Cin] -> every device layout the layer's schedules stream from
static bool upload_layouts(Net *net, const std::vector<unsigned char> &elems, int Cout, int ntaps, int Cin, int dt, ConvLayer *L) {
  const int K = ntaps * Cin, es = elem_bytes(dt);
  const auto rows = permute_rows(relayout_k(elems, Cout, ntaps, Cin, es), Cout, (size_t)K * es);
  if (!put_bytes(net, L->w, rows)) return false;
  if (((size_t)K * es) % 128 == 0 && Cout % 16 == 0) {   // (byte-level: every element type)
    if (!put_bytes(net, L->wfrag, fragment_order(rows, Cout, (size_t)K * es))) return false;
    if (ntaps == 1 && es == 2 && !put_bytes(net, L->wstep, fragment_order_step_major(rows, Cout, (size_t)K * es))) return false;
  }
  if (!is_q8(dt) && ntaps == 1 && ((size_t)K * es) % 64 == 0 && Cout % 256 == 0) {
    if (!put_bytes(net, L->wpack, pack_stage_w(rows, Cout, (size_t)K * es, 256))) return false;      // gemm_k32_kernel
  } else if (!is_q8(dt) && ntaps == 9 && Cin % 64 == 0 && Cout % 128 == 0) {
    if (!put_bytes(net, L->wpack, pack_stage_w(rows, Cout, (size_t)K * es, 128))) return false;      // conv_halo_kernel
  }
  if (ntaps == 9 && ((size_t)K * es) % 128 == 0 && Cout % 256 == 0) {
    if (!put_bytes(net, L->wpack128, pack_stage_w128(rows, Cout, (size_t)K * es, 256, 8))) return false;   // conv_big_pp_kernel
  }
  if (is_q8(dt) && ntaps == 9 && ((size_t)K * es) % 128 == 0 && Cout % 128 == 0) {
    if (!put_bytes(net, L->wpack, pack_stage_w128(rows, Cout, (size_t)K * es, 128, 4))) return false;      // conv_halo8_kernel
    L->wdeep = L->wpack;                                                                                   // conv_deep_kernel: the same order
  } else if (((size_t)K * es) % 128 == 0 && Cout % 128 == 0) {
    if (!put_bytes(net, L->wdeep, pack_stage_w128(rows, Cout, (size_t)K * es, 128, 4))) return false;      // conv_deep_kernel
  }
  return true;
}

// 8-bit quantisation of a layer's rows with the per-INPUT-channel activation scales folded in first (w'[co][tap][ci] = w * s_in[ci];
// s_in = null: all 1): per output row a scale sw (FP8: amax / 448, OCP e4m3, RNE, saturating; I8: amax / 127) and, for I8, the
// row sum of the quantised integers (the -128 offset of the unsigned activations contributes 128 * sum to every accumulator).
//
// I8 rounding [r5]: ERROR-FEEDBACK rounding against the calibration frames' channel means (m_int: [J][Cin], the mean INTEGER
// activation of every input channel in each of J calibration frames; null = round to nearest).  Why: with round-to-nearest the
// weight errors d_k of a row are independent, so the row's mean output error sum_k d_k * mean(x_k) is a random walk over K = 1152-4608
// terms -- a common-mode shift of every hypothesis' features that the discriminating heads amplify, and that differs from scene to
// scene with the channel means (tools/q8_sim_cross.py: ALL of the cross-scene common-mode error of the INT8 trunk comes from the
// weights, none from the 8-bit activations; a bias correction removes it only for the calibration frames' own means).  Here every
// weight whose fraction lies within TAU of .5 (either neighbour costs almost the same rounding error) is rounded up or down so that
// the running sums r_j = sum_k d_k m_j[c(k)] stay near zero for EVERY frame j: the mean error cancels by construction, also for
// scenes whose channel means are (near) combinations of the calibration frames'.  Weights further from .5 round to nearest, which
// keeps the per-pixel (de-meaned) error where it was.
#ifdef FP_TEST_HOOKS
static float g_q8_headroom = 1.25f;   // INT8 activation scale = |max| * headroom / 255 (tools/q8_multi.py --headroom)
// imgbias: the per-image first-order compensation (q8_img_bias_kernel); wclip / efr: the row-step search / rounding form of quantise_q8
static int g_q8_wclip = 1, g_q8_efr = 2, g_q8_imgbias = 1;   // A/B (tools/q8_multi.py --wq): the row-step search / the error-feedback rounding of quantise_q8
#else
static constexpr float g_q8_headroom = 1.25f;
static constexpr int g_q8_wclip = 1, g_q8_efr = 2, g_q8_imgbias = 1;
#endif
// [r6] which residual stages of the trunk an 8-bit network runs on 8-bit operands (the others keep their f16 weights and kernels):
// bit 0 = encodeA.2-3 (4 convs, 128 ch), bit 1 = encodeAB.0-1 (4 convs, 256 ch), bit 2 = encodeAB.2 (3x3 / s2, 256 -> 512),
// bit 3 = encodeAB.3-4 (4 convs, 512 ch).  A network keeps the mask it was loaded with (Net::q8_blocks).
static constexpr int Q8_BLOCKS_ALL = 15;
#ifdef FP_TEST_HOOKS
static int env_int(const char *name, int dflt) { const char *e = std::getenv(name); return e && *e ? std::atoi(e) : dflt; }
static int g_q8_blocks = env_int("FP_Q8_BLOCKS", Q8_BLOCKS_ALL);   // A/B (fpt_set_q8_blocks; tools/q8_blocks.py): networks loaded AFTER a change carry the new mask
#else
static constexpr int g_q8_blocks = Q8_BLOCKS_ALL;
#endif
#ifdef FP_TEST_HOOKS
static float env_float(const char *name, float dflt) { const char *e = std::getenv(name); return e && *e ? (float)std::atof(e) : dflt; }
static const float kEfrTau = env_float("FP_Q8_TAU", 0.2f), kEfrLam = env_float("FP_Q8_LAM", 0.05f);   // A/B of the rounding knobs (tools/q8_multi.py)
#else
static constexpr float kEfrTau = 0.2f, kEfrLam = 0.05f;
#endif
static std::vector<unsigned char> quantise_q8(const ConvLayer &L, int dt, const float *s_in, std::vector<float> *sw, std::vector<double> *qsum,
                                              const float *m_int = nullptr, int J = 0, std::vector<float> *tmat_t = nullptr) {
  const int K = L.ntaps * L.Cin;
  std::vector<unsigned char> o((size_t)L.Cout * K);
  if (tmat_t) tmat_t->assign((size_t)L.Cin * L.Cout, 0.f);
  sw->assign(L.Cout, 1.f);
  qsum->assign(L.Cout, 0.0);
  std::vector<float> wf(K);
  std::vector<double> r(std::max(J, 1));
  for (int co = 0; co < L.Cout; co++) {
    const float *src = &L.rows_f32[(size_t)co * K];
    float amax = 0.f;
    for (int k = 0; k < K; k++) {
      wf[k] = s_in ? src[k] * s_in[k % L.Cin] : src[k];
      amax = std::max(amax, std::fabs(wf[k]));
    }
    float sc = amax > 0.f ? amax / (dt == DT_FP8 ? 448.f : 127.f) : 1.f;
    if (dt == DT_I8 && m_int && J > 0 && amax > 0.f && g_q8_wclip) {
      // the row's step [r5]: the range that minimises the activation-weighted squared rounding + clipping error,
      // sum_k (q_k sc - w_k)^2 E_j[m_j,c(k)^2], over amax * {1, .95, ..., .5} / 127 -- a row's few largest folded weights (large weight on a
      // channel with a large activation scale) otherwise set the step of the thousands of ordinary ones
      std::vector<double> m2(L.Cin, 0.0);
      for (int j = 0; j < J; j++)
        for (int c = 0; c < L.Cin; c++) m2[c] += (double)m_int[(size_t)j * L.Cin + c] * m_int[(size_t)j * L.Cin + c] / J;
      double best = -1;
      float best_sc = sc;
      for (int step = 0; step <= 10; step++) {
        const float cand = amax * (1.f - 0.05f * step) / 127.f;
        double err = 0;
        for (int k = 0; k < K; k++) {
          const float q = std::max(-127.f, std::min(127.f, std::nearbyint(wf[k] / cand)));
          const double d = (double)q * cand - wf[k];
          err += d * d * (m2[k % L.Cin] + 1.0);
        }
        if (best < 0 || err < best) { best = err; best_sc = cand; }
      }
      sc = best_sc;
    }
    (*sw)[co] = sc;
    double qs = 0;
    std::fill(r.begin(), r.end(), 0.0);
    if (dt == DT_I8 && m_int && J > 0 && g_q8_efr == 2) {
      // ---- per input channel: the TAP SUM of the rounding errors [r5, second form] ---------------------------------------------
      // The mean output error of the row is sum_c T_c mean(x_c) with T_c = sum over the taps of channel c of its weights' rounding
      // errors (every tap of a channel sees the same mean).  Cancelling it against the calibration frames' means (first form) leaves
      // what a NEW scene's means add: mean(x_c) = m_c (1 + eps_c) with eps_c different per scene and channel, i.e. an error
      // sum_c T_c m_c eps_c that no finite set of calibration frames spans.  It is small for EVERY scene when every |T_c| is small:
      // round to nearest, then flip the weights closest to .5 (|fraction - .5| < TAU) while that brings |T_c| towards <= .5 (standard
      // deviation 0.86 -> 0.42 steps: not every channel has an eligible weight on the right side), and use the last free choice per channel (T_c or T_c -+ 1 when |T_c| is near .5) to keep the
      // running sums r_j = sum_c T_c m_jc of the calibration frames near zero.
      const int nt = L.ntaps, Cin = L.Cin;
      std::vector<int> qv(nt);
      std::vector<float> fr(nt);
      std::vector<char> can(nt);
      for (int c = 0; c < Cin; c++) {
        double T = 0;
        for (int t = 0; t < nt; t++) {
          const float v = wf[(size_t)t * Cin + c] / sc;
          const float base = std::floor(v);
          fr[t] = v - base;
          qv[t] = std::max(-127, std::min(127, (int)base + (fr[t] >= 0.5f ? 1 : 0)));
          can[t] = std::fabs(fr[t] - 0.5f) < kEfrTau && std::fabs(v) < 126.f;
          T += (double)qv[t] - (double)v;
        }
        auto flip_toward = [&](int dir) -> bool {   // dir = +1: raise T by one (flip a rounded-down weight up), -1: lower it; cheapest eligible weight
          int best = -1;
          float best_cost = 1e9f;
          for (int t = 0; t < nt; t++) {
            if (!can[t]) continue;
            const bool is_up = fr[t] >= 0.5f ? qv[t] == (int)std::floor(wf[(size_t)t * Cin + c] / sc) + 1 : false;
            const int cur = qv[t] - (int)std::floor(wf[(size_t)t * Cin + c] / sc);   // 0 = down, 1 = up
            (void)is_up;
            if (dir > 0 && cur != 0) continue;
            if (dir < 0 && cur != 1) continue;
            const float cost = std::fabs(fr[t] - 0.5f);
            if (cost < best_cost) { best_cost = cost; best = t; }
          }
          if (best < 0) return false;
          qv[best] += dir;
          can[best] = 0;   // a weight is moved at most once
          T += dir;
          return true;
        };
        while (T > 0.5 && flip_toward(-1)) {}
        while (T < -0.5 && flip_toward(+1)) {}
        // the free choice: T or T - sign(T) (|.| = 1 - |T|): take it when it serves the calibration frames' running sums more than it costs
        {
          const int dir = T > 0 ? -1 : +1;
          double now = 0, alt = 0, mbar2 = 0;
          for (int j = 0; j < J; j++) {
            const double m = m_int[(size_t)j * Cin + c];
            const double a = r[j] + T * m, b2 = r[j] + (T + dir) * m;
            now += a * a; alt += b2 * b2; mbar2 += m * m;
          }
          const double lam = (double)kEfrLam * mbar2;   // what a unit of T_c^2 costs on unseen scenes: (scene-to-scene variation of a channel mean ~ 20 %)^2 x m^2
          if (alt + lam * (T + dir) * (T + dir) < now + lam * T * T) {
            const double keep = T;
            if (!flip_toward(dir)) T = keep;
          }
        }
        for (int j = 0; j < J; j++) r[j] += T * m_int[(size_t)j * Cin + c];
        if (tmat_t) (*tmat_t)[(size_t)c * L.Cout + co] = (float)T;
        for (int t = 0; t < nt; t++) {
          o[(size_t)co * K + (size_t)t * Cin + c] = (unsigned char)(signed char)qv[t];
          qs += qv[t];
        }
      }
      (*qsum)[co] = qs;
      continue;
    }
    for (int k = 0; k < K; k++) {
      if (dt == DT_FP8) { o[(size_t)co * K + k] = f32_to_e4m3_bits(wf[k] / sc); continue; }
      const float v = wf[k] / sc;
      int q;
      if (m_int && J > 0) {
        const float base = std::floor(v), frac = v - base;
        bool up = frac >= 0.5f;
        const int c = k % L.Cin;
        const double e_dn = -(double)frac, e_up = 1.0 - (double)frac;
        if (std::fabs(frac - 0.5f) < kEfrTau && std::fabs(v) < 126.f) {
          double c_dn = 0, c_up = 0;
          for (int j = 0; j < J; j++) {
            const double m = m_int[(size_t)j * L.Cin + c];
            const double a = r[j] + e_dn * m, b = r[j] + e_up * m;
            c_dn += a * a; c_up += b * b;
          }
          up = c_up < c_dn;
        }
        q = std::max(-127, std::min(127, (int)base + (up ? 1 : 0)));
        const double e = (double)q - (double)v;   // (the error actually made: a clipped weight's is larger than one step)
        for (int j = 0; j < J; j++) r[j] += e * m_int[(size_t)j * L.Cin + c];
      } else {
        q = (int)std::max(-127.f, std::min(127.f, std::nearbyint(v)));
      }
      o[(size_t)co * K + k] = (unsigned char)(signed char)q;
      qs += q;
      if (tmat_t && dt == DT_I8) (*tmat_t)[(size_t)(k % L.Cin) * L.Cout + co] += (float)((double)q - (double)v);
    }
    (*qsum)[co] = qs;
  }
  return o;
}

// [Cout][KH][KW][Cin] f32 rows -> device layer of element type dt.  8-bit layers are quantised with unit activation scales here
// (so that every buffer exists) and again, with the calibrated scales, by net_apply_q8.
static bool finish_layer(Net *net, const std::vector<float> &rows_f32, const std::vector<float> &bias, int Cout, int ntaps, int Cin,
                         int dt, ConvLayer *L) {
  const int K = ntaps * Cin;
  L->dt = dt;
  L->ntaps = ntaps;
  if (is_q8(dt)) {
    L->rows_f32 = rows_f32;
    L->bias_f32 = bias;
    std::vector<float> sw;
    std::vector<double> qsum;
    const auto elems = quantise_q8(*L, dt, nullptr, &sw, &qsum);
    if (!upload_layouts(net, elems, Cout, ntaps, Cin, dt, L)) return false;
    return put(net, L->bias, bias) && put(net, L->cscale, sw);
  }
  if (!upload_layouts(net, to_elems(rows_f32, Cout, K, dt, nullptr), Cout, ntaps, Cin, dt, L)) return false;
  return put(net, L->bias, bias);
}

// PyTorch conv weight [Cout,Cin,KH,KW] -> kernel layout; the layer must have exactly the expected shape (the kernels and
// the arena carve hard-code the architecture: a foreign file is a load error, not an out-of-bounds launch)
static bool make_conv(Net *net, const std::map<std::string, HostTensor> &m, const std::string &prefix, int stride, int Cout,
                      int Cin, int k, int dt, ConvLayer *L, std::string *err) {
  const HostTensor *w, *b;
  if (!get(m, prefix + ".weight", &w, err) || !get(m, prefix + ".bias", &b, err)) return false;
  if (!shape_is(w, {Cout, Cin, k, k}) || !shape_is(b, {Cout})) { *err = prefix + ": unexpected weight / bias shape"; return false; }
  std::vector<float> hw((size_t)Cout * k * k * Cin);
  for (int co = 0; co < Cout; co++)
    for (int ci = 0; ci < Cin; ci++)
      for (int kh = 0; kh < k; kh++)
        for (int kw = 0; kw < k; kw++)
          hw[(((size_t)co * k + kh) * k + kw) * Cin + ci] = w->data[(((size_t)co * Cin + ci) * k + kh) * k + kw];
  L->Cin = Cin; L->Cout = Cout; L->KH = k; L->KW = k; L->stride = stride; L->pad = (k - 1) / 2;
  return finish_layer(net, hw, b->data, Cout, k * k, Cin, dt, L);
}

// 7x7 stride-2 pad-3 stem on [.,160,160,6] == 4x4 stride-1 pad-2 conv on the space-to-depth input [.,80,80,32]:
// w_s2d[co][a][b][(dy*2+dx)*8 + c] = w[co][c][2a+dy-1][2b+dx-1] (zero outside the 7x7 support / for c >= 6)
static bool make_stem(Net *net, const std::map<std::string, HostTensor> &m, const std::string &prefix, int dt, ConvLayer *L,
                      std::string *err) {
  const HostTensor *w, *b;
  if (!get(m, prefix + ".weight", &w, err) || !get(m, prefix + ".bias", &b, err)) return false;
  if (!shape_is(w, {64, 6, 7, 7}) || !shape_is(b, {64})) { *err = prefix + ": expected [64,6,7,7] stem weight"; return false; }
  std::vector<float> hw((size_t)64 * 16 * 32, 0.f);
  for (int co = 0; co < 64; co++)
    for (int a = 0; a < 4; a++)
      for (int bb = 0; bb < 4; bb++)
        for (int dy = 0; dy < 2; dy++)
          for (int dx = 0; dx < 2; dx++) {
            int kh = 2 * a + dy - 1, kw = 2 * bb + dx - 1;
            if (kh < 0 || kw < 0) continue;
            for (int c = 0; c < 6; c++)
              hw[(((size_t)co * 4 + a) * 4 + bb) * 32 + (dy * 2 + dx) * 8 + c] = w->data[(((size_t)co * 6 + c) * 7 + kh) * 7 + kw];
          }
  L->Cin = 32; L->Cout = 64; L->KH = 4; L->KW = 4; L->stride = 1; L->pad = 2; L->algo_K = 7 * 7 * 6;
  return finish_layer(net, hw, b->data, 64, 16, 32, dt, L);
}

// Linear [out,in] as a 1x1 conv
static bool make_linear_conv(Net *net, const std::map<std::string, HostTensor> &m, const std::string &wname,
                             const std::string &bname, int out, int in, int dt, ConvLayer *L, std::string *err) {
  const HostTensor *w, *b;
  if (!get(m, wname, &w, err) || !get(m, bname, &b, err)) return false;
  if (!shape_is(w, {out, in}) || !shape_is(b, {out})) { *err = wname + ": unexpected Linear shape"; return false; }
  L->Cout = out; L->Cin = in; L->KH = L->KW = 1; L->stride = 1; L->pad = 0;
  return finish_layer(net, w->data, b->data, out, 1, in, dt, L);
}

static bool make_linear_f32(Net *net, const std::map<std::string, HostTensor> &m, const std::string &wname,
                            const std::string &bname, int out, int in, LinearF32 *L, std::string *err) {
  const HostTensor *w, *b;
  if (!get(m, wname, &w, err) || !get(m, bname, &b, err)) return false;
  if (!shape_is(w, {out, in}) || !shape_is(b, {out})) { *err = wname + ": unexpected Linear shape"; return false; }
  L->out = out; L->in = in;
  return put(net, L->w, w->data) && put(net, L->b, b->data);
}

static bool make_ln(Net *net, const std::map<std::string, HostTensor> &m, const std::string &prefix, LNParams *L,
                    std::string *err) {
  const HostTensor *w, *b;
  if (!get(m, prefix + ".weight", &w, err) || !get(m, prefix + ".bias", &b, err)) return false;
  if (!shape_is(w, {EMBED}) || !shape_is(b, {EMBED})) { *err = prefix + ": unexpected LayerNorm shape"; return false; }
  return put(net, L->g, w->data) && put(net, L->b, b->data);
}

static bool make_mha(Net *net, const std::map<std::string, HostTensor> &m, const std::string &prefix, int dt, MHA *a,
                     std::string *err) {
  return make_linear_conv(net, m, prefix + ".in_proj_weight", prefix + ".in_proj_bias", 3 * EMBED, EMBED, dt, &a->in_proj, err) &&
         make_linear_conv(net, m, prefix + ".out_proj.weight", prefix + ".out_proj.bias", EMBED, EMBED, dt, &a->out_proj, err) &&
         make_linear_f32(net, m, prefix + ".out_proj.weight", prefix + ".out_proj.bias", EMBED, EMBED, &a->out_proj_f32, err);
}

// What the schedule behind the trunk (plan_heads) takes for granted of a loaded network: qkv_tile_kernel and the one-launch encoder tail
// (enc_tail_kernel) read 512-wide Linear layers from their step-major copies in the token path's element type, and the refiner's read-outs
// are Linear(512, 3).  The product has no other form to fall back on (the launch chains exist in the test build only), so a network that
// does not fit fails to load, with an error that says so.  With this loader the check can never fire: make_linear_conv / make_linear_f32
// fix every shape, the heads are built in the 2-byte type `adt`, and finish_layer makes the step-major copy of every 2-byte Linear layer.
static bool check_head_layouts(const Net *net, std::string *err) {
  const int dt = net->act_dt;
  const auto lin = [&](const ConvLayer &L, int Cout) { return L.wstep && L.Cin == EMBED && L.Cout == Cout && L.dt == dt; };
  bool ok = dt == DT_F16 || dt == DT_BF16;
  if (net->scorer) {
    ok = ok && lin(net->att.in_proj, 3 * EMBED);
  } else {
    for (const EncLayer *L : {&net->trans, &net->rot})
      ok = ok && lin(L->att.in_proj, 3 * EMBED) && lin(L->att.out_proj, EMBED) && lin(L->lin1, EMBED) && lin(L->lin2, EMBED) && L->head.in == EMBED && L->head.out == 3;
  }
  if (!ok) *err = "the transformer layers do not fit qkv_tile_kernel / the one-launch encoder tail (512-wide 2-byte Linear layers with a step-major copy, Linear(512,3) read-outs): no other schedule exists in this build";
  return ok;
}

static Net *net_load_impl(const char *path, bool is_scorer, int prec, std::string *err) {
  std::map<std::string, HostTensor> m;
  if (!read_fpw(path, m, err)) return nullptr;
  std::unique_ptr<Net> net(new Net());
  net->scorer = is_scorer;
  net->prec = prec;
  net->deferred = true;   // host phase: every put() records a pending upload (net_commit makes the device copies)
  // PREC_FP8 / PREC_INT8: the 3x3 trunk convolutions from encodeA.2 on (91 % of the FLOPs) run on 8-bit operands; the stem and
  // encodeA.1 (bandwidth-bound, K = 294 / 576) and the transformer part stay in f16
  const int adt = prec == PREC_BF16 ? DT_BF16 : DT_F16;
  const int tdt = prec == PREC_FP8 ? DT_FP8 : prec == PREC_INT8 ? DT_I8 : adt;
  net->act_dt = adt;
  net->qdt = tdt;
  net->q8_blocks = is_q8(tdt) ? (g_q8_blocks & Q8_BLOCKS_ALL) : 0;
  const auto ldt = [&](int layer) { return net->q8_on(layer) ? tdt : adt; };   // a stage outside the mask keeps 2-byte weights
  bool ok = make_stem(net.get(), m, "encodeA.0", adt, &net->a0, err) && make_conv(net.get(), m, "encodeA.1", 2, 128, 64, 3, adt, &net->a1, err);
  for (int i = 0; ok && i < 2; i++)
    for (int j = 0; ok && j < 2; j++) {
      std::string cj = ".conv" + std::to_string(j + 1);
      ok = make_conv(net.get(), m, "encodeA." + std::to_string(2 + i) + cj, 1, 128, 128, 3, ldt(0), &net->ra[i][j], err) &&
           make_conv(net.get(), m, "encodeAB." + std::to_string(i) + cj, 1, 256, 256, 3, ldt(4), &net->rb[i][j], err) &&
           make_conv(net.get(), m, "encodeAB." + std::to_string(3 + i) + cj, 1, 512, 512, 3, ldt(9), &net->rc[i][j], err);
    }
  ok = ok && make_conv(net.get(), m, "encodeAB.2", 2, 512, 256, 3, ldt(8), &net->b2, err);
  if (ok && !is_scorer) {
    EncLayer *heads[2] = {&net->trans, &net->rot};
    const char *names[2] = {"trans_head", "rot_head"};
    for (int i = 0; ok && i < 2; i++) {
      std::string p0 = std::string(names[i]) + ".0", p1 = std::string(names[i]) + ".1";
      ok = make_mha(net.get(), m, p0 + ".self_attn", adt, &heads[i]->att, err) &&
           make_linear_conv(net.get(), m, p0 + ".linear1.weight", p0 + ".linear1.bias", EMBED, EMBED, adt, &heads[i]->lin1, err) &&
           make_linear_conv(net.get(), m, p0 + ".linear2.weight", p0 + ".linear2.bias", EMBED, EMBED, adt, &heads[i]->lin2, err) &&
           make_ln(net.get(), m, p0 + ".norm1", &heads[i]->ln1, err) && make_ln(net.get(), m, p0 + ".norm2", &heads[i]->ln2, err) &&
           make_linear_f32(net.get(), m, p1 + ".weight", p1 + ".bias", 3, EMBED, &heads[i]->head, err);
    }
    if (ok) {
      ok = make_grouped(net.get(), net->trans.att.in_proj, net->rot.att.in_proj, &net->g_in_proj);
#ifdef FP_TEST_HOOKS
      ok = ok && make_grouped(net.get(), net->trans.att.out_proj, net->rot.att.out_proj, &net->g_out_proj) &&
           make_grouped(net.get(), net->trans.lin1, net->rot.lin1, &net->g_lin1) && make_grouped(net.get(), net->trans.lin2, net->rot.lin2, &net->g_lin2);
#endif
      if (!ok) *err = "could not build the grouped head weights";
    }
  } else if (ok) {
    ok = make_mha(net.get(), m, "att", adt, &net->att, err) && make_mha(net.get(), m, "att_cross", adt, &net->att_cross, err) &&
         make_linear_f32(net.get(), m, "linear.weight", "linear.bias", 1, EMBED, &net->score_lin, err);
  }
  ok = ok && check_head_layouts(net.get(), err);
  if (ok) {
    // PositionalEmbedding(d_model=512, max_len=400): pe[t,2i]=sin(t*w_i), pe[t,2i+1]=cos(t*w_i), w_i=exp(-2i*ln(1e4)/512)
    std::vector<float> pe((size_t)400 * EMBED);
    for (int t = 0; t < 400; t++)
      for (int i = 0; i < EMBED / 2; i++) {
        float div = std::exp((float)(2 * i) * -(std::log(10000.0f) / (float)EMBED));
        pe[(size_t)t * EMBED + 2 * i] = std::sin((float)t * div);
        pe[(size_t)t * EMBED + 2 * i + 1] = std::cos((float)t * div);
      }
    ok = put_bytes(net.get(), net->pe, to_elems(pe, 400, EMBED, adt, nullptr));
    net->pe_host = pe;
    if (!ok) *err = "device allocation failed";
  }
  if (!ok) return nullptr;
  return net.release();
}

// Host phase of loading: the weight file is read and every device layout is built in host memory.  No HIP call, no device needed:
// callers run it OUTSIDE the process-wide exclusive section (fp_create, fp_set_precision, fp_calibrate: fp_api.hip).
Net *net_prepare(const char *path, bool is_scorer, int prec, std::string *err) {
  try {  // a malformed file must not take the process down through the C ABI
    return net_load_impl(path, is_scorer, prec, err);
  } catch (const std::exception &e) {
    *err = std::string("loading ") + path + ": " + e.what();
    return nullptr;
  }
}
// Device phase: ONE allocation (every buffer a 256-byte-aligned slice of it), ONE staged upload, the pointer fields patched.  On
// failure the network is unusable and the caller frees it.
int net_commit(Net *net, std::string *err) {
  if (!net->deferred) return 0;
  auto slice = [](const Net::Pending &q) { return (std::max<size_t>(q.bytes.size(), 1) + 255) & ~(size_t)255; };
  size_t total = 0;
  for (const Net::Pending &q : net->pending) total += slice(q);
  const size_t calib_off = total;
  total += (size_t)N_TRUNK_ACT * 512 * (sizeof(float) + sizeof(long long));
  unsigned char *arena = nullptr;
  if (hipMalloc((void **)&arena, total) != hipSuccess) { *err = "device allocation failed"; return 1; }
  net->allocs.push_back(arena);
  std::vector<unsigned char> image(total, 0);   // host image of the arena (the calibration statistics start zeroed)
  size_t off = 0;
  for (const Net::Pending &q : net->pending) {
    if (!q.bytes.empty()) std::memcpy(&image[off], q.bytes.data(), q.bytes.size());
    off += slice(q);
  }
  if (fp::memcpy_sync(arena, image.data(), total, hipMemcpyHostToDevice) != hipSuccess) { *err = "device upload failed"; return 1; }
  off = 0;
  for (Net::Pending &q : net->pending) {
    *q.slot = arena + off;
    off += slice(q);
  }
  net->calib_sum = reinterpret_cast<long long *>(arena + calib_off);
  net->calib_amax = reinterpret_cast<float *>(arena + calib_off + (size_t)N_TRUNK_ACT * 512 * sizeof(long long));
  // fields that ALIAS another field's buffer were copied while both held the placeholder: ConvLayer::wdeep = wpack (8-bit 3x3 layers)
  for (int r = Q8_FIRST_ROW; r < N_TRUNK; r++) {
    ConvLayer &l = TRUNK[r].layer(*net);
    if (is_q8(l.dt) && l.wdeep == &g_placeholder) l.wdeep = l.wpack;
  }
  net->pending.clear();
  net->pending.shrink_to_fit();
  net->deferred = false;
  return 0;
}

Net *net_load(const char *path, bool is_scorer, int prec, std::string *err) {
  Net *n = net_prepare(path, is_scorer, prec, err);
  if (n && net_commit(n, err)) { delete n; n = nullptr; }
  return n;
}

void net_free(Net *n) { delete n; }
int net_precision(const Net *n) { return n->prec; }
int net_input_dt(const Net *n) { return n->act_dt; }
bool net_q8_ready(const Net *n) { return !(n->prec == PREC_FP8 || n->prec == PREC_INT8) || n->q8_ready; }

// ---- calibration of the 8-bit networks ------------------------------------------------------------------
// Statistics: while calib_mode != 0 the trunk records, per channel of each of its 15 activations, |max| (mode 1) and the sum of
// the stored values (8-bit tensors: de-quantised) -- fp_api.hip turns the sums into means.
void net_calib_begin(Net *net, hipStream_t s, int mode, int only_act) {
  (void)hipMemsetAsync(net->calib_sum, 0, (size_t)N_TRUNK_ACT * 512 * (sizeof(float) + sizeof(long long)), s);
  net->calib_mode = mode;
  net->calib_only = only_act;
  for (int i = 0; i < N_TRUNK_ACT; i++) net->calib_count[i] = 0;
}
// sum_out: per-channel MEANS over the interior pixels of the recorded activations (sums / pixel count)
int net_calib_end(Net *net, hipStream_t s, float *amax_out /*[15][512] or null*/, float *sum_out /*[15][512]*/) {
  net->calib_mode = 0;
  net->calib_only = -1;
  if (amax_out) FP_HIP_OK(hipMemcpyAsync(amax_out, net->calib_amax, (size_t)N_TRUNK_ACT * 512 * sizeof(float), hipMemcpyDeviceToHost, s));
  std::vector<long long> sums(sum_out ? (size_t)N_TRUNK_ACT * 512 : 0);
  if (sum_out) FP_HIP_OK(hipMemcpyAsync(sums.data(), net->calib_sum, sums.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
  FP_HIP_OK(hipStreamSynchronize(s));
  if (sum_out)
    for (int a = 0; a < N_TRUNK_ACT; a++)
      for (int c = 0; c < 512; c++)
        sum_out[a * 512 + c] = net->calib_count[a] > 0 ? (float)((double)sums[a * 512 + c] * (1.0 / 1048576.0) / net->calib_count[a]) : 0.f;
  return 0;
}
void net_calib_abort(Net *net) { net->calib_mode = 0; net->calib_only = -1; }   // a calibration pass that failed half-way
void net_q8_unready(Net *net) { net->q8_ready = false; }                          // the precision's record was dropped: quantise again before use
// (8-bit layer i = 0..12 is TRUNK row i + 2: it reads activation i + 1 and writes activation i + 2)
int net_q8_bias_channels(int layer) { return trunk_layer_cout(Q8_FIRST_ROW + layer); }
bool net_q8_layer_on(const Net *n, int layer) { return n->q8_on(layer); }
int net_q8_blocks(const Net *n) { return n->q8_blocks; }

// One 8-bit layer: (weights) quantise its rows with the input-channel scales s_in folded in and upload every layout; then the epilogue
// tables.  accumulator -> real value: acc * sw (+ DT_I8: 128 * sw * sum_k q, the offset of the unsigned activations) + bias + fix;
// s_out_fold != null (the output is 8-bit ONLY): the consumer's inverse scales multiply both (legal: no residual, ReLU).
static int apply_q8_layer(Net *net, ConvLayer &l, int dt, const float *s_in, const float *bias_fix, const float *s_out_fold, bool weights,
                          const float *m_int = nullptr, int J = 0) {
  const int Cout = l.Cout;
  if (weights) {
    std::vector<float> sw;
    std::vector<double> qsum;
    std::vector<float> tmat;
    const auto elems = quantise_q8(l, dt, s_in, &sw, &qsum, dt == DT_I8 ? m_int : nullptr, J, dt == DT_I8 ? &tmat : nullptr);
    if (dt == DT_I8 && !put(net, l.tmat_t, tmat)) { set_error("net_apply_q8: device upload failed"); return 1; }
    if (!upload_layouts(net, elems, Cout, l.ntaps, l.Cin, dt, &l)) { set_error("net_apply_q8: device upload failed"); return 1; }
    l.q_sw = sw; l.q_sum = qsum;
  }
  std::vector<float> cs(Cout), bs(Cout);
  for (int co = 0; co < Cout; co++) {
    double b = (double)l.bias_f32[co] + (bias_fix ? bias_fix[co] : 0.f);
    if (dt == DT_I8) b += 128.0 * l.q_sw[co] * l.q_sum[co];
    double c = l.q_sw[co];
    if (s_out_fold) { const double inv = 1.0 / s_out_fold[co]; b *= inv; c *= inv; }
    cs[co] = (float)c; bs[co] = (float)b;
  }
  if (!put(net, l.cscale, cs) || !put(net, l.bias, bs)) { set_error("net_apply_q8: device upload failed"); return 1; }
  return 0;
}

// Applies a calibration to an 8-bit network: amax [15][512] = per-channel |max| of the trunk activations of the f16 network on
// the calibration frame; bias_fix [13][512] (may be null = zeros) and tok_fix [512] (may be null) = the solved bias correction.
// weights = false: only the biases / the positional table are rebuilt (the correction sweeps).
//   scale of activation a, channel c:  FP8: amax / 224 (one binade of headroom below the e4m3 maximum 448)
//                                      I8 : amax * 1.25 / 255 (unsigned 8-bit: every tensor here is a ReLU output)
//   (amax floored at 1/1024 of the tensor's largest channel)
//   the concat tensor (activation 5) gets the SAME scale for channel c of its a-half and its b-half, so that its producer (128
//   output channels, two image groups) indexes one table.
// frame_means [n_frames][15][512] (weights = true only; null / 0 = round to nearest): per-channel means of the f16 network's trunk
// activations in each calibration frame -- what the INT8 weights' error-feedback rounding cancels against (quantise_q8).
int net_apply_q8(Net *net, const float *amax, const float *bias_fix, const float *tok_fix, bool weights, const float *frame_means, int n_frames) {
  FP_CHECK(net->prec == PREC_FP8 || net->prec == PREC_INT8, "net_apply_q8: not an 8-bit network");
  const int dt = net->qdt;
  ConvLayer *L[13];   // the 8-bit layers in trunk order
  for (int i = 0; i < 13; i++) L[i] = &TRUNK[Q8_FIRST_ROW + i].layer(*net);
  if (weights) {
    for (int a = 1; a <= 13; a++) {
      const int C = TRUNK[a].C;
      std::vector<float> sc(C);
      // a channel that is (almost) dead on the calibration frame gets the floor tensor-|max| / 1024, NOT a scale of 1: the scales are
      // folded into the consumer's weights, and one large scale would take the whole range of every weight row
      float tmax = 0.f;
      for (int c = 0; c < C; c++) tmax = std::max(tmax, amax[a * 512 + c]);
      if (!(tmax > 0.f)) tmax = 1.f;
      for (int c = 0; c < C; c++) {
        float m = amax[a * 512 + c];
        if (a == 5) m = std::max(amax[a * 512 + (c & 127)], amax[a * 512 + (c & 127) + 128]);
        m = std::max(m, tmax * (1.f / 1024.f));
        sc[c] = dt == DT_FP8 ? m / 224.f : m * g_q8_headroom / 255.f;
      }
      net->act_scale[a] = sc;
      std::vector<float> inv(C);
      for (int c = 0; c < C; c++) inv[c] = 1.f / sc[c];
      if (!put(net, net->act_oinv[a], inv) || !put(net, net->act_scale_dev[a], sc)) { set_error("net_apply_q8: device upload failed"); return 1; }
    }
  }
  FP_CHECK(!net->act_scale[1].empty(), "net_apply_q8: bias update before the scales were set");
  if (weights) net->q8_img_comp = dt == DT_I8 && frame_means != nullptr && n_frames > 0;
  for (int i = 0; i < 13; i++) {
    ConvLayer &l = *L[i];
    const int Cout = l.Cout;
    if (bias_fix) net->bias_fix[i].assign(bias_fix + (size_t)i * 512, bias_fix + (size_t)i * 512 + Cout);
    else if (net->bias_fix[i].empty()) net->bias_fix[i].assign(Cout, 0.f);
  }
  std::vector<float> m_int;
  for (int i = 0; i < 13; i++) {
    const int a = i + 1, Cin = L[i]->Cin;   // layer i reads activation i + 1
    if (!net->q8_on(i)) continue;           // [r6] a 2-byte layer of a partly 8-bit trunk: nothing to quantise
    const bool efr = weights && dt == DT_I8 && frame_means && n_frames > 0 && g_q8_efr;
    if (efr) {   // mean integer activation of every input channel per frame: f16 mean / scale
      m_int.assign((size_t)n_frames * Cin, 0.f);
      for (int j = 0; j < n_frames; j++)
        for (int c = 0; c < Cin; c++) m_int[(size_t)j * Cin + c] = frame_means[((size_t)j * N_TRUNK_ACT + a) * 512 + c] / net->act_scale[a][c];
    }
    if (apply_q8_layer(net, *L[i], dt, net->act_scale[i + 1].data(), net->bias_fix[i].data(),
                       trunk_folded_out(Q8_FIRST_ROW + i) ? net->act_scale[i + 2].data() : nullptr, weights, efr ? m_int.data() : nullptr, efr ? n_frames : 0)) return 1;
  }
  if (tok_fix) net->tok_fix.assign(tok_fix, tok_fix + EMBED);
  else if (net->tok_fix.empty()) net->tok_fix.assign(EMBED, 0.f);
  {  // positional table + token correction (the trunk's last epilogue adds the table to the rounded token)
    std::vector<float> pe(net->pe_host);
    for (int t = 0; t < 400; t++)
      for (int c = 0; c < EMBED; c++) pe[(size_t)t * EMBED + c] += net->tok_fix[c];
    const auto e = to_elems(pe, 400, EMBED, net->act_dt, nullptr);
    if (fp::memcpy_sync(net->pe, e.data(), e.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("net_apply_q8: device upload failed"); return 1; }
  }
  net->q8_ready = true;
  return 0;
}
// Output-layer correction of an 8-bit network: fix (refiner: [trans 3 | rot 3], scorer: [512] on the pooled score feature) is added to
// the biases of the f32 output layers (Linear(512,3) x 2 / att.out_proj) -- the last stage of the calibration's bias correction.
int net_q8_set_out_fix(Net *net, const float *fix) {
  const int n = net->scorer ? EMBED : 6;
  if (net->out_bias0.empty()) {
    net->out_bias0.resize(n);
    if (net->scorer) FP_HIP_OK(fp::memcpy_sync(net->out_bias0.data(), net->att.out_proj_f32.b, EMBED * 4, hipMemcpyDeviceToHost));
    else {
      FP_HIP_OK(fp::memcpy_sync(net->out_bias0.data(), net->trans.head.b, 12, hipMemcpyDeviceToHost));
      FP_HIP_OK(fp::memcpy_sync(net->out_bias0.data() + 3, net->rot.head.b, 12, hipMemcpyDeviceToHost));
    }
  }
  net->out_fix.assign(fix, fix + n);
  std::vector<float> b(n);
  for (int i = 0; i < n; i++) b[i] = net->out_bias0[i] + fix[i];
  if (net->scorer) FP_HIP_OK(fp::memcpy_sync(net->att.out_proj_f32.b, b.data(), EMBED * 4, hipMemcpyHostToDevice));
  else {
    FP_HIP_OK(fp::memcpy_sync(net->trans.head.b, b.data(), 12, hipMemcpyHostToDevice));
    FP_HIP_OK(fp::memcpy_sync(net->rot.head.b, b.data() + 3, 12, hipMemcpyHostToDevice));
  }
  return 0;
}
void net_q8_get_fix(const Net *net, float *bias_fix /*[13][512]*/, float *tok_fix /*[512]*/) {
  std::memset(bias_fix, 0, sizeof(float) * 13 * 512);
  std::memset(tok_fix, 0, sizeof(float) * 512);
  for (int i = 0; i < 13; i++)
    for (size_t c = 0; c < net->bias_fix[i].size(); c++) bias_fix[(size_t)i * 512 + c] = net->bias_fix[i][c];
  for (size_t c = 0; c < net->tok_fix.size(); c++) tok_fix[c] = net->tok_fix[c];
}

// =================================================================================================
// scratch
// =================================================================================================

struct NNScratch {
  int cap = 0;
  int q8 = 0;       // 0: 2-byte network; DT_FP8 / DT_I8: the arena also carries 1-byte slots for the 8-bit operand copies, whose zero
                    // border is the byte 0x00 (FP8) / 0x80 (I8: unsigned 0 stored with the offset of -128)
  unsigned char *buf = nullptr;
  float *f32 = nullptr;
  // cross-attention head over all gathered hypotheses (sized by n_total, independent of the local shard)
  int head_cap = 0;
  unsigned char *head_buf = nullptr;
  float *head_f32 = nullptr;
  // fp32 partial slabs of split-K convolutions (small batches); per model so that models on different streams /
  // threads never share it
  float *splitk = nullptr;
  size_t splitk_cap = 0;
  int *img_sum = nullptr;      // INT8 networks: [2 * cap][512] per-image channel sums (integer atomics; zero between uses) ...
  float *img_bias = nullptr;   // ... and the per-image bias made from them (q8_img_*_kernel)
  ~NNScratch() {
    if (img_sum) (void)hipFree(img_sum);
    if (img_bias) (void)hipFree(img_bias);
    if (splitk) (void)hipFree(splitk);
    if (buf) (void)hipFree(buf);
    if (f32) (void)hipFree(f32);
    if (head_buf) (void)hipFree(head_buf);
    if (head_f32) (void)hipFree(head_f32);
  }
};
NNScratch *nn_scratch_create(int prec) {
  NNScratch *w = new NNScratch();
  w->q8 = prec == PREC_FP8 ? DT_FP8 : prec == PREC_INT8 ? DT_I8 : 0;
  return w;
}

void nn_scratch_free(NNScratch *w) { delete w; }

// per-hypothesis activation sizes (BYTES at 2 bytes per element: one arena layout for every precision; an FP8 tensor uses
// the first half of its slot); conv inputs carry their physical zero border.  A scratch object serves ONE precision:
// the border positions of a tensor depend on its element size.
static constexpr size_t SZ_STEM = 2ull * 82 * 82 * 64 * 2;   // stem out, read by the 3x3/s2 conv (border 1)
static constexpr size_t SZ_128 = 2ull * 42 * 42 * 128 * 2;
static constexpr size_t SZ_256 = 42ull * 42 * 256 * 2;
static constexpr size_t SZ_512 = 22ull * 22 * 512 * 2;
static constexpr size_t SZ_TOK = 400ull * 512 * 2;            // token buffers (no border)
static constexpr size_t SZ_QKV = 400ull * 1536 * 2;
static constexpr size_t PER_HYP = SZ_STEM + 3 * SZ_128 + 3 * SZ_256 + 3 * SZ_512 + SZ_QKV + 4 * SZ_TOK;
static constexpr size_t PER_HYP_Q8 = (3 * SZ_128 + 3 * SZ_256 + 3 * SZ_512) / 2;   // the 1-byte copies (8-bit networks only)
static size_t per_hyp_bytes(const NNScratch *w) { return PER_HYP + (w->q8 ? PER_HYP_Q8 : 0); }
void nn_scratch_debug_info(const NNScratch *w, const void **buf, size_t *bytes, const void **f32, size_t *f32_bytes) {
  *buf = w->buf; *bytes = (size_t)w->cap * per_hyp_bytes(w);
  *f32 = w->f32; *f32_bytes = (size_t)w->cap * EMBED * sizeof(float);
}

// f32 side buffer: [cap][512] pooled features and, in the test build, the [2][LN_PMEAN_PARTS][512] partial column sums of
// layernorm_pmean_kernel (Track's launch chain cuts a 400-token sequence into LN_PMEAN_PARTS runs of LN_PMEAN_ROWS rows)
static constexpr int LN_PMEAN_PARTS = 16, LN_PMEAN_ROWS = 25;
#ifdef FP_TEST_HOOKS
static constexpr size_t F32_PSUMS = (size_t)2 * LN_PMEAN_PARTS * EMBED;
static float *pmean_sums(const NNScratch *ws) { return ws->f32 + (size_t)ws->cap * EMBED; }
#else
static constexpr size_t F32_PSUMS = 0;
#endif

static int ensure_scratch(NNScratch *ws, int N, hipStream_t s) {
  if (N <= ws->cap) return 0;
  if (ws->buf) (void)hipFree(ws->buf);
  if (ws->f32) (void)hipFree(ws->f32);
  ws->buf = nullptr; ws->f32 = nullptr; ws->cap = 0;
  int cap = std::max(N, 8);
  g_alloc_epoch++;
  FP_HIP_OK(hipMalloc((void **)&ws->buf, (size_t)cap * per_hyp_bytes(ws)));
  FP_HIP_OK(hipMalloc((void **)&ws->f32, ((size_t)cap * EMBED + F32_PSUMS) * sizeof(float)));
  // the zero borders are written here once and never again: every producer stores interiors only, and the arena is
  // carved by CAPACITY (not by the current N), so an image slot's border never moves
  FP_HIP_OK(hipMemsetAsync(ws->buf, 0, (size_t)cap * PER_HYP, s));
  if (ws->q8) FP_HIP_OK(hipMemsetAsync(ws->buf + (size_t)cap * PER_HYP, ws->q8 == DT_I8 ? 0x80 : 0, (size_t)cap * PER_HYP_Q8, s));
  if (ws->q8 == DT_I8) {
    if (ws->img_sum) (void)hipFree(ws->img_sum);
    if (ws->img_bias) (void)hipFree(ws->img_bias);
    ws->img_sum = nullptr; ws->img_bias = nullptr;
    FP_HIP_OK(hipMalloc((void **)&ws->img_sum, (size_t)2 * cap * 512 * sizeof(int)));
    FP_HIP_OK(hipMemsetAsync(ws->img_sum, 0, (size_t)2 * cap * 512 * sizeof(int), s));
    FP_HIP_OK(hipMalloc((void **)&ws->img_bias, (size_t)2 * cap * 512 * sizeof(float)));
  }
  ws->cap = cap;
  return 0;
}

static int ensure_head_scratch(NNScratch *ws, int n_total) {
  if (n_total <= ws->head_cap) return 0;
  if (ws->head_buf) (void)hipFree(ws->head_buf);
  if (ws->head_f32) (void)hipFree(ws->head_f32);
  ws->head_buf = nullptr; ws->head_f32 = nullptr; ws->head_cap = 0;
  int cap = std::max(n_total, 256);
  g_alloc_epoch++;
  FP_HIP_OK(hipMalloc((void **)&ws->head_buf, (size_t)cap * 5 * EMBED * 2));
  FP_HIP_OK(hipMalloc((void **)&ws->head_f32, (size_t)cap * EMBED * sizeof(float)));
  ws->head_cap = cap;
  return 0;
}

// =================================================================================================
// launch helpers
// =================================================================================================

struct Ctx {
  hipStream_t s;
  Profiler *prof;
  const Net *net;
  NNScratch *ws = nullptr;  // owner of the split-K slab (null only in the single-threaded test hooks)
};

// A/B and ablation switches exist only in the test build (libfoundationpose_amd_test.so, -DFP_TEST_HOOKS); in the product
// they are compile-time constants, so nothing can flip a schedule under a running model.  (A kernel that only a switch reaches is
// kept out of the product by #ifdef FP_TEST_HOOKS around its launch: a constant condition alone still instantiates it.)
#ifdef FP_TEST_HOOKS
#define FP_HOOK static int
static unsigned long long *g_clk_probe = nullptr;
static NNScratch g_hook_ws;  // split-K slab of the fpt_* test hooks
#else
#define FP_HOOK [[maybe_unused]] static constexpr int
static constexpr unsigned long long *g_clk_probe = nullptr;
#endif
FP_HOOK g_conv_variant = 0;    // 0 default; 7 force / 8 disable the resident-halo kernels; 3 = 256x128 ping-pong everywhere; 5 = 256x256 rounds without
                               // the halo kernels
FP_HOOK g_conv_ablate = 0;     // timing-only ablations (wrong results) of conv_big_pp_kernel / conv_halo_kernel
FP_HOOK g_splitk_ablate = 0;   // test build, wrong results: conv_splitk_reduce_kernel sums all slices but the last (the float64 checks must fail)
FP_HOOK g_i8_stream = 0;       // test build A/B: 1 = INT8 networks with an 8-bit residual stream (plan_trunk: i8_stream; faster, but its common-mode error is frame-specific: DESIGN.md section 4.4)
FP_HOOK g_conv_ragged = 1;     // 256x256 rounds with 288-row tiles that absorb the left-over rows (plan_conv); 0 = a separate left-over launch, as before them
FP_HOOK g_smallm = 1;          // small problems (Track, a few objects) on conv_smallx_kernel: K split over the waves of a workgroup, no split-K slabs / reduce launch
                               // (0 = off, 2 = for every size, 3 = its first version, conv_smallm_kernel)
// the five switches of the schedule behind the trunk: read by heads_override() alone, decided on by plan_heads alone (HeadsOverride)
FP_HOOK g_enc_tail = 1;        // [r5] out_proj + LayerNorm 1 + FFN + LayerNorm 2 + token sums of BOTH refiner heads as one launch (enc_tail_kernel); 0 = the launch
                               // chains (test build only: the float64-tapped reference)
FP_HOOK g_ln_pmean = 1;        // [r5] Track's launch chain: LayerNorm 2 + partial token sums in one launch (layernorm_pmean_kernel) instead of layernorm + token_mean
FP_HOOK g_fuse_pose = 1;       // Track: 1 = the read-out kernel applies RefinePostProcess too (one launch less), 0 = the caller launches pose_update
FP_HOOK g_qkv_ablate = 0;      // timing-only ablations of qkv_tile_kernel (test build, wrong results)
FP_HOOK g_att_variant = 1;     // a row of ATT_VARIANTS: 1 = attention32_kernel / attention32_skv_kernel as shipped, 8 = without the XCD remap, 16.. = timing ablations

// Thresholds of the convolution schedule (plan_conv).  They were A/B switches until their experiments settled (EXPERIMENTS.md).
static constexpr int SPLITK_TARGET = 128;   // workgroups a split-K launch aims for (96-128 best, 256 is 6 % slower)
static constexpr int SPLITK_MIN_KT = 9;     // layers with fewer 128-byte K-steps never split
static constexpr int SMALL_DEEP_MAXKT = 18; // small problems (Track): conv_deep_kernel<64> over ALL K-steps instead of split-K + reduce when K has at most this many 128-byte steps
static constexpr int SMALLM_MAXKT = 80;     // the small-problem kernel takes layers with fewer 128-byte K-steps than this: every layer of both networks (72 for conv_512); 40 was the limit of its first version
static constexpr int SMALLM_MAXT16 = 1024;  // ... and with at most this many 16-pixel x 64-channel tiles (the grouped QKV of Track has 1200)
// Settled the other way, and therefore not in the schedule: split-K for left-over rows (measured -0.1 ms per Register, but a row's fp32
// summation order would then depend on where it falls in the batch, and sharded and unsharded Register must pick the same near-tied
// winner); the left-over rows on a side stream next to the 256x256 rounds (measured SLOWER, Register 10.85 -> 11.20 ms: a deep-ring
// workgroup needs a whole CU, 147 KB of LDS, so it waits for a 256x256 tile to finish, then holds that CU out of the next round: the
// rounds lose their lock-step and end in a tail longer than the 35 us the lone launch took); conv_big_pp_kernel's epilogue stores staged
// through LDS (measured [r3] conv_512 3.205 -> 3.227 / 3.184 -> 3.180 ms, i.e. nothing -- the 256x256 tile's store burst is not bound by
// the store shape, unlike gemm_k32_kernel's, -6 %); the 16-row tail of a 400-token sequence on attention32_skv_kernel (attention 0.555 ->
// 0.625 ms per Register); 3x3 / 40x40 weights global -> registers (conv_256 -3 % in the stage profile, nothing on the wall clock).

// =================================================================================================
// the convolution / Linear schedule
// =================================================================================================
// plan_conv decides which kernels run a layer, over which rows, with how many split-K slices and whether the positional table is
// fused; run_conv executes the steps.  The plan is plain host arithmetic on the problem's shape: it can be asked without a GPU
// (fpt_plan_conv, tests/test_conv_plan_cpu.py).

enum ConvKernel {
  CK_SMALLX, CK_SMALLM, CK_STEM_HALO, CK_GEMM_K32, CK_S2_HALO, CK_HALO, CK_HALO8, CK_PP32, CK_BIG_PP, CK_PP, CK_DEEP64, CK_DEEP128,
  CK_IGEMM128, CK_IGEMM64, CK_SPLITK_REDUCE
};

struct ConvProblem {
  int Cin = 0, Cout = 0, KH = 0, KW = 0, stride = 1, pad = 0, algo_K = 0;   // the layer (ConvLayer)
  bool wfrag = false, wpack = false;   // the layer carries the fragment-order / gemm_k32_kernel's stage-order copy of its weights
  int NB = 0, H = 0, W = 0, ipad = 0;  // input [NB, H + 2 * ipad, W + 2 * ipad, Cin]
  int dt = DT_F16, odt = DT_F16;       // element type of the operands / of the output (DT_DUAL_*, DT_QS_* ... included)
  bool has_res = false;
  int split_imgs = 0;
  int grp_rows = 0;                    // rows per weight group (ConvGroup), 0 = none
  bool post = false;                   // a positional table is offered (ConvParams::post)
  int conv_variant = 0, conv_ablate = 0, smallm = 1;   // the test build's switches (g_conv_variant, g_conv_ablate, g_smallm)
  int ragged = 1;                      // ... (g_conv_ragged)
};

struct ConvStep {
  int kernel = 0;               // ConvKernel
  const char *name = "";        // as the profiler and the launch log name it
  int mi = 0, ni = 0;           // conv_smallx_kernel / conv_smallm_kernel: <MI, NI>
  bool post = false;            // the POST instantiation (the reduce: ConvParams::post): the step adds the positional table
  bool deep = false;            // conv_smallm_kernel: DEEP
  bool wpack = false;           // gemm_k32_kernel: WPACK
  int ablate = 0;               // test build: the timing-only ablation instantiated (0 = the real kernel)
  int m_begin = 0, M = 0;       // output rows [m_begin, M)
  int n_tall = 0;               // conv_big_pp_kernel: row tiles of the grid that are 288 rows tall (the ragged rounds), 0 = all 256
  int ksplit = 1, kt_per = 0;   // split-K slices and 128-byte K-steps per slice
  unsigned grid = 0;
  int block = 256, lds = 0;     // threads per workgroup, dynamic LDS bytes
  double flops = 0, bytes = 0;  // the step's share of the layer (profiler)
};

struct ConvPlan {
  static constexpr int MAX_STEPS = 4;   // pp32 rounds -> 256x256 rounds -> ping-pong rounds -> deep-ring left-over; or a split-K launch + its reduce
  int n = 0;
  ConvStep step[MAX_STEPS];
  bool post_fused = false;      // every output row got the positional table (otherwise none did, and the caller adds it)
};

// output size of a layer on an H x W input
static void conv_out_hw(int KH, int KW, int stride, int pad, int H, int W, int *OH, int *OW) {
  *OH = (H + 2 * pad - KH) / stride + 1;
  *OW = (W + 2 * pad - KW) / stride + 1;
  if (KH == 4 && pad == 2 && stride == 1) { *OH = H; *OW = W; }  // s2d stem: asymmetric padding (2 before, 1 after)
}

static int plan_conv(const ConvProblem &q, ConvPlan *plan) {
  *plan = ConvPlan{};
  const bool B2 = !is_q8(q.dt);            // 2-byte element type: the 64-byte-row kernels exist
  const bool SAME = q.dt == q.odt;         // kernels without an ODT parameter write their operand type
  const bool QOUT = odt_q(q.odt) >= 0;     // an 8-bit tensor is written (alone or next to the f16 stream tensor): no POST instantiation
  const bool grp = q.grp_rows > 0;
  int OH, OW;
  conv_out_hw(q.KH, q.KW, q.stride, q.pad, q.H, q.W, &OH, &OW);
  const int M = q.NB * OH * OW, Ktot = q.KH * q.KW * q.Cin, Cout = q.Cout;
  const int cin_b = q.Cin * elem_bytes(q.dt), KT = Ktot * elem_bytes(q.dt) / 128;
  double flops = 2.0 * (double)M * Cout * (q.algo_K > 0 ? q.algo_K : Ktot);
  double bytes = ((double)q.NB * q.H * q.W * q.Cin + (double)M * Cout * (q.has_res ? 2 : 1) + (double)Cout * Ktot) * elem_bytes(q.dt);
  constexpr int LDS_IG128 = 2 * (128 * 128 + 128 * 128), LDS_IG64 = 2 * (128 * 128 + 64 * 128);
  constexpr int LDS3_128 = 3 * (256 * 128 + 128 * 128);
  constexpr int LDS_BIG = 2 * (256 * 128 + 256 * 128);
  constexpr int LDS_BIG_TALL = 2 * (288 * 128 + 256 * 128);
  constexpr int LDS_HALO40 = ((10 * 42 + 7) / 8) * 1024 + 3 * 128 * 64;
  constexpr int LDS_HALO8 = ((10 * 42 + 7) / 8) * 1024 + 128 * 128;
  constexpr int LDS_STEM_HALO = ((11 * 84 + 15) / 16) * 1024 + 3 * 64 * 64;
  constexpr int LDS_DEEP64 = 6 * (64 + 128) * 128, LDS_DEEP128 = 4 * (128 + 128) * 128;
  constexpr int LDS_GEMM_K32 = 3 * (128 + 256) * 64;
  constexpr int LDS_S2_HALO = ((9 * 41 + 7) / 8) * 1024 + 3 * 128 * 64;
  constexpr int LDS_PP32 = 4 * (512 + 128) * 64;
  int m_begin = 0, ksplit = 1, kt_per = KT;
  // a step over rows [m_begin, m_end) that takes the share `frac` of what is left of the layer's flops and bytes
  bool overflow = false;
  const auto add = [&](int kernel, const char *name, int m_end, int grid, int block, int lds, double frac = 1.0) -> ConvStep & {
    overflow = overflow || plan->n == ConvPlan::MAX_STEPS;
    ConvStep &st = plan->step[overflow ? ConvPlan::MAX_STEPS - 1 : plan->n++];
    st = ConvStep{};
    st.kernel = kernel; st.name = name;
    st.m_begin = m_begin; st.M = m_end; st.ksplit = ksplit; st.kt_per = kt_per;
    st.grid = (unsigned)grid; st.block = block; st.lds = lds;
    st.flops = flops * frac; st.bytes = bytes * frac;
    flops *= (1.0 - frac); bytes *= (1.0 - frac);
    return st;
  };
  const auto finish = [&]() {
    FP_CHECK(!overflow, "plan_conv: more steps than ConvPlan holds");
    return 0;
  };

  // ---- small problems: one launch per layer, the K-steps split over the four waves of a workgroup (conv_smallx_kernel)
  if (B2 || Cout % 128 == 0) {                            // (FP8 layers all have Cout % 128 == 0: 64-channel tiles only)
    const int cw = (Cout % 128 == 0) ? 64 : 32;           // channels per workgroup = the block of the host-side row permutation
    const int t16 = ((M + 15) / 16) * (Cout / cw);
    // Measured on Track (tools/profile_track.sh, profiles/r03g_track_timeline.txt): 5.6-7.2 us for the layers of up to 18 K-steps, 8.5-9.1
    // for the 36-step ones, 10.2-10.6 for conv_512 (72 steps; 12.8 + 5.5 us as split-K + reduce).  The first version
    // (conv_smallm_kernel: both operands global -> registers in MFMA-operand shape, 64 clocks of the vector L1 per instruction) lost on
    // the long-K layers (21 us); smallm = 3 selects it for A/B (2-byte types), smallm = 2 forces the small-problem kernel for every size.
    if (q.smallm && q.wfrag && (KT < SMALLM_MAXKT || q.smallm >= 2) && q.conv_variant == 0 && q.conv_ablate == 0 && Cout % cw == 0 &&
        t16 <= SMALLM_MAXT16 * (64 / cw) && (!grp || q.grp_rows % 32 == 0) && ((Cout / cw) % 8 == 0 || 8 % (Cout / cw) == 0)) {
      const int t32 = ((M + 31) / 32) * (Cout / cw);
      const bool two = t32 >= 160;                        // 32-pixel tiles halve the weight stream once they still fill the chip
      // grid = 8 XCD lanes x ceil(workgroups / 8), see the kernel's placement rule
      const int ntl = Cout / cw, mtl = two ? (M + 31) / 32 : (M + 15) / 16;
      const int per_xcd = ntl >= 8 ? mtl * (ntl / 8) : (mtl + 8 / ntl - 1) / (8 / ntl);
      const int mi = two ? 2 : 1, ni = cw == 64 ? 4 : 2;
      const bool first = q.smallm == 3 && B2;
      ConvStep &st = add(first ? CK_SMALLM : CK_SMALLX, "conv_smallm_kernel", M, 8 * per_xcd, 256,
                         first ? 3 * ni * mi * 1024 : 4 * (mi == 1 ? 4 : 3) * mi * 2048 + 3 * ni * mi * 1024);
      st.mi = mi; st.ni = ni;
      st.deep = KT >= 32;                                 // every wave has >= 8 K-steps >= 2 * PF (PF = 4 / 3)
      st.post = q.post && !QOUT && cw == 64;              // (no 32-channel layer carries a positional table)
      plan->post_fused = st.post;
      return finish();
    }
  }
  const bool small_deep = !grp && KT >= 4 && KT <= SMALL_DEEP_MAXKT && Cout % 128 == 0 && ((M + 63) / 64) * (Cout / 128) >= 40 &&
                          ((M + 63) / 64) * (Cout / 128) <= 256;
  // split-K for small problems (Track, N <= ~8): a 128x128 tile count far below the 512 workgroup slots of the chip
  // would leave most CUs idle while a few walk up to 72 K-steps; give every CU a slice instead (2-byte types only)
  if (!small_deep && KT >= SPLITK_MIN_KT && B2) {
    const int tiles = ((M + 127) / 128) * (Cout % 128 == 0 ? Cout / 128 : Cout / 64);
    // a little above the split-K range (a batch of ~8 objects): long-K layers still leave half the chip idle for 72 K-steps;
    // two slices per tile while the grid fits one round of the 256 CUs
    const int target = tiles <= 96 ? SPLITK_TARGET : (tiles <= 128 && KT >= 36) ? 2 * tiles : 0;
    const int S = std::min(std::max(target / tiles, 1), KT / 2);
    if (target && S > 1) {
      kt_per = (KT + S - 1) / S;
      ksplit = (KT + kt_per - 1) / kt_per;
    }
  }
  const bool halo_ok = q.conv_variant == 0 || q.conv_variant == 7;
  const bool force = q.conv_variant == 7;
  if (B2 && SAME && !grp && halo_ok && q.Cin == 32 && q.KH == 4 && q.KW == 4 && Cout == 64 && q.ipad == 2 && q.W == 80 && q.H == 80 && ksplit == 1 &&
      !q.has_res && q.split_imgs == 0 && (force || q.NB * 10 >= 300)) {
    add(CK_STEM_HALO, "conv_stem_halo_kernel", M, q.NB * 10, 256, LDS_STEM_HALO);
    return finish();
  }
  if (B2 && SAME && !grp && q.conv_variant == 0 && q.KH == 1 && q.KW == 1 && q.stride == 1 && q.pad == 0 && q.ipad == 0 && Cout % 256 == 0 &&
      Ktot % 32 == 0 && ksplit == 1 && q.split_imgs == 0 && ((M + 127) / 128) * (Cout / 256) >= 512) {
    add(CK_GEMM_K32, "gemm_k32_kernel", M, ((M + 127) / 128) * (Cout / 256), 256, LDS_GEMM_K32).wpack = q.wpack;
    return finish();
  }
  if (B2 && !grp && halo_ok && q.KH == 3 && q.KW == 3 && q.stride == 2 && q.pad == 1 && q.ipad == 1 && q.W == 80 && q.H == 80 && q.Cin == 64 &&
      Cout == 128 && ksplit == 1 && !q.has_res && q.split_imgs == 0 && (force || q.NB * 10 >= 300)) {
    add(CK_S2_HALO, "conv_s2_halo_kernel", M, q.NB * 10, 256, LDS_S2_HALO);
    return finish();
  }
  // 3x3 / stride 1 on 40x40 maps with the input tile resident in LDS; measured crossover vs the implicit-GEMM tiles: ~32 hypotheses
  // (conv_halo_kernel writes its operand type, conv_halo8_kernel the 8-bit type of its operands, alone or next to the f16 stream)
  if ((B2 ? SAME : odt_q(q.odt) == q.dt) && !grp && halo_ok && q.KH == 3 && q.KW == 3 && q.stride == 1 && q.pad == 1 && q.ipad == 1 && q.W == 40 &&
      q.H % 8 == 0 && cin_b % 128 == 0 && Cout % 128 == 0 && ksplit == 1 && (force || q.NB * (q.H / 8) * (Cout / 128) >= 300)) {
    const int grid = q.NB * (q.H / 8) * (Cout / 128);
    if (B2) {
      const int a = q.conv_ablate;
      add(CK_HALO, "conv_halo_kernel", M, grid, 256, LDS_HALO40).ablate = (q.dt == DT_F16 && (a == 1 || a == 2 || a == 8 || a == 16 || a == 32)) ? a : 0;
    } else {
      add(CK_HALO8, "conv_halo8_kernel", M, grid, 256, LDS_HALO8);
    }
    return finish();
  }
  if (B2 && !grp && (q.conv_variant == 0 || q.conv_variant == 8) && Cout == 128 && ksplit == 1 && KT >= 4 && KT <= 80) {
    // 512x128 ping-pong tiles (conv_pp32_kernel) for as many FULL rounds of the 256 CUs as the problem has; the remaining
    // rows go to the kernels below
    const int mt_big = (M / 512 / 256) * 256;
    if (mt_big > 0) {
      add(CK_PP32, "conv_pp32_kernel<512,128>", mt_big * 512, mt_big, 512, LDS_PP32, (double)(mt_big * 512) / (double)M);
      m_begin = mt_big * 512;
      if (m_begin >= M) return finish();
    }
  }
  bool post_main = false;  // the positional table is added by the 256x256 rounds + deep-ring left-over
  // (encodeA.1 has 128 output channels: no 256-wide instantiation of the f16 -> 8-bit boundary)
  if (!(q.dt == DT_F16 && QOUT) && !grp && (q.conv_variant == 5 || q.conv_variant == 0 || q.conv_variant == 8) && Cout % 256 == 0 && ksplit == 1 && KT >= 2) {
    // 256x256 tiles for as many FULL rounds of the 256 CUs as the problem has, the remaining rows on smaller tiles
    const int nt2 = Cout / 256;
    const int mt_all = M / 256;                           // whole 256-row m-tiles
    const int mt_big = (mt_all * nt2 / 256) * 256 / nt2;  // m-tiles covered by full rounds
    const int rows_left = M - mt_big * 256;
    // the positional table is fused only when every row takes a schedule that implements it: the 256x256 rounds + the deep-ring
    // kernel for the left-over (N = 252); otherwise nobody adds it here and the caller launches add_pos_embed_kernel
    post_main = q.post && !QOUT && mt_big > 0 && q.conv_variant == 0 && q.conv_ablate == 0 && KT >= 16 &&
                (rows_left == 0 || ((rows_left + 63) / 64) * (Cout / 128) <= 256);
    // Ragged rounds: a left-over of at most one 32-row slice per first-round workgroup is absorbed by the rounds themselves -- n_tall of
    // their row tiles are 288 rows tall, all dispatched in the first round (conv_big_pp_kernel) -- instead of a deep-ring launch of its
    // own on an otherwise idle chip.  Every row keeps its K order, so the outputs are the same bits.  Not with the positional table
    // offered (that schedule, rounds + deep ring both adding the table, stays as it is), not for the 8-bit types (no tall body), and
    // only where the tile -> row map of the kernel holds: whole rounds, a channel-tile count that divides an XCD's share of a round.
    const int n_tall = (rows_left + 31) / 32;
    if (q.ragged && B2 && SAME && mt_big > 0 && rows_left > 0 && q.conv_variant == 0 && q.conv_ablate == 0 && !q.post && 256 % nt2 == 0 &&
        n_tall * nt2 <= 256) {
      add(CK_BIG_PP, "conv_big_pp_kernel", M, mt_big * nt2, 512, LDS_BIG_TALL).n_tall = n_tall;
      return finish();
    }
    if (mt_big > 0) {
      const int a = q.conv_ablate;
      ConvStep &st = add(CK_BIG_PP, "conv_big_pp_kernel", mt_big * 256, mt_big * nt2, 512, LDS_BIG, (double)(mt_big * 256) / (double)M);
      st.ablate = (q.dt == DT_F16 && (a == 1 || a == 2 || a == 3 || a == 4 || a == 8 || a == 16)) ? a : 0;
      st.post = post_main;
      m_begin = mt_big * 256;
      if (m_begin >= M) { plan->post_fused = post_main; return finish(); }
    }
  }
  // on the remaining paths only the deep-ring left-over behind fused 256x256 rounds and the split-K reduce implement the table
  plan->post_fused = q.post && (post_main || ksplit > 1);
  if (!grp && (m_begin > 0 || M >= 8192 || small_deep) && (KT >= 16 || small_deep) && ksplit == 1 && Cout % 128 == 0) {
    // left-over rows on an otherwise idle chip (and long-K layers too small for one full 256x256 round as a whole): a lone workgroup
    // per CU walks all K-steps, so per-step latency is what counts: conv_512 left-overs 61 us per launch on the 2-stage 128x128 tile,
    // 55 us on the 256x128 ping-pong, 39 us on conv_deep_kernel<64> (neutral-to-slower for the 8-step Linear layers, hence KT >= 16)
    const int n128 = Cout / 128;
    // conv_deep_kernel owns its CU, so it only pays while its grid is a single round (<= 256 workgroups).  A larger
    // left-over (mid-sized batches) first takes full rounds of the 256x128 ping-pong kernel, then the deep kernel.
    int rows = M - m_begin;
    if (((rows + 63) / 64) * n128 > 256) {
      const int mt_pp = (((rows + 255) / 256) * n128 / 256) * 256 / n128;  // 256-row m-tiles in full rounds
      const int rows_pp = std::min(mt_pp * 256, rows);
      const int rest = rows - rows_pp;
      const bool cascade = mt_pp > 0 && ((rest + 63) / 64) * n128 <= 256;
      const int m_end = cascade ? m_begin + rows_pp : M;
      add(CK_PP, "conv_pp_kernel(rem)", m_end, ((m_end - m_begin + 255) / 256) * n128, 512, LDS3_128, cascade ? (double)rows_pp / rows : 1.0);
      if (!cascade || rest == 0) return finish();
      m_begin += rows_pp;
      rows = rest;
    }
    add(CK_DEEP64, "conv_deep_kernel", M, ((rows + 63) / 64) * n128, 256, LDS_DEEP64).post = post_main;
    return finish();
  }
  if (!grp && q.conv_variant == 3 && KT >= 3 && ksplit == 1 && Cout % 128 == 0) {
    add(CK_PP, "conv_pp_kernel", M, ((M + 255) / 256) * (Cout / 128), 512, LDS3_128);
    return finish();
  }
  const int mtiles = (M - m_begin + 127) / 128;
  if (Cout % 128 == 0 && ksplit == 1 && m_begin == 0 && KT >= 4 && KT <= 8 && mtiles * (Cout / 128) <= 128 && (!grp || q.grp_rows % 128 == 0)) {
    // short-K layers of small problems (the Linear layers of Track): a workgroup is a chain of <= 8 K-steps whose load latency the
    // two-stage tile below exposes every step; the deep ring keeps three steps in flight
    add(CK_DEEP128, "conv_deep_kernel(short-K)", M, mtiles * (Cout / 128), 256, LDS_DEEP128);
  } else if (Cout % 128 == 0 && !grp && ksplit > 1 && kt_per >= 4) {
    // split-K slices on the deep-ring kernel (three K-steps in flight instead of one: a slice is a latency chain)
    add(CK_DEEP128, "conv_deep_kernel(split-K)", M, mtiles * (Cout / 128) * ksplit, 256, LDS_DEEP128);
  } else if (Cout % 128 == 0) {
    add(CK_IGEMM128, "conv_igemm_kernel<128>", M, mtiles * (Cout / 128) * ksplit, 256, LDS_IG128);
  } else {
    add(CK_IGEMM64, "conv_igemm_kernel<64>", M, mtiles * (Cout / 64) * ksplit, 256, LDS_IG64);
  }
  if (ksplit > 1) {
    const size_t octs = (size_t)(M - m_begin) * (Cout / 8);
    flops = 0; bytes = 0;
    add(CK_SPLITK_REDUCE, "conv_splitk_reduce_kernel", M, (int)((octs + 255) / 256), 256, 0).post = q.post;
  }
  return finish();
}

// =================================================================================================
// the schedule behind the trunk: QKV projection, attention, encoder tail, token pooling, read-out
// =================================================================================================
// plan_heads decides what runs behind the token tensor of the refiner (both heads), of the scorer's feature pass and of its cross-attention
// head; refiner_forward, scorer_features and scorer_head build the query and execute the plan.  Like plan_conv it is plain host arithmetic
// on the pass, the batch and the element type: it makes no HIP call, reads no global, and can be asked without a GPU (fpt_plan_heads,
// tests/test_heads_plan_cpu.py).  The Linear layers inside a form go through run_conv / plan_conv as before; their schedule is not
// restated here.  The shapes the forms rely on (512-wide Linear layers with a step-major copy, Linear(512, 3) read-outs) are what the loader
// builds for every network it accepts (check_head_layouts).

// Thresholds of this schedule, each measured in its round (EXPERIMENTS.md).
static constexpr int SEQ_TOKENS = 400;            // tokens per hypothesis (the 20 x 20 map of the trunk)
static_assert(LN_PMEAN_PARTS * LN_PMEAN_ROWS == SEQ_TOKENS, "layernorm_pmean_kernel's partition covers a sequence");
static constexpr int QKV_TILE_TOKENS = 80;        // qkv_tile_kernel: tokens per workgroup, resident in LDS (a sequence = 5 tiles)
static constexpr int QKV_TILE_MIN_ROWS = 800;     // ... from two sequences on (one sequence alone is a scorer batch of 1: too few workgroups)
static constexpr int ATT_QROWS = 128;             // attention32_kernel: query rows per workgroup (4 waves x 32)
static constexpr int ATT_SKV_QROWS = 32;          // attention32_skv_kernel: query rows per workgroup, its 4 waves split the keys
static constexpr int ATT_SKV_MAX_WGS = 64;        // the split-key kernel takes over when attention32_kernel's grid would have at most this many
static constexpr int ATT_SKV_MIN_T = 32;          // workgroups (a small grid of long latency chains) and the sequence is longer than one key block
static constexpr int TRACK_GROUP_PITCH = 512;     // Track: rows between the two heads' sequences in the grouped launches (400 padded to the 128-row tile)
static constexpr int ENC_TAIL_TOKENS_1 = 16, ENC_TAIL_TOKENS_5 = 80;   // enc_tail_kernel<., 1> / <., 5>: tokens per workgroup
static constexpr int LN_MEAN_MIN_N = 96;          // per-head chain: layernorm_mean_kernel (one workgroup per sequence) from this many sequences on; below it
                                                  // is a serial chain (26 us at N = 32 against 9 + 9 for layernorm + token_mean)
// dynamic LDS bytes
static constexpr int LDS_QKV_TILE = 16 * QKV_TILE_TOKENS * 64;
static constexpr int LDS_ATT_SKV = 4 * 2 * (32 * 256 + 8 * 1056);      // per wave: two buffers of a K tile + 8 V sub-tiles
static constexpr int LDS_ENC_TAIL_1 = 16 * ENC_TAIL_TOKENS_1 * 64 + 2 * 8 * ENC_TAIL_TOKENS_1 * 4;              // tile + LayerNorm exchanges
static constexpr int LDS_ENC_TAIL_5 = 16 * ENC_TAIL_TOKENS_5 * 64 + 2 * 8 * ENC_TAIL_TOKENS_5 * 4 + 4 * 8192;   // ... + the two parked x1 fragments
// Settled the other way and retired (EXPERIMENTS.md, "Heads schedule in one plan"): the round-1 attention_kernel; 8 waves per workgroup and
// the lazy running maximum in attention32_kernel (their instantiations; the template keeps the two parameters); the token mean inside
// Track's read-out launch (token_mean_pose_kernel); the switch that put the QKV projection of N > 1 back on the Linear schedule.

enum HeadsPass { HP_REFINER = 0, HP_SCORER_FEATURES = 1, HP_SCORER_HEAD = 2 };
enum QkvForm { QKV_LINEAR = 0, QKV_TILE = 1, QKV_GROUPED = 2 };   // the Linear schedule (plan_conv) / qkv_tile_kernel / Track's grouped Linear of both heads
enum AttKernel { ATT_32 = 0, ATT_32_SKV = 1 };
// enc_tail_kernel<., 1> / <., 5> in one launch, or (test build) Track's grouped five-launch chain / the chain per head; none in the scorer
enum TailForm { TAIL_NONE = 0, TAIL_ONE_1 = 1, TAIL_ONE_5 = 2, TAIL_GROUPED_CHAIN = 3, TAIL_HEAD_CHAIN = 4 };
// the tail's partial dot products / layernorm_pmean_kernel / layernorm_mean_kernel / layernorm_kernel + token_mean_kernel / token_mean_kernel alone (scorer)
enum PoolForm { POOL_TAIL_PDOT = 0, POOL_LN_PMEAN = 1, POOL_LN_MEAN = 2, POOL_LN_TOKEN_MEAN = 3, POOL_TOKEN_MEAN = 4 };
enum ReadoutKernel { RO_ENC_HEADS = 0, RO_SMALL_LINEAR2_POSE = 1, RO_SMALL_LINEAR2 = 2, RO_SMALL_LINEAR = 3 };

// The switches of the test build (fpt_set_enc_tail ...).  Only plan_heads reads them; the product passes the defaults.
struct HeadsOverride {
  int enc_tail = 1;      // 0: the refiner's encoder tail as launch chains
  int ln_pmean = 1;      // Track's chain: 0 = layernorm + token_mean instead of layernorm_pmean_kernel
  int fuse_pose = 1;     // 0: never fuse RefinePostProcess into the read-out
  int qkv_ablate = 0;    // timing ablation of qkv_tile_kernel (f16; 1, 2, 3, 4, 7)
  int att_variant = 1;   // id of a row of ATT_VARIANTS
};

// The instantiations of attention32_kernel: row 0 is the product's, the others exist in the test build only (timing, wrong results from
// row 2 on).  The launcher builds its kernel table from these rows (launch_attention); plan_attention picks the row.
struct AttVariant {
  int id;        // fpt_set_att_variant / fpt_attention_bench
  bool remap;    // the XCD remap of the grid
  int ablate;    // ABL bits: 1 no staging after the first tile, 2 no softmax, 4 no PV, 8 no QK, 16 no prefetch distance, 32 no LDS stores
};
static constexpr AttVariant ATT_VARIANTS[] = {{1, true, 0},  {8, false, 0},  {16, true, 16}, {17, true, 1}, {18, true, 2},  {19, true, 32},
                                              {20, true, 4}, {22, true, 6}, {24, true, 8},  {30, true, 14}, {31, true, 15}};
#ifdef FP_TEST_HOOKS
static constexpr int N_ATT_VARIANTS = (int)(sizeof(ATT_VARIANTS) / sizeof(ATT_VARIANTS[0]));
#else
static constexpr int N_ATT_VARIANTS = 1;   // the product instantiates row 0 alone
#endif

struct HeadsQuery {
  int pass = HP_REFINER;
  int N = 1;                 // hypotheses (the scorer head: of all shards together)
  int dt = DT_F16;           // element type of the token path (DT_F16 / DT_BF16)
  bool fuse_offer = false;   // the caller offers a PoseUpdateFuse
  HeadsOverride ov;
};

struct AttLaunch {
  int kernel = ATT_32;       // AttKernel
  int variant = 0;           // row of ATT_VARIANTS (attention32_kernel; the split-key kernel has the product's form only)
  int B = 0, T = 0, pitch = 0;   // sequences, tokens per sequence, rows between the first tokens of consecutive sequences
  int nq = 0;                // query tiles per sequence and head
  unsigned grid = 0;
  int block = 256, lds = 0;  // threads per workgroup, dynamic LDS bytes
};

struct HeadsPlan {
  int qkv = QKV_LINEAR;      // QkvForm
  int qkv_ablate = 0;        // test build: the qkv_tile_kernel ablation instantiated (0 = the real kernel)
  unsigned qkv_grid = 0;     // qkv_tile_kernel: workgroups (512 threads)
  int qkv_lds = 0;
  AttLaunch att;
  int tail = TAIL_NONE;      // TailForm
  int tail_tiles = 0;        // enc_tail_kernel: tiles per head (the grid is both heads')
  unsigned tail_grid = 0;
  int tail_lds = 0;
  int pool = POOL_TOKEN_MEAN;      // PoolForm
  int readout = RO_SMALL_LINEAR;   // ReadoutKernel
  bool fuse_pose = false;    // RefinePostProcess runs inside the read-out kernel
};

// the launch of ONE of the two kernels over B sequences of T tokens: query tiles, grid, dynamic LDS.  The only copy of this arithmetic:
// plan_attention chooses between two of these, the test build's fpt_attention_raw forces either.
static AttLaunch attention_launch(int kernel, int variant, int B, int T, int pitch) {
  AttLaunch a;
  a.kernel = kernel; a.variant = variant;
  a.B = B; a.T = T; a.pitch = pitch;
  const int qrows = kernel == ATT_32_SKV ? ATT_SKV_QROWS : ATT_QROWS;
  a.nq = (T + qrows - 1) / qrows;
  a.grid = (unsigned)(a.nq * HEADS * B);
  a.lds = kernel == ATT_32_SKV ? LDS_ATT_SKV : 0;
  return a;
}

// self- or cross-attention over B sequences of T tokens
static AttLaunch plan_attention(int B, int T, int pitch, const HeadsOverride &ov) {
  int variant = 0;
  for (int i = 0; i < N_ATT_VARIANTS; i++)
    if (ATT_VARIANTS[i].id == ov.att_variant) variant = i;   // (a retired or unknown id: the product's row)
  const AttLaunch a = attention_launch(ATT_32, variant, B, T, pitch);
  // a small grid of long latency chains (Track: 2 sequences; the cross-attention: one): split the keys over the waves instead
  if (variant == 0 && a.grid <= (unsigned)ATT_SKV_MAX_WGS && T > ATT_SKV_MIN_T) return attention_launch(ATT_32_SKV, 0, B, T, pitch);
  return a;
}

// the launch of qkv_tile_kernel over `rows` tokens and of ONE enc_tail_kernel form over `tiles` tiles per head: workgroups and dynamic LDS.
// The only copies of this arithmetic: plan_heads fills its plan through them, the test build's fpt_qkv_tile_raw / fpt_enc_tail_raw
// build theirs from them alone.
static void qkv_tile_launch(int rows, HeadsPlan *plan) {
  plan->qkv = QKV_TILE;
  plan->qkv_grid = (unsigned)(rows / QKV_TILE_TOKENS);
  plan->qkv_lds = LDS_QKV_TILE;
}
static void enc_tail_launch(int form, int tiles, HeadsPlan *plan) {
  plan->tail = form;
  plan->tail_tiles = tiles;
  plan->tail_grid = (unsigned)(2 * tiles);
  plan->tail_lds = form == TAIL_ONE_1 ? LDS_ENC_TAIL_1 : LDS_ENC_TAIL_5;
}

static int plan_heads(const HeadsQuery &q, HeadsPlan *plan) {
  *plan = HeadsPlan{};
  FP_CHECK(q.dt == DT_F16 || q.dt == DT_BF16, "plan_heads: the transformer part runs on 2-byte elements");
  FP_CHECK(q.pass >= HP_REFINER && q.pass <= HP_SCORER_HEAD && q.N >= 1, "plan_heads: invalid query");
  const HeadsOverride &ov = q.ov;
  const int N = q.N;
  if (q.pass == HP_SCORER_HEAD) {   // cross-attention: the N hypotheses are ONE sequence; Linear layers in front and behind, Linear(512, 1) in f32
    plan->att = plan_attention(1, N, N, ov);
    return 0;
  }
  FP_CHECK(N <= MAX_BATCH, "plan_heads: batch outside 1..FP_MAX_BATCH");
  const bool refiner = q.pass == HP_REFINER;
  const bool track = refiner && N == 1;         // both heads in ONE launch per layer: Track is bound by its dependent launches, not by work
  const bool chain = refiner && !ov.enc_tail;
  const int rows = N * SEQ_TOKENS;
  if (track) {
    plan->qkv = QKV_GROUPED;
  } else if (!chain && rows % QKV_TILE_TOKENS == 0 && rows >= QKV_TILE_MIN_ROWS) {
    qkv_tile_launch(rows, plan);
    const int a = ov.qkv_ablate;
    plan->qkv_ablate = (q.dt == DT_F16 && (a == 1 || a == 2 || a == 3 || a == 4 || a == 7)) ? a : 0;
  }
  plan->att = track ? plan_attention(2, SEQ_TOKENS, TRACK_GROUP_PITCH, ov) : plan_attention(N, SEQ_TOKENS, SEQ_TOKENS, ov);
  if (!refiner) return 0;   // scorer features: token mean, then out_proj as a 512 x 512 GEMV in f32 (out_proj is affine: it commutes with the mean)
  if (!chain) {
    // [r5] everything row-wise behind the attention -- out_proj, LayerNorm 1, FFN, LayerNorm 2 and each tile's share of the read-out -- as ONE
    // launch for both heads, and one small launch that adds the shares up
    enc_tail_launch(track ? TAIL_ONE_1 : TAIL_ONE_5, rows / (track ? ENC_TAIL_TOKENS_1 : ENC_TAIL_TOKENS_5), plan);
    plan->pool = POOL_TAIL_PDOT;
    plan->readout = RO_ENC_HEADS;
    plan->fuse_pose = track && q.fuse_offer && ov.fuse_pose;
  } else if (track) {
    plan->tail = TAIL_GROUPED_CHAIN;
    plan->pool = ov.ln_pmean ? POOL_LN_PMEAN : POOL_LN_TOKEN_MEAN;
    plan->fuse_pose = q.fuse_offer && ov.fuse_pose;
    plan->readout = plan->fuse_pose ? RO_SMALL_LINEAR2_POSE : RO_SMALL_LINEAR2;
  } else {
    plan->tail = TAIL_HEAD_CHAIN;
    plan->pool = N >= LN_MEAN_MIN_N ? POOL_LN_MEAN : POOL_LN_TOKEN_MEAN;
  }
  return 0;
}

// Activation taps (test build only; tests/test_layers_gpu.py): an armed tap copies the tensor a producer just wrote -- borders
// included -- device to device into the test's buffer, on the forward pass's own stream.
// In the product FP_TAP expands to nothing (its arguments are not evaluated).  Points: fp_nn.h, enum TapPoint.
#ifdef FP_TEST_HOOKS
struct TapSlot {
  void *dst = nullptr;
  size_t cap = 0;    // bytes the test's buffer holds
  size_t need = 0;   // bytes the producer wrote in the last armed call (copied only when they fit)
};
static TapSlot g_tap[2][TAP_POINTS];   // [refiner, scorer]
static int g_tap_pe_fused[2] = {-1, -1};   // the last call's conv_512 -> tokens fused the positional table (1) or not (0)
static void tap(const Ctx &c, int point, const void *src, size_t bytes) {
  TapSlot &t = g_tap[c.net->scorer ? 1 : 0][point];
  if (!t.dst) return;
  t.need = bytes;
  if (bytes <= t.cap) (void)hipMemcpyAsync(t.dst, src, bytes, hipMemcpyDeviceToDevice, c.s);
}
// image window (fpt_tap_window): nimg < 0 = whole tensors.  A per-image tap of [imgs][img_bytes] whose first N images are the hypotheses'
// own then copies hypotheses [img0, img0 + nimg) and, when the tensor also holds observed crops (images N..), the matching ones -- or the
// one shared crop.  Taps of cross-hypothesis or small tensors stay whole (FP_TAP).
static int g_tap_img0 = 0, g_tap_nimg = -1;
static void tap_imgs(const Ctx &c, int point, const void *src, size_t img_bytes, int imgs, int N) {
  if (g_tap_nimg < 0) { tap(c, point, src, img_bytes * imgs); return; }
  TapSlot &t = g_tap[c.net->scorer ? 1 : 0][point];
  if (!t.dst) return;
  const int w0 = std::min(g_tap_img0, N), w1 = std::min(N, g_tap_img0 + g_tap_nimg);
  const int nb = imgs - N;   // observed crops: 0, 1 (shared) or N
  const size_t wn = (size_t)(w1 - w0), nbw = nb == N ? wn : (size_t)nb;
  t.need = w1 > w0 ? (wn + nbw) * img_bytes : 0;
  if (!t.need || t.need > t.cap) return;
  const unsigned char *s = static_cast<const unsigned char *>(src);
  unsigned char *d = static_cast<unsigned char *>(t.dst);
  (void)hipMemcpyAsync(d, s + (size_t)w0 * img_bytes, wn * img_bytes, hipMemcpyDeviceToDevice, c.s);
  if (nbw) (void)hipMemcpyAsync(d + wn * img_bytes, s + ((size_t)N + (nb == N ? w0 : 0)) * img_bytes, nbw * img_bytes, hipMemcpyDeviceToDevice, c.s);
}
#define FP_TAP(c, point, src, bytes) tap(c, point, src, bytes)
#define FP_TAP_IMGS(c, point, src, img_bytes, imgs, N) tap_imgs(c, point, src, img_bytes, imgs, N)

// Launch log (test build only; fpt_launch_log_*): while armed, every network kernel launch of run_conv and the other launch helpers
// appends one record -- the schedule that ran, for the coverage test of tests/test_layers_gpu.py.  It reads the schedule decisions and
// makes none.
struct LaunchRec {
  int net, prec;        // 0 refiner / 1 scorer, PREC_*
  int side;             // always 0 (kept for the layout of the record: a side stream was an experiment once)
  int m_begin, M;       // output rows [m_begin, M) of a convolution / GEMM launch (0, 0 elsewhere)
  int ksplit;           // split-K slices (1 = none)
  int pe;               // the launch adds the positional table in its epilogue
  char name[80];        // "tag/kernel" as the profiler names it
};
static int g_launch_log_on = 0;   // 1: the networks' launches, 2: also the launches outside the networks (log_geometry_launch)
static std::vector<LaunchRec> g_launch_log;
void log_geometry_launch(const char *name) {
  if (g_launch_log_on != 2) return;
  LaunchRec r{-1, -1, 0, 0, 0, 1, 0, {}};
  std::snprintf(r.name, sizeof(r.name), "%s", name);
  g_launch_log.push_back(r);
}
// Plan-only mode (fpt_plan_forward): the host side of a forward pass runs and the launch log records what it would launch, but no
// network kernel is issued -- FP_LAUNCH / FP_LAUNCH_RAW do nothing.  The schedule is decided exactly as in a real call.
static bool g_plan_only = false;
void nn_plan_only(bool on) { g_plan_only = on; }
#else
#define FP_TAP(c, point, src, bytes) ((void)0)
#define FP_TAP_IMGS(c, point, src, img_bytes, imgs, N) ((void)0)
#endif

// ProfScope of one network launch; in the test build it also appends the launch to the armed launch log.  The second form is a step
// of a convolution / Linear plan: "tag/kernel", and the record's rows, slices and positional table straight from the step.
struct NetScope : ProfScope {
  NetScope(const Ctx &c, const char *name, double flops = 0, double bytes = 0);
  NetScope(const Ctx &c, const char *tag, const ConvStep &st);
#ifdef FP_TEST_HOOKS
  long idx = -1;
#endif
};
inline NetScope::NetScope(const Ctx &c, const char *name, double flops, double bytes) : ProfScope(c.prof, c.s, name, flops, bytes) {
#ifdef FP_TEST_HOOKS
  if (!g_launch_log_on || !c.net) return;
  LaunchRec r{c.net->scorer ? 1 : 0, c.net->prec, 0, 0, 0, 1, 0, {}};
  std::snprintf(r.name, sizeof(r.name), "%s", name);
  idx = (long)g_launch_log.size();
  g_launch_log.push_back(r);
#endif
}
inline NetScope::NetScope(const Ctx &c, const char *tag, const ConvStep &st) : NetScope(c, (std::string(tag) + "/" + st.name).c_str(), st.flops, st.bytes) {
#ifdef FP_TEST_HOOKS
  if (idx < 0) return;
  LaunchRec &r = g_launch_log[(size_t)idx];
  r.m_begin = st.m_begin; r.M = st.M; r.ksplit = st.ksplit; r.pe = st.post ? 1 : 0;
#endif
}

// One launch = (once per launch site, element type and DEVICE) dynamic-LDS opt-in + the launch itself.  FP_LAUNCH_RAW: a network
// launch without the opt-in.  In the test build both do nothing in plan-only mode.
#ifdef FP_TEST_HOOKS
#define FP_LAUNCH_SKIP g_plan_only
#else
#define FP_LAUNCH_SKIP false
#endif
#define FP_LAUNCH(KERN, grid, block, lds_bytes, stream, ...)                                                                        \
  do {                                                                                                                              \
    if (FP_LAUNCH_SKIP) break;                                                                                                      \
    static fp::PerDeviceOnce fp_attr_once_;                                                                                         \
    fp_attr_once_.run([] { (void)hipFuncSetAttribute((const void *)(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }); \
    hipLaunchKernelGGL((KERN), grid, block, lds_bytes, stream, __VA_ARGS__);                                                        \
  } while (0)
#define FP_LAUNCH_RAW(...)                       \
  do {                                           \
    if (!FP_LAUNCH_SKIP) hipLaunchKernelGGL(__VA_ARGS__); \
  } while (0)

// a tensor as run_conv sees it: element type + (FP8) per-tensor scale, real = stored * scale
struct Act {
  void *p = nullptr;
  int dt = DT_F16;
  float scale = 1.f;
};

// in: [NB, H+2*ipad, W+2*ipad, Cin]; out: [.., OH+2*opad, OW+2*opad, ..]; res: border rpad
struct ConvGroup {  // two weight groups along M (see ConvParams::grp_rows); L holds [2][Cout][K] weights and [2][Cout] biases
  int rows = 0;     // rows per group (multiple of 128); the launch covers 2 * rows
  bool in_shared = false, res_shared = false;
};

template <int MI, int NI, int DT, int ODT, bool POST>
static void launch_conv_small(const Ctx &c, const ConvStep &st, const ConvParams &p) {
#ifdef FP_TEST_HOOKS   // A/B (g_smallm == 3): the first version, input fragments global -> registers in operand shape
  if constexpr (!is_q8(DT)) {
    if (st.kernel == CK_SMALLM) {
      if (st.deep) FP_LAUNCH((conv_smallm_kernel<MI, NI, DT, ODT, POST, true>), dim3(st.grid), dim3(256), st.lds, c.s, p);
      else FP_LAUNCH((conv_smallm_kernel<MI, NI, DT, ODT, POST, false>), dim3(st.grid), dim3(256), st.lds, c.s, p);
      return;
    }
  }
#endif
  FP_LAUNCH((conv_smallx_kernel<MI, NI, DT, ODT, POST>), dim3(st.grid), dim3(256), st.lds, c.s, p);
}

// One step of a plan on its kernel.  DT = element type of the layer's operands; ODT = of its output.  ODT != DT only for the layers at
// the 8-bit boundaries (encodeA.1: f16 -> 8-bit, the last encodeAB conv: 8-bit -> f16 tokens) and the scaled / dual 8-bit outputs; every
// pair instantiates only the kernels plan_conv can choose for it.
template <int DT, int ODT>
static int launch_conv_step(const Ctx &c, const ConvStep &st, const ConvParams &p) {
  constexpr bool B2 = !is_q8(DT), SAME = DT == ODT, QOUT = odt_q(ODT) >= 0;   // as in plan_conv
  const dim3 grid(st.grid), block((unsigned)st.block);
  switch (st.kernel) {
    case CK_SMALLX:
    case CK_SMALLM:
      if constexpr (!QOUT) {
        if (st.post && st.ni == 4) {
          if (st.mi == 2) launch_conv_small<2, 4, DT, ODT, true>(c, st, p); else launch_conv_small<1, 4, DT, ODT, true>(c, st, p);
          return 0;
        }
      }
      if (st.post) break;
      if (st.ni == 4) {
        if (st.mi == 2) launch_conv_small<2, 4, DT, ODT, false>(c, st, p); else launch_conv_small<1, 4, DT, ODT, false>(c, st, p);
        return 0;
      }
      if constexpr (B2) {
        if (st.mi == 2) launch_conv_small<2, 2, DT, ODT, false>(c, st, p); else launch_conv_small<1, 2, DT, ODT, false>(c, st, p);
        return 0;
      }
      break;
    case CK_STEM_HALO:
      if constexpr (B2 && SAME) { FP_LAUNCH((conv_stem_halo_kernel<DT>), grid, block, st.lds, c.s, p); return 0; }
      break;
    case CK_GEMM_K32:
      if constexpr (B2 && SAME) {
        if (st.wpack) FP_LAUNCH((gemm_k32_kernel<0, DT, true, true>), grid, block, st.lds, c.s, p);
        else FP_LAUNCH((gemm_k32_kernel<0, DT, true>), grid, block, st.lds, c.s, p);
        return 0;
      }
      break;
    case CK_S2_HALO:
      if constexpr (B2) { FP_LAUNCH((conv_s2_halo_kernel<DT, ODT>), grid, block, st.lds, c.s, p); return 0; }
      break;
    case CK_HALO:
      if constexpr (B2 && SAME) {
#ifdef FP_TEST_HOOKS
        switch (st.ablate) {
          case 1: FP_LAUNCH((conv_halo_kernel<40, 1, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 2: FP_LAUNCH((conv_halo_kernel<40, 2, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 8: FP_LAUNCH((conv_halo_kernel<40, 8, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 16: FP_LAUNCH((conv_halo_kernel<40, 16, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 32: FP_LAUNCH((conv_halo_kernel<40, 32, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          default: break;
        }
#endif
        FP_LAUNCH((conv_halo_kernel<40, 0, DT>), grid, block, st.lds, c.s, p);
        return 0;
      }
      break;
    case CK_HALO8:
      if constexpr (!B2 && odt_q(ODT) == DT) { FP_LAUNCH((conv_halo8_kernel<DT, ODT>), grid, block, st.lds, c.s, p); return 0; }
      break;
    case CK_PP32:
      if constexpr (B2) { FP_LAUNCH((conv_pp32_kernel<512, 128, DT, ODT>), grid, block, st.lds, c.s, p); return 0; }
      break;
    case CK_BIG_PP:
      if constexpr (!(DT == DT_F16 && QOUT)) {
#ifdef FP_TEST_HOOKS
        switch (st.ablate) {
          case 1: FP_LAUNCH((conv_big_pp_kernel<1, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 2: FP_LAUNCH((conv_big_pp_kernel<2, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 3: FP_LAUNCH((conv_big_pp_kernel<3, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 4: FP_LAUNCH((conv_big_pp_kernel<4, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 8: FP_LAUNCH((conv_big_pp_kernel<8, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          case 16: FP_LAUNCH((conv_big_pp_kernel<16, DT_F16>), grid, block, st.lds, c.s, p); return 0;
          default: break;
        }
#endif
        if constexpr (!QOUT) {
          if (st.post) { FP_LAUNCH((conv_big_pp_kernel<0, DT, ODT, true>), grid, block, st.lds, c.s, p); return 0; }
        }
        if (st.post) break;
        FP_LAUNCH((conv_big_pp_kernel<0, DT, ODT>), grid, block, st.lds, c.s, p);
        return 0;
      }
      break;
    case CK_PP:
      FP_LAUNCH((conv_pp_kernel<128, DT, ODT>), grid, block, st.lds, c.s, p);
      return 0;
    case CK_DEEP64:
      if constexpr (!QOUT) {
        if (st.post) { FP_LAUNCH((conv_deep_kernel<64, DT, ODT, true>), grid, block, st.lds, c.s, p); return 0; }
      }
      if (st.post) break;
      FP_LAUNCH((conv_deep_kernel<64, DT, ODT>), grid, block, st.lds, c.s, p);
      return 0;
    case CK_DEEP128:
      FP_LAUNCH((conv_deep_kernel<128, DT, ODT>), grid, block, st.lds, c.s, p);
      return 0;
    case CK_IGEMM128:
      FP_LAUNCH((conv_igemm_kernel<128, 3, DT, ODT>), grid, block, st.lds, c.s, p);
      return 0;
    case CK_IGEMM64:
      FP_LAUNCH((conv_igemm_kernel<64, 3, DT, ODT>), grid, block, st.lds, c.s, p);
      return 0;
    case CK_SPLITK_REDUCE: {
#ifdef FP_TEST_HOOKS
      ConvParams pr = p;
      if (g_splitk_ablate) pr.ksplit = p.ksplit - 1;   // ablation: the reduction drops the last slice
#else
      const ConvParams &pr = p;
#endif
      FP_LAUNCH_RAW(conv_splitk_reduce_kernel, grid, block, 0, c.s, pr);
      return 0;
    }
  }
  FP_CHECK(false, std::string("run_conv: the plan chose ") + st.name + " for element types that have no such kernel");
}

// the fp32 partial slabs of a split-K launch: grown on demand (also in plan-only mode: a planned call leaves the model as a real one would)
static int ensure_splitk(const Ctx &c, size_t need, float **slab) {
#ifdef FP_TEST_HOOKS
  NNScratch *sk = c.ws ? c.ws : &g_hook_ws;
#else
  NNScratch *sk = c.ws;
#endif
  if (need > sk->splitk_cap) {
    if (sk->splitk) (void)hipFree(sk->splitk);
    sk->splitk = nullptr; sk->splitk_cap = 0;
    g_alloc_epoch++;
    FP_HIP_OK(hipMalloc((void **)&sk->splitk, need * sizeof(float)));
    sk->splitk_cap = need;
  }
  *slab = sk->splitk;
  return 0;
}

using ConvLaunch = int (*)(const Ctx &, const ConvStep &, const ConvParams &);
#ifdef FP_TEST_HOOKS
static ConvPlan g_last_conv_plan;   // the plan and the kernels' ODT of the last run_conv call of this process (single-threaded test hooks)
static int g_last_conv_odt = -1;
#endif

// what one run_conv call runs layer L on, by name
struct ConvArgs {
  Act in, out;
  int NB = 0, H = 0, W = 0;          // images and interior size of `in`
  int ipad = 0, opad = 0, rpad = 0;  // zero borders of in / out / res
  bool relu = false;
  const Act *res = nullptr;          // skip operand, added in front of the ReLU
  int split_imgs = 0;                // > 0: the output is the a|b channel concat of images [0, split_imgs) and the ones behind them
  const ConvGroup *grp = nullptr;
  const void *post = nullptr;        // a positional table the layer may add to its output (see ConvParams::post); *post_fused tells the
  bool *post_fused = nullptr;        // caller whether the plan did (otherwise the caller launches add_pos_embed_kernel)
  const Act *out2 = nullptr;         // 8-bit networks: the layer also writes the 8-bit copy of its f16 output (DT_DUAL_*) ...
  const float *oinv = nullptr;       // ... value * oinv[channel]; without out2: `out` is that scaled 8-bit copy alone (DT_QS_*)
  const float *rscale = nullptr;     // res is an 8-bit tensor with these per-channel scales (DT_QSR_I8 / DT_F16RQ_I8)
  const float *bias_img = nullptr;   // INT8: [NB][Cout] biases, one row per image
};
static int run_conv(const Ctx &c, const char *tag, const ConvLayer &L, const ConvArgs &g) {
  const Act &in = g.in, &out = g.out, *res = g.res, *out2 = g.out2;
  const int NB = g.NB, H = g.H, W = g.W, ipad = g.ipad, opad = g.opad, rpad = g.rpad, split_imgs = g.split_imgs;
  const ConvGroup *grp = g.grp;
  const void *post = g.post; bool *post_fused = g.post_fused;
  const float *oinv = g.oinv, *rscale = g.rscale, *bias_img = g.bias_img;
  ConvParams p;
  p.bias_img = bias_img;
  FP_CHECK(!bias_img || (L.dt == DT_I8 && !grp), "run_conv: a per-image bias belongs to an INT8 layer");
  p.out2 = out2 ? (unsigned char *)out2->p : nullptr;
  p.oinv = oinv;
  p.rscale = rscale;
  FP_CHECK(!rscale || (res && res->dt == DT_I8 && L.dt == DT_I8 && !out2 && !grp), "run_conv: unsupported 8-bit residual");
  FP_CHECK(!out2 || (out.dt == DT_F16 && is_q8(out2->dt) && oinv && !grp && !post), "run_conv: unsupported dual output");
  FP_CHECK(out2 || !oinv || (is_q8(out.dt) && (out.dt == L.dt || (L.dt == DT_F16 && out.dt == DT_I8)) && !grp && !post), "run_conv: unsupported scaled 8-bit output");
  p.post = nullptr;
  if (post_fused) *post_fused = false;
  FP_CHECK(in.dt == L.dt, "run_conv: input element type does not match the layer's weights");
  FP_CHECK(!is_q8(L.dt) || L.cscale, "run_conv: 8-bit layer without scales");
  const int es = elem_bytes(L.dt);
  p.clk = g_clk_probe;
  p.grp_rows = grp ? grp->rows : 0;
  p.in_shared = grp && grp->in_shared;
  p.res_shared = grp && grp->res_shared;
  p.grp_w_bytes = grp ? (unsigned)((size_t)L.Cout * L.KH * L.KW * L.Cin * es) : 0;
  FP_CHECK(!grp || (grp->rows % 128 == 0 && L.KH == 1 && L.KW == 1 && NB == 2 * grp->rows && !is_q8(L.dt)), "grouped launch: unsupported shape");
  p.in = (const unsigned char *)in.p; p.w = L.w; p.wfrag = L.wfrag; p.wpack = L.wpack; p.wpack128 = L.wpack128; p.wdeep = L.wdeep; p.bias = L.bias; p.cscale = is_q8(L.dt) ? L.cscale : nullptr;
  p.res = res ? (const unsigned char *)res->p : nullptr; p.out = (unsigned char *)out.p;
  p.out_dt = out.dt; p.res_dt = res ? res->dt : out.dt;
  p.NB = NB; p.H = H; p.W = W; p.Cin = L.Cin;
  p.KH = L.KH; p.KW = L.KW; p.stride = L.stride; p.pad = L.pad;
  p.ipad = ipad; p.opad = opad; p.rpad = rpad;
  conv_out_hw(L.KH, L.KW, L.stride, L.pad, H, W, &p.OH, &p.OW);
  p.Cout = L.Cout;
  p.M = NB * p.OH * p.OW;
  p.Ktot = L.KH * L.KW * L.Cin;
  p.cin_b = L.Cin * es;
  p.krow_b = p.Ktot * es;
  p.ntaps = L.KH * L.KW;
  p.relu = g.relu ? 1 : 0;
  p.split_imgs = split_imgs;
  p.out_ld = split_imgs > 0 ? 2 * L.Cout : L.Cout;
  p.res_ld = L.Cout;
  p.ksplit = 1; p.kt_per = p.krow_b / 128; p.partial = nullptr;
  p.m_begin = 0; p.n_tall = 0;
  FP_CHECK(ipad >= L.pad && (p.cin_b == 64 || p.cin_b % 128 == 0) && p.krow_b % 128 == 0 && (L.Cout % 64) == 0 &&
               (p.cin_b != 64 || L.KW % 2 == 0) && p.krow_b / 128 <= 80,
           "conv shape not supported by the MFMA kernel");
  {
    // K order: 128-byte channel chunks -> (chunk outer, tap inner); 64-byte pixels (s2d stem) -> two horizontally adjacent
    // taps (128 contiguous bytes) per K-step.  koff = byte offset of the K-step's X slab from the row's (tap 0, ch 0) address.
    const int IWp = W + 2 * ipad;
    for (int kt = 0; kt < p.krow_b / 128; kt++) {
      int kh, kw, ch;
      if (p.cin_b >= 128) { ch = kt / p.ntaps; int tap = kt % p.ntaps; kh = tap / L.KW; kw = tap % L.KW; }
      else { ch = 0; int tap = 2 * kt; kh = tap / L.KW; kw = tap % L.KW; }
      p.koff[kt] = (unsigned)((kh * IWp + kw) * p.cin_b + ch * 128);
      if (2 * kt + 1 < 160) { p.koff32[2 * kt] = p.koff[kt]; p.koff32[2 * kt + 1] = p.koff[kt] + 64; }
    }
  }
  FP_CHECK(!res || res->dt == (rscale ? DT_I8 : is_q8(L.dt) ? DT_F16 : L.dt), "run_conv: the residual must have the layer's operand type (f16 for the 8-bit layers)");
  FP_CHECK(!post || (opad == 0 && split_imgs == 0 && !is_q8(out.dt) && post_fused), "run_conv: positional table on an unsupported layer");

  // the output type as the kernels' ODT parameter, and the instantiations of that <DT, ODT> pair
  int odt = -1;
  ConvLaunch launch = nullptr;
#define FP_CONV_PAIR(DT_, ODT_) (odt = ODT_, launch = &launch_conv_step<DT_, ODT_>)
  if (out2) {
    if (L.dt == DT_FP8 && out2->dt == DT_FP8) FP_CONV_PAIR(DT_FP8, DT_DUAL_FP8);
    else if (L.dt == DT_I8 && out2->dt == DT_I8) FP_CONV_PAIR(DT_I8, DT_DUAL_I8);
    else if (L.dt == DT_F16 && out2->dt == DT_FP8) FP_CONV_PAIR(DT_F16, DT_DUAL_FP8);
    else if (L.dt == DT_F16 && out2->dt == DT_I8) FP_CONV_PAIR(DT_F16, DT_DUAL_I8);
  } else if (rscale) {   // (plan_trunk: i8_stream) the residual is the 8-bit stream copy
#ifdef FP_TEST_HOOKS
    FP_CHECK(oinv || out.dt == DT_F16, "run_conv: 8-bit residual with an unsupported output type");
    if (oinv) FP_CONV_PAIR(DT_I8, DT_QSR_I8); else FP_CONV_PAIR(DT_I8, DT_F16RQ_I8);
#else
    FP_CHECK(false, "run_conv: 8-bit residual operands exist in the test build only");
#endif
  } else if (oinv) {   // 8-bit output alone, scaled in the epilogue
    if (L.dt == DT_FP8) FP_CONV_PAIR(DT_FP8, DT_QS_FP8);
    else if (L.dt == DT_F16) {
#ifdef FP_TEST_HOOKS
      FP_CONV_PAIR(DT_F16, DT_QS_I8);   // (encodeA.1 of the i8_stream trunk)
#else
      FP_CHECK(false, "run_conv: f16 -> scaled 8-bit alone exists in the test build only");
#endif
    } else FP_CONV_PAIR(DT_I8, DT_QS_I8);
  }
  else if (L.dt == DT_FP8 && out.dt == DT_FP8) FP_CONV_PAIR(DT_FP8, DT_FP8);
  else if (L.dt == DT_FP8 && out.dt == DT_F16) FP_CONV_PAIR(DT_FP8, DT_F16);
  else if (L.dt == DT_I8 && out.dt == DT_I8) FP_CONV_PAIR(DT_I8, DT_I8);
  else if (L.dt == DT_I8 && out.dt == DT_F16) FP_CONV_PAIR(DT_I8, DT_F16);
  else if (L.dt == DT_BF16 && out.dt == DT_BF16) FP_CONV_PAIR(DT_BF16, DT_BF16);
  else if (L.dt == DT_F16 && out.dt == DT_F16) FP_CONV_PAIR(DT_F16, DT_F16);
#undef FP_CONV_PAIR
  FP_CHECK(launch, "run_conv: unsupported combination of operand / output element types");

  ConvProblem q;
  q.Cin = L.Cin; q.Cout = L.Cout; q.KH = L.KH; q.KW = L.KW; q.stride = L.stride; q.pad = L.pad; q.algo_K = L.algo_K;
  q.wfrag = L.wfrag != nullptr; q.wpack = L.wpack != nullptr;
  q.NB = NB; q.H = H; q.W = W; q.ipad = ipad;
  q.dt = L.dt; q.odt = odt;
  q.has_res = res != nullptr; q.split_imgs = split_imgs;
  q.grp_rows = grp ? grp->rows : 0;
  q.post = post != nullptr;
  q.conv_variant = g_conv_variant; q.conv_ablate = g_conv_ablate; q.smallm = g_smallm; q.ragged = g_conv_ragged;
  ConvPlan plan;
  if (plan_conv(q, &plan)) return 1;
  if (post_fused) *post_fused = plan.post_fused;
#ifdef FP_TEST_HOOKS
  g_last_conv_plan = plan; g_last_conv_odt = odt;   // (fpt_conv_q8_raw reports the plan that ran: this one, not a second plan_conv call)
#endif
  for (int i = 0; i < plan.n; i++) {
    const ConvStep &st = plan.step[i];
    p.m_begin = st.m_begin; p.M = st.M; p.n_tall = st.n_tall;
    p.ksplit = st.ksplit; p.kt_per = st.kt_per;
    p.post = st.post ? (const unsigned char *)post : nullptr;
    if (st.ksplit > 1 && ensure_splitk(c, (size_t)st.ksplit * (st.M - st.m_begin) * L.Cout, &p.partial)) return 1;
    NetScope ps(c, tag, st);
    if (launch(c, st, p)) return 1;
  }
  return 0;
}

// plain GEMM rows x Cin -> rows x Cout (Linear layer) on unpadded buffers
static int run_gemm(const Ctx &c, const char *tag, const ConvLayer &L, const void *in, int rows, void *out, bool relu,
                    const void *res = nullptr, const ConvGroup *grp = nullptr) {
  const Act ar{const_cast<void *>(res), L.dt, 1.f};
  ConvArgs g;
  g.in = Act{const_cast<void *>(in), L.dt, 1.f}; g.NB = rows; g.H = 1; g.W = 1; g.out = Act{out, L.dt, 1.f};
  g.relu = relu; g.res = res ? &ar : nullptr; g.grp = grp;
  return run_conv(c, tag, L, g);
}

// f16 / bf16 dispatch of the transformer part: f(tag) with tag.value = DT_F16 or DT_BF16 as a constant, tag's E = the element type
template <int DT>
struct DtTag {
  static constexpr int value = DT;
  using E = typename ElemT<DT>::t;
};
template <typename F>
static void with_dt(int dt, F &&f) {
  if (dt == DT_BF16) f(DtTag<DT_BF16>{});
  else f(DtTag<DT_F16>{});
}

static HeadsOverride heads_override() {   // the test build's switches; the defaults in the product, where they are constants
  HeadsOverride ov;
  ov.enc_tail = g_enc_tail; ov.ln_pmean = g_ln_pmean; ov.fuse_pose = g_fuse_pose; ov.qkv_ablate = g_qkv_ablate; ov.att_variant = g_att_variant;
  return ov;
}

// the QKV projection of `rows` tokens ([rows][512] -> [rows][1536]) in the form the plan chose: qkv_tile_kernel or the Linear schedule
static int run_qkv(const Ctx &c, const HeadsPlan &hp, const ConvLayer &L, const void *x, int rows, void *qkv) {
  if (hp.qkv != QKV_TILE) return run_gemm(c, "gemm_qkv", L, x, rows, qkv, false);
  NetScope ps(c, "gemm_qkv/qkv_tile_kernel", 2.0 * rows * EMBED * 3.0 * EMBED, (double)rows * EMBED * 2.0 * 4.0);
  const QkvTileParams q{(const unsigned char *)x, L.wstep, L.bias, (unsigned char *)qkv, (int)hp.qkv_grid};
  const dim3 grid(hp.qkv_grid), blk(512);
#ifdef FP_TEST_HOOKS
  switch (hp.qkv_ablate) {
    case 1: FP_LAUNCH((qkv_tile_kernel<DT_F16, 1>), grid, blk, hp.qkv_lds, c.s, q); return 0;
    case 2: FP_LAUNCH((qkv_tile_kernel<DT_F16, 2>), grid, blk, hp.qkv_lds, c.s, q); return 0;
    case 3: FP_LAUNCH((qkv_tile_kernel<DT_F16, 3>), grid, blk, hp.qkv_lds, c.s, q); return 0;
    case 4: FP_LAUNCH((qkv_tile_kernel<DT_F16, 4>), grid, blk, hp.qkv_lds, c.s, q); return 0;
    case 7: FP_LAUNCH((qkv_tile_kernel<DT_F16, 7>), grid, blk, hp.qkv_lds, c.s, q); return 0;
    default: break;
  }
#endif
  with_dt(L.dt, [&](auto t) { FP_LAUNCH((qkv_tile_kernel<decltype(t)::value>), grid, blk, hp.qkv_lds, c.s, q); });
  return 0;
}

// attention32_kernel's instantiations, one per row of ATT_VARIANTS (the product: row 0 alone)
template <int DT, size_t... I>
static void launch_attention32(const Ctx &c, const AttLaunch &a, const typename ElemT<DT>::t *q, typename ElemT<DT>::t *o, int ld, std::index_sequence<I...>) {
  const auto launch = [&](auto row) {
    constexpr AttVariant V = ATT_VARIANTS[decltype(row)::value];
    FP_LAUNCH_RAW((attention32_kernel<V.remap, DT, V.ablate>), dim3(a.grid), dim3(a.block), a.lds, c.s, q, o, a.T, a.nq, a.pitch, ld);
  };
  ((a.variant == (int)I ? launch(std::integral_constant<size_t, I>{}) : (void)0), ...);
}
static int run_attention(const Ctx &c, int dt, const AttLaunch &a, const void *qkv, void *out, int ld = 3 * EMBED) {
  double flops = 4.0 * (double)a.B * HEADS * (double)a.T * a.T * HDIM;
  NetScope ps(c, "attention", flops, (double)a.B * a.T * (1536 + 512) * 2.0);
  with_dt(dt, [&](auto t) {
    constexpr int DT = decltype(t)::value;
    using E = typename decltype(t)::E;
    if (a.kernel == ATT_32_SKV) FP_LAUNCH((attention32_skv_kernel<true, DT>), dim3(a.grid), dim3(a.block), a.lds, c.s, (const E *)qkv, (E *)out, a.T, a.nq, a.pitch, ld);
    else launch_attention32<DT>(c, a, (const E *)qkv, (E *)out, ld, std::make_index_sequence<N_ATT_VARIANTS>{});
  });
  return 0;
}

static void run_small_linear(const Ctx &c, const float *x, const LinearF32 &L, float *y, int B) {
  NetScope ps(c, "small_linear", 2.0 * B * L.out * L.in, 0);
  size_t waves = (size_t)((B + 7) / 8) * L.out;
  FP_LAUNCH_RAW(small_linear_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c.s, x, L.w, L.b, y, B, L.out, L.in);
}

static void run_token_mean(const Ctx &c, int dt, const void *x, float *out, int B, int T, int tstride = 0) {
  NetScope ps(c, "token_mean", 0, (double)B * T * EMBED * 2.0);
  with_dt(dt, [&](auto t) {
    using E = typename decltype(t)::E;
    FP_LAUNCH_RAW(token_mean_kernel<decltype(t)::value>, dim3(B, EMBED / 64), dim3(256), 0, c.s, (const E *)x, out, T, tstride ? tstride : T);
  });
}

#ifdef FP_TEST_HOOKS   // launchers of the chain forms' kernels (fp_nn_small_kernels.inc)
static void run_layernorm(const Ctx &c, int dt, const void *x, const LNParams &ln, void *y, size_t rows, const LNParams *ln1 = nullptr,
                          size_t split_row = 0) {
  NetScope ps(c, "layernorm", 0, (double)rows * EMBED * 4.0);
  const dim3 grid((unsigned)((rows + 3) / 4));
  const float *g1 = ln1 ? ln1->g : ln.g, *b1 = ln1 ? ln1->b : ln.b;
  const size_t sr = ln1 ? split_row : rows;
  with_dt(dt, [&](auto t) {
    using E = typename decltype(t)::E;
    FP_LAUNCH_RAW(layernorm_kernel<decltype(t)::value>, grid, dim3(256), 0, c.s, (const E *)x, ln.g, ln.b, (E *)y, rows, g1, b1, sr);
  });
}

static void run_layernorm_mean(const Ctx &c, int dt, const void *x, const LNParams &ln, float *out, int B, int T) {
  NetScope ps(c, "layernorm_mean", 0, (double)B * T * EMBED * 2.0);
  with_dt(dt, [&](auto t) {
    using E = typename decltype(t)::E;
    FP_LAUNCH_RAW(layernorm_mean_kernel<decltype(t)::value>, dim3(B), dim3(1024), 0, c.s, (const E *)x, ln.g, ln.b, ln.g, ln.b, B, out, T, T);
  });
}
#endif

// calibration statistics of a trunk activation [pixels incl. the zero border][C]: per channel |max| (optional) and the sum of the
// values -- 8-bit tensors de-quantised with their per-channel scale (DT_I8: (stored ^ 0x80) * scale).  Border pixels hold 0 and
// add nothing.  thread = (8 channels, a strided set of pixels): a thread's partial sum has a fixed order, the partial sums are
// combined as 2^-20 fixed-point INTEGER atomics -- order-independent, so the statistics (and every table derived from them) are
// reproducible bit for bit.
template <int DT>
__global__ __launch_bounds__(256) void chan_stats_kernel(const unsigned char *__restrict__ x, size_t pixels, int C, const float *__restrict__ scale,
                                                         float *__restrict__ amax, long long *__restrict__ sum) {
  const int groups = C / 8;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  const int cg = (int)(t % groups);
  const size_t p0 = t / groups, pstride = nthreads / groups;
  if (p0 >= pstride) return;   // (threads beyond the last whole group of `groups`)
  float m[8], sacc[8], sc[8];
#pragma unroll
  for (int e = 0; e < 8; e++) { m[e] = 0.f; sacc[e] = 0.f; sc[e] = (is_q8(DT) && scale) ? scale[cg * 8 + e] : 1.f; }
  for (size_t px = p0; px < pixels; px += pstride) {
    float f[8];
    if constexpr (DT == DT_I8) {
      const i2 v = *reinterpret_cast<const i2 *>(x + px * C + cg * 8);
#pragma unroll
      for (int e = 0; e < 8; e++) f[e] = (float)(((unsigned)v[e >> 2] >> ((e & 3) * 8) & 0xffu) ^ 0x80u) * sc[e];
    } else {
      decode8(load8_raw(x + (px * C + cg * 8) * elem_bytes(DT), DT), DT, f);
      if constexpr (DT == DT_FP8) {
#pragma unroll
        for (int e = 0; e < 8; e++) f[e] *= sc[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) { m[e] = fmaxf(m[e], fabsf(f[e])); sacc[e] += f[e]; }
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    if (amax && m[e] > 0.f) atomicMax(reinterpret_cast<int *>(amax + cg * 8 + e), __float_as_int(m[e]));   // (bits of non-negative floats order like ints)
    if (sacc[e] != 0.f) atomicAdd(reinterpret_cast<unsigned long long *>(sum + cg * 8 + e), (unsigned long long)__double2ll_rn((double)sacc[e] * 1048576.0));
  }
}
// the launch of chan_stats_kernel on a tensor [pixels][C] of element type dt (calib_record; fpt_chan_stats_raw); returns the grid
static unsigned launch_chan_stats(hipStream_t s, int dt, const unsigned char *x, size_t pixels, int C, const float *scale, float *amax, long long *sum) {
  const int groups = C / 8;
  const dim3 grid((unsigned)((size_t)1024 * groups / 256)), blk(256);   // 1024 pixel lanes per channel group
  if (dt == DT_BF16) FP_LAUNCH_RAW(chan_stats_kernel<DT_BF16>, grid, blk, 0, s, x, pixels, C, scale, amax, sum);
  else if (dt == DT_FP8) FP_LAUNCH_RAW(chan_stats_kernel<DT_FP8>, grid, blk, 0, s, x, pixels, C, scale, amax, sum);
  else if (dt == DT_I8) FP_LAUNCH_RAW(chan_stats_kernel<DT_I8>, grid, blk, 0, s, x, pixels, C, scale, amax, sum);
  else FP_LAUNCH_RAW(chan_stats_kernel<DT_F16>, grid, blk, 0, s, x, pixels, C, scale, amax, sum);
  return grid.x;
}
// act_id: trunk activation (0..14) = the tensor [imgs][HW + 2 pad][HW + 2 pad][C] at `buf`; dt / scale describe its elements
static void calib_record(const Ctx &c, int act_id, const void *buf, int imgs, int HW, int pad, int C, int dt, const float *scale) {
  if (!c.net->calib_mode || (c.net->calib_only >= 0 && c.net->calib_only != act_id)) return;
  const size_t pixels = (size_t)imgs * (HW + 2 * pad) * (HW + 2 * pad);
  c.net->calib_count[act_id] += (double)imgs * HW * HW;   // interior pixels: what net_calib_end divides the sums by
  float *amax = c.net->calib_mode == 1 ? c.net->calib_amax + act_id * 512 : nullptr;
  long long *sum = c.net->calib_sum + act_id * 512;
  launch_chan_stats(c.s, dt, (const unsigned char *)buf, pixels, C, scale, amax, sum);
}

// arena carve (by capacity, see ensure_scratch)
struct Arena {
  unsigned char *stem, *x128[3], *x256[3], *x512[3], *tokens, *qkv, *att, *y1, *y2;
  unsigned char *q128[3], *q256[3], *q512[3];   // 8-bit networks: 1-byte operand copies
};
static Arena carve(NNScratch *ws) {
  Arena a;
  const size_t cap = (size_t)ws->cap;
  unsigned char *p = ws->buf;
  a.stem = p; p += cap * SZ_STEM;
  for (int i = 0; i < 3; i++) { a.x128[i] = p; p += cap * SZ_128; }
  for (int i = 0; i < 3; i++) { a.x256[i] = p; p += cap * SZ_256; }
  for (int i = 0; i < 3; i++) { a.x512[i] = p; p += cap * SZ_512; }
  a.tokens = p; p += cap * SZ_TOK;
  a.qkv = p; p += cap * SZ_QKV;
  a.att = p; p += cap * SZ_TOK;
  a.y1 = p; p += cap * SZ_TOK;
  a.y2 = p; p += cap * SZ_TOK;
  for (int i = 0; i < 3; i++) { a.q128[i] = p; p += cap * SZ_128 / 2; }
  for (int i = 0; i < 3; i++) { a.q256[i] = p; p += cap * SZ_256 / 2; }
  for (int i = 0; i < 3; i++) { a.q512[i] = p; p += cap * SZ_512 / 2; }   // (only allocated for 8-bit networks; never touched otherwise)
  return a;
}

#ifdef FP_TEST_HOOKS
// nn_scratch_poison (test build): 2-byte pattern over the interior of [imgs][H + 2b][W + 2b][C], alternating pos / neg by element
__global__ void poison16_kernel(uint16_t *p, size_t imgs, int H, int W, int b, int C, uint16_t pos, uint16_t neg) {
  const size_t n = imgs * H * W * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    size_t r = i / C;
    const size_t ch = i % C, x = r % W;
    r /= W;
    const size_t y = r % H, img = r / H;
    p[((img * (H + 2 * b) + y + b) * (W + 2 * b) + x + b) * C + ch] = (i & 1) ? neg : pos;
  }
}
__global__ void poison32_kernel(uint32_t *p, size_t n, uint32_t pos, uint32_t neg) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = (i & 1) ? neg : pos;
}
int nn_scratch_poison(NNScratch *ws, int dt, int kind, hipStream_t s) {
  const bool bf = dt == DT_BF16;
  const uint16_t p16 = kind == 0 ? (bf ? 0x7FC0 : 0x7E00) : (bf ? 0x7F7F : 0x7BFF), n16 = kind == 0 ? p16 : (uint16_t)(p16 | 0x8000);
  const uint32_t p32 = kind == 0 ? 0x7FC00000u : 0x7F7FFFFFu, n32 = kind == 0 ? p32 : 0xFF7FFFFFu;
  auto grid = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)); };
  auto fill16 = [&](void *p, size_t imgs, int H, int W, int b, int C) {
    const size_t n = imgs * H * W * C;
    if (n) hipLaunchKernelGGL(poison16_kernel, grid(n), dim3(256), 0, s, (uint16_t *)p, imgs, H, W, b, C, p16, n16);
  };
  auto fill32 = [&](float *p, size_t n) {
    if (p && n) hipLaunchKernelGGL(poison32_kernel, grid(n), dim3(256), 0, s, (uint32_t *)p, n, p32, n32);
  };
  if (ws->buf) {
    const Arena a = carve(ws);
    const size_t cap = (size_t)ws->cap;
    fill16(a.stem, 2 * cap, 80, 80, 1, 64);
    for (int i = 0; i < 3; i++) {
      fill16(a.x128[i], 2 * cap, 40, 40, 1, 128);
      fill16(a.x256[i], cap, 40, 40, 1, 256);
      fill16(a.x512[i], cap, 20, 20, 1, 512);
    }
    for (unsigned char *t : {a.tokens, a.att, a.y1, a.y2}) fill16(t, cap, 400, 1, 0, EMBED);
    fill16(a.qkv, cap, 400, 1, 0, 3 * EMBED);
    fill32(ws->f32, cap * EMBED + F32_PSUMS);   // the pooled rows and the partial sums of layernorm_pmean_kernel
  }
  fill32(ws->splitk, ws->splitk_cap);
  if (ws->head_buf) fill16(ws->head_buf, (size_t)ws->head_cap * 5, 1, 1, 0, EMBED);
  fill32(ws->head_f32, (size_t)ws->head_cap * EMBED);
  FP_HIP_OK(hipGetLastError());
  return 0;
}
#endif

// the last trunk convolution writes the un-bordered token tensor; whoever did not fuse the positional table adds it here
static void add_pos_embed(const Ctx &c, const Arena &a, int N) {
  const Net *net = c.net;
  size_t rows = (size_t)N * 400;
  NetScope ps(c, "add_pos_embed", 0, (double)rows * EMBED * 4.0);
  size_t chunks = rows * (EMBED / 8);
  const dim3 grid((unsigned)((chunks + 255) / 256));
  if (net->act_dt == DT_BF16) FP_LAUNCH_RAW(add_pos_embed_kernel<DT_BF16>, grid, dim3(256), 0, c.s, (__bf16 *)a.tokens, (const __bf16 *)net->pe, 400, rows);
  else FP_LAUNCH_RAW(add_pos_embed_kernel<DT_F16>, grid, dim3(256), 0, c.s, (_Float16 *)a.tokens, (const _Float16 *)net->pe, 400, rows);
}
static void broadcast_b(const Ctx &c, unsigned char *cat, int N, int cb /* bytes of the b-half of a pixel */) {
  NetScope ps(c, "broadcast_b", 0, (double)N * 1600 * 2 * cb);
  size_t total = (size_t)(N - 1) * 1600 * (cb / 16);
  FP_LAUNCH_RAW(broadcast_b_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.s, cat, N, 42, 42, 40, 40, 1, cb);
}

// the launch of q8_img_bias_fused_kernel for layer L on its 8-bit input xq [NBi, HW + 2, HW + 2, Cin] (q8_img_bias; fpt_q8_img_bias_raw).
// lattice: the sums run over the even rows x even columns of the padded image (HW + 2 is even): (HW/2 + 1)^2 lattice points, (HW/2)^2
// of them interior; otherwise over every pixel
static unsigned launch_q8_img_bias_fused(hipStream_t s, const ConvLayer &L, const unsigned char *xq, int NBi, int HW, bool lattice, float *out) {
  const int wp2 = lattice ? (HW + 2) / 2 : 0;
  const dim3 grid((NBi + Q8_BIAS_IMGS - 1) / Q8_BIAS_IMGS);
  FP_LAUNCH_RAW(q8_img_bias_fused_kernel, grid, dim3(1024), 0, s, xq, wp2 ? wp2 * wp2 : (HW + 2) * (HW + 2), L.tmat_t, L.cscale,
                     L.bias, wp2 ? 1.f / (float)((HW / 2) * (HW / 2)) : 1.f / (float)(HW * HW), L.Cin, L.Cout, out, wp2, (HW + 2) * (HW + 2), NBi);
  return grid.x;
}
#ifdef FP_TEST_HOOKS
// the three-launch form of the same (A/B, test build): sums [NBi][Cin] must be zero on entry and are left zero
static void launch_q8_img_bias_3(hipStream_t s, const ConvLayer &L, const unsigned char *xq, int NBi, int HW, int *sums, float *out) {
  FP_LAUNCH_RAW(q8_img_sum_kernel, dim3(NBi, HW == 40 ? 6 : 2), dim3(256), 0, s, xq, (HW + 2) * (HW + 2), L.Cin, sums);
  FP_LAUNCH_RAW(q8_img_bias_kernel, dim3(NBi, L.Cout / 64), dim3(256), 0, s, sums, L.tmat_t, L.cscale, L.bias, 1.f / (float)(HW * HW), L.Cin, L.Cout, out);
  (void)hipMemsetAsync(sums, 0, (size_t)NBi * L.Cin * sizeof(int), s);
}
#endif
// the launch of q8_copy_kernel: the 8-bit copy (type q) of the bordered f16 tensor x16 [imgs, HW + 2, HW + 2, Cc] (run_trunk; fpt_q8_copy_raw)
static unsigned launch_q8_copy(hipStream_t s, int q, const void *x16, void *xq, const float *oinv, int imgs, int HW, int Cc) {
  const size_t octs = (size_t)imgs * HW * HW * (Cc / 8);
  const dim3 grid((unsigned)((octs + 255) / 256));
  if (q == DT_FP8) FP_LAUNCH_RAW(q8_copy_kernel<DT_FP8>, grid, dim3(256), 0, s, (const _Float16 *)x16, (unsigned char *)xq, oinv, HW + 2, HW + 2, 1, Cc, octs);
  else FP_LAUNCH_RAW(q8_copy_kernel<DT_I8>, grid, dim3(256), 0, s, (const _Float16 *)x16, (unsigned char *)xq, oinv, HW + 2, HW + 2, 1, Cc, octs);
  return grid.x;
}
// INT8 [r5]: the per-image bias of layer L for its 8-bit input xq ([NBi, HW+2, HW+2, Cin] bytes): bias minus the first-order compensation
// of the weights' rounding error for that image's channel means.  (The error-feedback rounding has already cancelled this term for the
// calibration frames' means; what the compensation adds is the image's deviation from them.)
static const float *q8_img_bias(const Ctx &c, const ConvLayer &L, const void *xq, int NBi, int HW) {
  NetScope ps(c, "q8_img_bias", 0, (double)NBi * (HW + 2) * (HW + 2) * L.Cin);
#ifdef FP_TEST_HOOKS
  if (g_q8_imgbias == 2) {   // A/B (test build): the three-launch form (sliced integer-atomic sums, 64-channel bias blocks, clear)
    launch_q8_img_bias_3(c.s, L, (const unsigned char *)xq, NBi, HW, c.ws->img_sum, c.ws->img_bias);
  } else
#endif
  {
    launch_q8_img_bias_fused(c.s, L, (const unsigned char *)xq, NBi, HW, g_q8_imgbias != 3, c.ws->img_bias);
  }
  return c.ws->img_bias;
}

// shared CNN trunk: nn_in [2N,84,84,32] (s2d, border 2) -> tokens [N,400,512] + positional embedding
// n_b = number of observed-crop (B) images following the N rendered (A) images: N, or 1 when all hypotheses share it
// The rows come from TRUNK, what each does in this network from plan_trunk; nothing is decided here.
static int run_trunk(const Ctx &c, const Arena &a, const void *nn_in, int N, int n_b) {
  const Net *net = c.net;
  TrunkQuery q;
  q.dt = net->act_dt; q.N = N; q.n_b = n_b;
  if (net->prec == PREC_FP8 || net->prec == PREC_INT8) {
    q.qdt = net->qdt; q.mask = net->q8_blocks; q.i8_stream = g_i8_stream != 0;
    q.img_comp = net->q8_img_comp && c.ws && c.ws->img_sum && g_q8_imgbias;
    for (int r = 0; r < N_TRUNK; r++)
      if (trunk_layer(*net, r).tmat_t) q.comp_rows |= 1u << r;
  }
  TrunkPlan tp;
  if (plan_trunk(q, &tp)) return 1;
  void *const s16[TS_COUNT] = {const_cast<void *>(nn_in), a.stem, a.x128[0], a.x128[1], a.x128[2], a.x256[0], a.x256[1], a.x256[2], a.x512[0], a.x512[1], a.x512[2], a.tokens};
  void *const sq[TS_COUNT] = {nullptr, nullptr, a.q128[0], a.q128[1], a.q128[2], a.q256[0], a.q256[1], a.q256[2], a.q512[0], a.q512[1], a.q512[2], nullptr};
  const auto tensor = [&](int slot, bool copy) { return Act{copy ? sq[slot] : s16[slot], copy ? q.qdt : q.dt, 1.f}; };
  const int NB2 = N + n_b;
  // ([r5] stem + encodeA.1 in chunks of 63 / 84 / 126 images, so that the stem's output would be read back from the 256 MB memory-side
  // cache instead of HBM: 10.93 -> 11.24 / 11.13 / 11.00 ms per Register, slower with every extra launch -- EXPERIMENTS.md R5.4)
  FP_TAP_IMGS(c, TAP_NN_IN, nn_in, (size_t)84 * 84 * 32 * 2, NB2, N);
  for (int r = 0; r < N_TRUNK; r++) {
    const TrunkRow &t = TRUNK[r];
    const TrunkStep &st = tp.step[r];
    const ConvLayer &L = trunk_layer(*net, r);
    const int NB = t.ab ? NB2 : N, imgs = t.concat ? N : NB;   // images of the input / of the output
    int OH, OW;
    conv_out_hw(L.KH, L.KW, L.stride, L.pad, t.HW, t.HW, &OH, &OW);
    const Act res = st.res != TS_NONE ? tensor(st.res, st.res_q) : Act{}, copy = st.outq != TS_NONE ? tensor(st.outq, true) : Act{};
    ConvArgs g;
    g.in = tensor(st.in, st.in_q); g.NB = NB; g.H = t.HW; g.W = t.HW; g.ipad = t.ipad; g.opad = t.opad; g.rpad = t.rpad;
    g.out = st.out16 != TS_NONE ? tensor(st.out16, false) : copy; g.relu = true;
    g.res = st.res != TS_NONE ? &res : nullptr; g.split_imgs = t.concat ? N : 0;
    bool pe_done = false;
    if (t.pe) { g.post = net->pe; g.post_fused = &pe_done; }
    g.out2 = st.out16 != TS_NONE && st.outq != TS_NONE ? &copy : nullptr;
    g.oinv = st.oinv >= 0 ? net->act_oinv[st.oinv] : nullptr; g.rscale = st.rscale >= 0 ? net->act_scale_dev[st.rscale] : nullptr;
    if (st.img_bias) g.bias_img = q8_img_bias(c, L, g.in.p, NB, t.HW);
    if (run_conv(c, t.tag, L, g)) return 1;
    if (t.pe) {   // whoever did not fuse the positional table adds it here
      if (!pe_done) add_pos_embed(c, a, N);
#ifdef FP_TEST_HOOKS
      g_tap_pe_fused[net->scorer ? 1 : 0] = pe_done ? 1 : 0;
#endif
      FP_TAP(c, TAP_PE, net->pe, (size_t)400 * EMBED * 2);
    }
    // image N landed in the concat's channels [C/2, C) of image 0; replicate it for the other hypotheses
    if (st.bcast16) broadcast_b(c, (unsigned char *)s16[t.out], N, t.C / 2 * 2);
    if (st.bcastq) broadcast_b(c, (unsigned char *)sq[t.out], N, t.C / 2);
    if (st.qcopy >= 0) {
      NetScope ps(c, "q8_copy", 0, (double)imgs * OH * OH * t.C * 3.0);
      launch_q8_copy(c.s, q.qdt, s16[t.out], sq[t.out], net->act_oinv[st.qcopy], imgs, OH, t.C);
      FP_HIP_OK(hipGetLastError());
    }
    if (st.rec != TS_NONE)
      calib_record(c, t.act, st.rec_q ? sq[st.rec] : s16[st.rec], imgs, OH, t.opad, t.C, st.rec_dt, st.rec_scale >= 0 ? net->act_scale_dev[st.rec_scale] : nullptr);
    if (st.out16 != TS_NONE) FP_TAP_IMGS(c, t.tap, s16[t.out], (size_t)(OH + 2 * t.opad) * (OH + 2 * t.opad) * t.C * 2, imgs, N);
  }
  return 0;
}

static HeadsQuery heads_query(int pass, int N, int dt, bool fuse_offer) {
  HeadsQuery q;
  q.pass = pass; q.N = N; q.dt = dt; q.fuse_offer = fuse_offer;
  q.ov = heads_override();
  return q;
}

bool refiner_fuses_pose(const Net *net) {
  HeadsPlan hp;
  return net && !net->scorer && plan_heads(heads_query(HP_REFINER, 1, net->act_dt, true), &hp) == 0 && hp.fuse_pose;
}

// Track: the QKV projection and the self-attention of BOTH heads as one grouped launch each.  Rows [0,400) = translation head, [512,912) =
// rotation head (groups padded to the 128-row tile; the rows in between carry don't-care values that no valid row ever reads: every op
// behind the trunk is row-wise, attention is per sequence).  The attention outputs land in a.att at the same pitch.
static int track_qkv_attention(const Ctx &c, const HeadsPlan &hp, const Arena &a) {
  const int G = hp.att.pitch;
  const ConvGroup g_x{G, true, true};
  if (run_gemm(c, "gemm_qkv", c.net->g_in_proj, a.tokens, 2 * G, a.qkv, false, nullptr, &g_x)) return 1;
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_QKV, a.qkv, (size_t)SEQ_TOKENS * 3 * EMBED * 2);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_QKV, a.qkv + (size_t)G * 3 * EMBED * 2, (size_t)SEQ_TOKENS * 3 * EMBED * 2);
  if (run_attention(c, c.net->act_dt, hp.att, a.qkv, a.att)) return 1;
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_ATT, a.att, (size_t)SEQ_TOKENS * EMBED * 2);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_ATT, a.att + (size_t)G * EMBED * 2, (size_t)SEQ_TOKENS * EMBED * 2);
  return 0;
}

static EncTailParams enc_tail_params(const Net *net, const void *x, const void *att_trans, const void *att_rot, float *pdot, int tiles) {
  EncTailParams q{};
  q.x = (const unsigned char *)x;
  q.pdot = pdot;
  q.tiles = tiles;
  q.head_out = net->trans.head.out;
  const EncLayer *heads[2] = {&net->trans, &net->rot};
  const void *att[2] = {att_trans, att_rot};
  for (int i = 0; i < 2; i++) {
    const EncLayer &L = *heads[i];
    q.att[i] = (const unsigned char *)att[i];
    q.w[i][0] = L.att.out_proj.wstep; q.w[i][1] = L.lin1.wstep; q.w[i][2] = L.lin2.wstep;
    q.bias[i][0] = L.att.out_proj.bias; q.bias[i][1] = L.lin1.bias; q.bias[i][2] = L.lin2.bias;
    q.ln_g[i][0] = L.ln1.g; q.ln_b[i][0] = L.ln1.b; q.ln_g[i][1] = L.ln2.g; q.ln_b[i][1] = L.ln2.b;
    q.head_w[i] = L.head.w;
  }
  return q;
}

// the launch sites of enc_tail_kernel and enc_heads_kernel (one site each: the dynamic-LDS opt-in of FP_LAUNCH belongs to the site), shared by
// heads_one_launch and the test build's fpt_enc_tail_raw / fpt_enc_heads_raw
static void launch_enc_tail(const Ctx &c, int dt, const HeadsPlan &hp, const EncTailParams &q) {
  with_dt(dt, [&](auto t) {
    constexpr int DT = decltype(t)::value;
    if (hp.tail == TAIL_ONE_1) FP_LAUNCH((enc_tail_kernel<DT, 1>), dim3(hp.tail_grid), dim3(512), hp.tail_lds, c.s, q);
    else FP_LAUNCH((enc_tail_kernel<DT, 5>), dim3(hp.tail_grid), dim3(512), hp.tail_lds, c.s, q);
  });
}
static void launch_enc_heads(const Ctx &c, const EncHeadsParams &p, const PoseUpdateFuse *fuse) {
  FP_LAUNCH_RAW(enc_heads_kernel, dim3((unsigned)p.n), dim3(64), 0, c.s, p, fuse ? *fuse : PoseUpdateFuse{}, fuse ? 1 : 0);
}

// The refiner heads of the product (TAIL_ONE_1 / TAIL_ONE_5): QKV projection + self-attention per head (Track: grouped), then ONE launch for
// everything row-wise behind them (enc_tail_kernel, fp_nn_enc_kernels.inc: five dependent launches per head before, 33 us of Track's 202 us
// graph) and one for the token mean + Linear(512,3) of both heads, which at Track also applies RefinePostProcess when the plan says so
static int heads_one_launch(const Ctx &c, const HeadsPlan &hp, const Arena &a, int N, float *trans_dev, float *rot_dev, const PoseUpdateFuse *fuse) {
  const Net *net = c.net;
  const int dt = net->act_dt;
  const size_t rows = (size_t)N * SEQ_TOKENS;
  const unsigned char *att[2] = {a.att, a.y1};
  if (hp.qkv == QKV_GROUPED) {
    if (track_qkv_attention(c, hp, a)) return 1;
    att[1] = a.att + (size_t)hp.att.pitch * EMBED * 2;
  } else {
    const EncLayer *heads[2] = {&net->trans, &net->rot};
    unsigned char *att_out[2] = {a.att, a.y1};
    for (int i = 0; i < 2; i++) {
      if (run_qkv(c, hp, heads[i]->att.in_proj, a.tokens, (int)rows, a.qkv)) return 1;
      FP_TAP_IMGS(c, TAP_HEAD + i * TAP_HEAD_STRIDE + TAP_H_QKV, a.qkv, (size_t)SEQ_TOKENS * 3 * EMBED * 2, N, N);
      if (run_attention(c, dt, hp.att, a.qkv, att_out[i])) return 1;
      FP_TAP_IMGS(c, TAP_HEAD + i * TAP_HEAD_STRIDE + TAP_H_ATT, att_out[i], (size_t)SEQ_TOKENS * EMBED * 2, N, N);
    }
  }
  float *const pdot = reinterpret_cast<float *>(a.y2);   // [2][tiles][4] f32
  {
    NetScope ps(c, "enc_tail", 2.0 * 3.0 * 2.0 * (double)rows * EMBED * EMBED, 2.0 * 2.0 * (double)rows * EMBED * 2.0);
    const EncTailParams q = enc_tail_params(net, a.tokens, att[0], att[1], pdot, hp.tail_tiles);
    launch_enc_tail(c, dt, hp, q);
  }
  FP_TAP(c, TAP_PDOT, pdot, (size_t)2 * hp.tail_tiles * 4 * sizeof(float));
  {
    NetScope ps(c, "small_linear", 2.0 * 2 * N * net->trans.head.out * EMBED, 0);
    const EncHeadsParams p{pdot, {net->trans.head.b, net->rot.head.b}, {trans_dev, rot_dev}, N, hp.tail_tiles / N, net->trans.head.out, (float)SEQ_TOKENS};
    launch_enc_heads(c, p, hp.fuse_pose ? fuse : nullptr);
  }
  return 0;
}

#ifdef FP_TEST_HOOKS
// The launch-chain forms of the refiner heads (HeadsOverride::enc_tail = 0): what the product ran until round 5, kept in the test build as
// the reference whose every intermediate tensor can be tapped and checked in float64 (tests/test_layers_gpu.py).

// Track (TAIL_GROUPED_CHAIN): out_proj, LayerNorm 1, FFN1, FFN2, LayerNorm 2 + pooling as grouped launches over both heads
static int heads_grouped_chain(const Ctx &c, const HeadsPlan &hp, const Arena &a, NNScratch *ws, float *trans_dev, float *rot_dev, const PoseUpdateFuse *fuse) {
  const Net *net = c.net;
  const int dt = net->act_dt, G = hp.att.pitch;
  const EncLayer &T0 = net->trans, &R0 = net->rot;
  const void *x = a.tokens;
  const ConvGroup g_in{G, false, true}, g_own{G, false, false};
  if (track_qkv_attention(c, hp, a)) return 1;
  const size_t hb = (size_t)SEQ_TOKENS * EMBED * 2, ho = (size_t)G * EMBED * 2;   // (taps: a head's 400 rows, the second head's offset)
  if (run_gemm(c, "gemm_512", net->g_out_proj, a.att, 2 * G, a.y1, false, x, &g_in)) return 1;   // + residual x (shared)
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_Y1, a.y1, hb);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_Y1, a.y1 + ho, hb);
  run_layernorm(c, dt, a.y1, T0.ln1, a.y2, 2 * G, &R0.ln1, G);
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_X1, a.y2, hb);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_X1, a.y2 + ho, hb);
  if (run_gemm(c, "gemm_512", net->g_lin1, a.y2, 2 * G, a.y1, true, nullptr, &g_own)) return 1;
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_HID, a.y1, hb);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_HID, a.y1 + ho, hb);
  if (run_gemm(c, "gemm_512", net->g_lin2, a.y1, 2 * G, a.att, false, a.y2, &g_own)) return 1;   // + residual x1
  FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_Y2, a.att, hb);
  FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_Y2, a.att + ho, hb);
  // LayerNorm 2 feeds nothing but the token mean.  [r5] ONE launch: 2 x 16 workgroups normalise 25 rows each and leave partial column sums,
  // which the heads kernel adds up (layernorm_pmean_kernel).  Before: LayerNorm over 800 workgroup-rows + a 16-workgroup mean, two
  // dependent launches (11 us; the one-workgroup-per-sequence fused kernel of Register is a 20 us serial chain at two sequences)
  const bool pmean = hp.pool == POOL_LN_PMEAN;
  float *const psums = pmean_sums(ws);   // [2][LN_PMEAN_PARTS][512]
  if (pmean) {
    NetScope ps(c, "layernorm_pmean", 0, 2.0 * SEQ_TOKENS * EMBED * 2.0);
    with_dt(dt, [&](auto t) {
      using E = typename decltype(t)::E;
      FP_LAUNCH_RAW(layernorm_pmean_kernel<decltype(t)::value>, dim3(2, LN_PMEAN_PARTS), dim3(256), 0, c.s, (const E *)a.att, T0.ln2.g, T0.ln2.b, R0.ln2.g, R0.ln2.b, 1,
                    psums, SEQ_TOKENS, G, LN_PMEAN_ROWS);
    });
    FP_TAP(c, TAP_HEAD + 0 * TAP_HEAD_STRIDE + TAP_H_POOL, psums, (size_t)LN_PMEAN_PARTS * EMBED * sizeof(float));   // (partial column sums: 16 x 25 rows)
    FP_TAP(c, TAP_HEAD + 1 * TAP_HEAD_STRIDE + TAP_H_POOL, psums + LN_PMEAN_PARTS * EMBED, (size_t)LN_PMEAN_PARTS * EMBED * sizeof(float));
  } else {
    run_layernorm(c, dt, a.att, T0.ln2, a.y1, 2 * G, &R0.ln2, G);
    run_token_mean(c, dt, a.y1, ws->f32, 2, SEQ_TOKENS, G);
  }
  NetScope ps(c, "small_linear", 2.0 * 2 * T0.head.out * T0.head.in, 0);
  SmallLinear2 sl{{pmean ? psums : ws->f32, pmean ? psums + LN_PMEAN_PARTS * EMBED : ws->f32 + EMBED}, {T0.head.w, R0.head.w}, {T0.head.b, R0.head.b}, {trans_dev, rot_dev}};
  if (pmean) { sl.parts = LN_PMEAN_PARTS; sl.tokens = (float)SEQ_TOKENS; }
  if (hp.readout == RO_SMALL_LINEAR2_POSE) FP_LAUNCH_RAW(small_linear2_pose_kernel, dim3(1), dim3(1024), 0, c.s, sl, T0.head.in, *fuse);
  else FP_LAUNCH_RAW(small_linear2_kernel, dim3((unsigned)((T0.head.out + 3) / 4), 2), dim3(256), 0, c.s, sl, 1, T0.head.out, T0.head.in);
  return 0;
}

// N > 1 (TAIL_HEAD_CHAIN): the post-norm TransformerEncoderLayer of each head as launches, x1 = LN1(x + SA(x)); x2 = LN2(x1 + W2 relu(W1 x1))
static int heads_per_head_chain(const Ctx &c, const HeadsPlan &hp, const Arena &a, NNScratch *ws, int N, float *trans_dev, float *rot_dev) {
  const Net *net = c.net;
  const int dt = net->act_dt;
  const void *x = a.tokens;
  const size_t rows = (size_t)N * SEQ_TOKENS;
  const EncLayer *heads[2] = {&net->trans, &net->rot};
  float *outs[2] = {trans_dev, rot_dev};
  for (int i = 0; i < 2; i++) {
    const EncLayer &L = *heads[i];
    const int tp = TAP_HEAD + i * TAP_HEAD_STRIDE;
    const size_t tb1 = (size_t)SEQ_TOKENS * EMBED * 2;   // (taps: one hypothesis' 400 rows)
    if (run_qkv(c, hp, L.att.in_proj, x, (int)rows, a.qkv)) return 1;
    FP_TAP_IMGS(c, tp + TAP_H_QKV, a.qkv, 3 * tb1, N, N);
    if (run_attention(c, dt, hp.att, a.qkv, a.att)) return 1;
    FP_TAP_IMGS(c, tp + TAP_H_ATT, a.att, tb1, N, N);
    if (run_gemm(c, "gemm_512", L.att.out_proj, a.att, (int)rows, a.y1, false, x)) return 1;  // + residual x
    FP_TAP_IMGS(c, tp + TAP_H_Y1, a.y1, tb1, N, N);
    run_layernorm(c, dt, a.y1, L.ln1, a.y2, rows);                                           // x1 = y2
    FP_TAP_IMGS(c, tp + TAP_H_X1, a.y2, tb1, N, N);
    if (run_gemm(c, "gemm_512", L.lin1, a.y2, (int)rows, a.y1, true)) return 1;
    FP_TAP_IMGS(c, tp + TAP_H_HID, a.y1, tb1, N, N);
    if (run_gemm(c, "gemm_512", L.lin2, a.y1, (int)rows, a.att, false, a.y2)) return 1;       // + residual x1
    FP_TAP_IMGS(c, tp + TAP_H_Y2, a.att, tb1, N, N);
    if (hp.pool == POOL_LN_MEAN) run_layernorm_mean(c, dt, a.att, L.ln2, ws->f32, N, SEQ_TOKENS);
    else {
      run_layernorm(c, dt, a.att, L.ln2, a.y1, rows);
      FP_TAP_IMGS(c, tp + TAP_H_LN2, a.y1, tb1, N, N);
      run_token_mean(c, dt, a.y1, ws->f32, N, SEQ_TOKENS);
    }
    FP_TAP(c, tp + TAP_H_POOL, ws->f32, (size_t)N * EMBED * sizeof(float));
    run_small_linear(c, ws->f32, L.head, outs[i], N);  // Linear(512,3) commutes with the token mean
  }
  return 0;
}
#endif

int refiner_forward(hipStream_t s, Profiler *prof, const Net *net, NNScratch *ws, const void *nn_in, int N,
                    float *trans_dev, float *rot_dev, int shared_b, const PoseUpdateFuse *fuse, bool *fused_out) {
  if (fused_out) *fused_out = false;
  FP_CHECK(net && !net->scorer, "refiner_forward: wrong network");
  FP_CHECK(N >= 1 && N <= MAX_BATCH, "[FoundationPose] refine-net batch " + std::to_string(N) + " outside 1..FP_MAX_BATCH = " + std::to_string(MAX_BATCH));
  FP_CHECK(net_q8_ready(net), "[FoundationPose] the 8-bit precisions need a calibration: call fp_calibrate (fp_calibrate_fp8) first");
  if (ensure_scratch(ws, N, s)) return 1;
  Ctx c{s, prof, net, ws};
  const Arena a = carve(ws);
  if (run_trunk(c, a, nn_in, N, shared_b ? 1 : N)) return 1;
  HeadsPlan hp;
  if (plan_heads(heads_query(HP_REFINER, N, net->act_dt, fuse != nullptr), &hp)) return 1;
  switch (hp.tail) {
    case TAIL_ONE_1:
    case TAIL_ONE_5:
      if (heads_one_launch(c, hp, a, N, trans_dev, rot_dev, fuse)) return 1;
      break;
#ifdef FP_TEST_HOOKS
    case TAIL_GROUPED_CHAIN:
      if (heads_grouped_chain(c, hp, a, ws, trans_dev, rot_dev, fuse)) return 1;
      break;
    case TAIL_HEAD_CHAIN:
      if (heads_per_head_chain(c, hp, a, ws, N, trans_dev, rot_dev)) return 1;
      break;
#endif
    default:
      FP_CHECK(false, "refiner_forward: the launch-chain forms of the heads exist in the test build only");
  }
  if (fused_out) *fused_out = hp.fuse_pose;
  FP_TAP(c, TAP_TRANS, trans_dev, (size_t)N * 3 * sizeof(float));
  FP_TAP(c, TAP_ROT, rot_dev, (size_t)N * 3 * sizeof(float));
  FP_HIP_OK(hipGetLastError());
  return 0;
}

int scorer_features(hipStream_t s, Profiler *prof, const Net *net, NNScratch *ws, const void *nn_in, int N, float *feat_dev) {
  FP_CHECK(net && net->scorer, "scorer_features: wrong network");
  FP_CHECK(N >= 1 && N <= MAX_BATCH, "[FoundationPose] score-net batch " + std::to_string(N) + " outside 1..FP_MAX_BATCH = " + std::to_string(MAX_BATCH));
  FP_CHECK(net_q8_ready(net), "[FoundationPose] the 8-bit precisions need a calibration: call fp_calibrate (fp_calibrate_fp8) first");
  if (ensure_scratch(ws, N, s)) return 1;
  Ctx c{s, prof, net, ws};
  const Arena a = carve(ws);
  if (run_trunk(c, a, nn_in, N, N)) return 1;
  HeadsPlan hp;
  if (plan_heads(heads_query(HP_SCORER_FEATURES, N, net->act_dt, false), &hp)) return 1;
  const size_t rows = (size_t)N * SEQ_TOKENS;
  if (run_qkv(c, hp, net->att.in_proj, a.tokens, (int)rows, a.qkv)) return 1;
  FP_TAP_IMGS(c, TAP_HEAD + TAP_H_QKV, a.qkv, (size_t)SEQ_TOKENS * 3 * EMBED * 2, N, N);
  if (run_attention(c, net->act_dt, hp.att, a.qkv, a.att)) return 1;
  FP_TAP_IMGS(c, TAP_HEAD + TAP_H_ATT, a.att, (size_t)SEQ_TOKENS * EMBED * 2, N, N);
  // feature = mean_t(out_proj(att)) = out_proj(mean_t(att))  (out_proj is affine) -> 512x512 GEMV per hypothesis
  run_token_mean(c, net->act_dt, a.att, ws->f32, N, SEQ_TOKENS);
  FP_TAP(c, TAP_HEAD + TAP_H_POOL, ws->f32, (size_t)N * EMBED * sizeof(float));
  run_small_linear(c, ws->f32, net->att.out_proj_f32, feat_dev, N);
  FP_TAP(c, TAP_FEAT, feat_dev, (size_t)N * EMBED * sizeof(float));
  FP_HIP_OK(hipGetLastError());
  return 0;
}

int scorer_head(hipStream_t s, Profiler *prof, const Net *net, NNScratch *ws, const float *feats_dev, int n_total, float *scores_dev) {
  FP_CHECK(net && net->scorer, "scorer_head: wrong network");
  if (ensure_head_scratch(ws, n_total)) return 1;
  Ctx c{s, prof, net, ws};
  const int N = n_total, dt = net->act_dt;
  HeadsPlan hp;
  if (plan_heads(heads_query(HP_SCORER_HEAD, N, dt, false), &hp)) return 1;
  unsigned char *p = ws->head_buf;
  unsigned char *xf = p; p += (size_t)N * EMBED * 2;
  unsigned char *qkv = p; p += (size_t)N * 3 * EMBED * 2;
  unsigned char *att = p; p += (size_t)N * EMBED * 2;
  float *o32 = ws->head_f32;                  // [N,512]
  {
    NetScope ps(c, "cast", 0, (double)N * EMBED * 6.0);
    size_t n = (size_t)N * EMBED;
    const dim3 grid((unsigned)((n + 255) / 256));
    with_dt(dt, [&](auto t) { FP_LAUNCH_RAW(cast_f32_kernel<decltype(t)::value>, grid, dim3(256), 0, c.s, feats_dev, (typename decltype(t)::E *)xf, n); });
  }
  FP_TAP(c, TAP_XF, xf, (size_t)N * EMBED * 2);
  // att_cross: sequence = the N hypotheses, batch 1
  if (run_gemm(c, "gemm_cross", net->att_cross.in_proj, xf, N, qkv, false)) return 1;
  FP_TAP(c, TAP_XQKV, qkv, (size_t)N * 3 * EMBED * 2);
  if (run_attention(c, dt, hp.att, qkv, att)) return 1;
  FP_TAP(c, TAP_XATT, att, (size_t)N * EMBED * 2);
  // out_proj through the same MFMA GEMM (M = N rows), then Linear(512,1) in f32
  if (run_gemm(c, "gemm_cross", net->att_cross.out_proj, att, N, xf, false)) return 1;
  FP_TAP(c, TAP_XOUT, xf, (size_t)N * EMBED * 2);
  {
    // Linear(512,1) on 2-byte rows: widen to f32 first (token_mean with T = 1 is a plain copy of each row)
    NetScope ps(c, "score_linear", 2.0 * N * EMBED, 0);
    with_dt(dt, [&](auto t) { FP_LAUNCH_RAW(token_mean_kernel<decltype(t)::value>, dim3(N, EMBED / 64), dim3(256), 0, c.s, (const typename decltype(t)::E *)xf, o32, 1, 1); });
  }
  FP_TAP(c, TAP_O32, o32, (size_t)N * EMBED * sizeof(float));
  run_small_linear(c, o32, net->score_lin, scores_dev, N);
  FP_TAP(c, TAP_SCORES, scores_dev, (size_t)N * sizeof(float));
  FP_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace fp

#ifdef FP_TEST_HOOKS
#include "fp_nn_test_hooks.inc"
#endif  // FP_TEST_HOOKS
