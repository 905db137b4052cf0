// fp_nn_test_hooks.inc -- the fpt_* kernel-level hooks, A/B switches and micro-benchmarks of the TEST build (libfoundationpose_amd_test.so,
// -DFP_TEST_HOOKS); included by fp_nn.hip after namespace fp is closed.  Nothing of this file is in the product library.

// =================================================================================================
// MFMA micro-benchmark (measurement only): every wave issues `iters` x 8 independent v_mfma_f32_16x16x32_f16 from
// registers -- the rate the matrix pipes sustain with all 256 CUs busy at whatever clock the power limit allows.
__global__ __launch_bounds__(256) void mfma_peak_kernel(float *out, int iters, int zero_operands, unsigned long long *clk) {
  using fp::f4;
  using fp::h8;
  const int lane = threadIdx.x & 63;
  h8 a, b;
  unsigned st = 2654435761u * (unsigned)(blockIdx.x * 256 + threadIdx.x + 1);
#pragma unroll
  for (int i = 0; i < 8; i++) {  // random operands in [-0.5, 0.5): data-dependent power draw like real activations
    st = st * 1664525u + 1013904223u;
    a[i] = (_Float16)(((st >> 8) & 0xffff) / 65536.0f - 0.5f);
    st = st * 1664525u + 1013904223u;
    b[i] = (_Float16)(((st >> 8) & 0xffff) / 65536.0f - 0.5f);
    if (zero_operands) { a[i] = 0; b[i] = 0; }
  }
  unsigned long long c0 = 0, w0 = 0;
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) { c0 = __builtin_readcyclecounter(); w0 = wall_clock64(); }
  f4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++)  // inline asm: the builtin made hipcc shuffle the accumulators through AGPRs every iteration
      asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[j]) : "v"(a), "v"(b));
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // drain the MFMA pipe before the accumulators are read
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; j++) sum += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  if (sum == 12345.678f) out[lane] = sum;  // keeps the accumulators live; never true in practice
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) { clk[0] = __builtin_readcyclecounter() - c0; clk[1] = wall_clock64() - w0; }
}

// kernel-level test / micro-benchmark hooks (not part of the public C ABI; used by tests/test_nn_gpu.py and
// tools/bench_conv.py).  Host f32 in / out, fp16 on the device exactly like the production path.
// =================================================================================================
namespace {
template <typename T>
struct DevBuf {
  T *p = nullptr;
  explicit DevBuf(size_t n) { if (hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) p = nullptr; }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
std::vector<__half> to_half(const float *src, size_t n) {
  std::vector<__half> h(n);
  for (size_t i = 0; i < n; i++) h[i] = __float2half(src[i]);
  return h;
}
// float <-> element bytes of a 2-byte tensor
std::vector<unsigned char> encode(const float *src, size_t n, int dt, float scale) {
  (void)scale;
  std::vector<float> tmp(src, src + n);
  return fp::to_elems(tmp, 1, (int)n, dt, nullptr);
}
float e4m3_to_f32(unsigned char b) {
  const int e = (b >> 3) & 15, m = b & 7;
  float v = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.0f + m / 8.0f, e - 7);
  return (b & 0x80) ? -v : v;
}
void decode(const unsigned char *src, size_t n, int dt, float scale, float *dst) {
  for (size_t i = 0; i < n; i++) {
    if (dt == fp::DT_FP8) dst[i] = e4m3_to_f32(src[i]) * scale;
    else if (dt == fp::DT_BF16) { uint32_t u = (uint32_t)reinterpret_cast<const uint16_t *>(src)[i] << 16; std::memcpy(&dst[i], &u, 4); }
    else dst[i] = __half2float(reinterpret_cast<const __half *>(src)[i]);
  }
}
}  // namespace

extern "C" {

// activation taps (fp_nn.h, enum TapPoint): net_kind 0 = refiner, 1 = scorer.  Armed taps stay armed until fpt_tap_clear.
int fpt_tap_arm(int net_kind, int point, void *dst, size_t bytes) {
  if (net_kind < 0 || net_kind > 1 || point < 0 || point >= fp::TAP_POINTS) return 1;
  fp::g_tap[net_kind][point] = fp::TapSlot{dst, bytes, 0};
  return 0;
}
void fpt_tap_clear() {
  for (auto &k : fp::g_tap)
    for (auto &t : k) t = fp::TapSlot{};
  fp::g_tap_pe_fused[0] = fp::g_tap_pe_fused[1] = -1;
  fp::g_tap_img0 = 0;
  fp::g_tap_nimg = -1;
}
// bytes the producer of an armed tap wrote in the last call (copied only if they fit the buffer); 0 = not reached
long long fpt_tap_bytes(int net_kind, int point) { return (long long)fp::g_tap[net_kind & 1][point % fp::TAP_POINTS].need; }
// tap only hypotheses [img0, img0 + nimg) of the per-image tensors (fp_nn.hip, tap_imgs); nimg < 0 = whole tensors again
int fpt_tap_window(int img0, int nimg) {
  if (img0 < 0 || nimg == 0) return 1;
  fp::g_tap_img0 = nimg < 0 ? 0 : img0;
  fp::g_tap_nimg = nimg < 0 ? -1 : nimg;
  return 0;
}
// launch log (fp_nn.hip, LaunchRec): arm(1) clears it and records every network launch from now on, arm(0) stops; get(i) copies record i
// out as ints {net, prec, side, m_begin, M, ksplit, pe} and its "tag/kernel" name (name_cap bytes, NUL-terminated)
void fpt_launch_log_arm(int on) {
  if (on) fp::g_launch_log.clear();
  fp::g_launch_log_on = on == 2 ? 2 : on != 0;   // 2: with the launches outside the networks (net = -1)
}
int fpt_launch_log_count() { return (int)fp::g_launch_log.size(); }
int fpt_launch_log_get(int i, int *fields7, char *name, int name_cap) {
  if (i < 0 || i >= (int)fp::g_launch_log.size() || !fields7 || !name || name_cap <= 0) return 1;
  const fp::LaunchRec &r = fp::g_launch_log[(size_t)i];
  const int f[7] = {r.net, r.prec, r.side, r.m_begin, r.M, r.ksplit, r.pe};
  std::memcpy(fields7, f, sizeof(f));
  std::snprintf(name, (size_t)name_cap, "%s", r.name);
  return 0;
}
// every record at once: fields7 [max][7] as fpt_launch_log_get, names [max][name_cap]; returns the records copied
int fpt_launch_log_get_all(int *fields7, char *names, int name_cap, int max) {
  const int n = std::min(max, (int)fp::g_launch_log.size());
  for (int i = 0; i < n; i++)
    if (fpt_launch_log_get(i, fields7 + (size_t)i * 7, names + (size_t)i * name_cap, name_cap)) return -1;
  return n;
}
void fpt_launch_log_clear() { fp::g_launch_log.clear(); }
// did the last trunk of this network kind add the positional table in the epilogue of its last convolution (1) or separately (0)
int fpt_tap_pe_fused(int net_kind) { return fp::g_tap_pe_fused[net_kind & 1]; }
void fpt_set_att_variant(int v) { fp::g_att_variant = v; }
void fpt_set_smallm(int v) { fp::g_smallm = v; }
void fpt_set_fuse_pose(int v) { fp::g_fuse_pose = v; }
void fpt_set_q8_headroom(float v) { fp::g_q8_headroom = v; }
void fpt_set_q8_wq(int wclip, int efr, int imgbias) { fp::g_q8_wclip = wclip; fp::g_q8_efr = efr; fp::g_q8_imgbias = imgbias; }
void fpt_set_ln_pmean(int v) { fp::g_ln_pmean = v; }
void fpt_set_enc_tail(int v) { fp::g_enc_tail = v; }
void fpt_set_qkv_ablate(int v) { fp::g_qkv_ablate = v; }
// HOST-ONLY (no HIP call: runs without a GPU, tests/test_quantiser_cpu.py): the INT8 weight quantiser of fp_nn.hip on rows [Cout][taps][Cin]
// with the activation scales s_in [Cin] folded in and (m_int != null) the calibration frames' mean integer activations [J][Cin]:
// -> q [Cout][taps][Cin] int8, sw [Cout], tmat_t [Cin][Cout] (tap sums of the rounding errors, transposed)
int fpt_quantise_i8(const float *rows, int Cout, int ntaps, int Cin, const float *s_in, const float *m_int, int J, signed char *q_out, float *sw_out, float *tmat_t_out) {
  fp::ConvLayer L;
  L.Cout = Cout; L.Cin = Cin; L.ntaps = ntaps;
  L.rows_f32.assign(rows, rows + (size_t)Cout * ntaps * Cin);
  std::vector<float> sw, tm;
  std::vector<double> qsum;
  const auto q = fp::quantise_q8(L, fp::DT_I8, s_in, &sw, &qsum, m_int, J, &tm);
  std::memcpy(q_out, q.data(), q.size());
  std::memcpy(sw_out, sw.data(), sw.size() * sizeof(float));
  std::memcpy(tmat_t_out, tm.data(), tm.size() * sizeof(float));
  return 0;
}
// HOST-ONLY (no HIP call: runs without a GPU, tests/q8_conv_cases.py): the weight codes and row scales quantise_q8 gives an 8-bit layer of
// element type dt (DT_FP8 / DT_I8) without calibration means, as fpt_conv_q8_raw's apply_q8_layer call does: rows [Cout][taps][Cin] f32,
// s_in [Cin] -> q [Cout][taps][Cin] (e4m3 bits / int8), sw [Cout]
int fpt_quantise_q8(int dt, const float *rows, int Cout, int ntaps, int Cin, const float *s_in, unsigned char *q_out, float *sw_out) {
  if (!fp::is_q8(dt) || !rows || !s_in || !q_out || !sw_out || Cout < 1 || ntaps < 1 || Cin < 1) return 1;
  fp::ConvLayer L;
  L.Cout = Cout; L.Cin = Cin; L.ntaps = ntaps;
  L.rows_f32.assign(rows, rows + (size_t)Cout * ntaps * Cin);
  std::vector<float> sw;
  std::vector<double> qsum;
  const auto q = fp::quantise_q8(L, dt, s_in, &sw, &qsum);
  std::memcpy(q_out, q.data(), q.size());
  std::memcpy(sw_out, sw.data(), sw.size() * sizeof(float));
  return 0;
}
// HOST-ONLY (no HIP call: runs without a GPU, tests/test_conv_plan_cpu.py): the schedule plan_conv chooses for one convolution / Linear
// layer under the current switches.  shape10 = {Cin, Cout, KH, KW, stride, pad, NB, H, W, ipad}; dt / odt = element type of the operands /
// the kernels' output type (fp_nn.h, DT_*); flags: 1 = residual, 2 = a positional table is offered, 4 / 8 = the layer carries the
// fragment-order / gemm_k32_kernel's stage-order copy of its weights.  Returns the number of steps (-1 = no plan) and copies up to `max`
// of them out: fields11 [max][11] = the launch-log record {net = -1, prec = -1, side = 0, m_begin, M, ksplit, pe} + {kernel (ConvKernel),
// kt_per, grid, LDS bytes}, names [max][name_cap]; *post_fused = every row got the positional table.  fpt_plan_conv_tall(i): the 288-row
// tiles (ConvStep::n_tall) of step i of the plan the last fpt_plan_conv call returned, -1 = no such step.
static fp::ConvPlan g_hook_conv_plan;
int fpt_plan_conv_tall(int i) { return i >= 0 && i < g_hook_conv_plan.n ? g_hook_conv_plan.step[i].n_tall : -1; }
int fpt_plan_conv(const int *shape10, int dt, int odt, int flags, int split_imgs, int grp_rows, int *fields11, char *names, int name_cap, int max, int *post_fused) {
  fp::ConvProblem q;
  q.Cin = shape10[0]; q.Cout = shape10[1]; q.KH = shape10[2]; q.KW = shape10[3]; q.stride = shape10[4]; q.pad = shape10[5];
  q.NB = shape10[6]; q.H = shape10[7]; q.W = shape10[8]; q.ipad = shape10[9];
  q.dt = dt; q.odt = odt;
  q.has_res = (flags & 1) != 0; q.post = (flags & 2) != 0; q.wfrag = (flags & 4) != 0; q.wpack = (flags & 8) != 0;
  q.split_imgs = split_imgs; q.grp_rows = grp_rows;
  q.conv_variant = fp::g_conv_variant; q.conv_ablate = fp::g_conv_ablate; q.smallm = fp::g_smallm; q.ragged = fp::g_conv_ragged;
  fp::ConvPlan plan;
  g_hook_conv_plan = fp::ConvPlan{};
  if (fp::plan_conv(q, &plan)) return -1;
  g_hook_conv_plan = plan;
  for (int i = 0; i < plan.n && i < max; i++) {
    const fp::ConvStep &st = plan.step[i];
    const int f[11] = {-1, -1, 0, st.m_begin, st.M, st.ksplit, st.post ? 1 : 0, st.kernel, st.kt_per, (int)st.grid, st.lds};
    std::memcpy(fields11 + (size_t)i * 11, f, sizeof(f));
    std::snprintf(names + (size_t)i * name_cap, (size_t)name_cap, "%s", st.name);
  }
  if (post_fused) *post_fused = plan.post_fused ? 1 : 0;
  return plan.n;
}
// HOST-ONLY (no HIP call: runs without a GPU, tests/test_heads_plan_cpu.py): what plan_heads chooses behind the trunk under the current
// switches.  pass: 0 refiner, 1 scorer features, 2 scorer head (fp_nn.hip HeadsPass); dt: DT_F16 / DT_BF16; fuse_offer: the caller offers a
// PoseUpdateFuse.  fields18 = {qkv form, qkv ablation, qkv grid, qkv LDS bytes, attention kernel, XCD remap, attention ablation bits, B, T,
// pitch, query tiles, attention grid, attention block, attention LDS bytes, tail form, pooling form, read-out kernel, pose fused} (the enums
// of fp_nn.hip) and tail3 = {tiles per head, grid, LDS bytes} of enc_tail_kernel.  Returns 0, or 1 when the query is refused.
int fpt_plan_heads(int pass, int N, int dt, int fuse_offer, int *fields18, int *tail3) {
  fp::HeadsPlan p;
  if (fp::plan_heads(fp::heads_query(pass, N, dt, fuse_offer != 0), &p)) return 1;
  const fp::AttVariant &v = fp::ATT_VARIANTS[p.att.variant];
  const int f[18] = {p.qkv, p.qkv_ablate, (int)p.qkv_grid, p.qkv_lds, p.att.kernel, v.remap ? 1 : 0, v.ablate, p.att.B, p.att.T,
                     p.att.pitch, p.att.nq, (int)p.att.grid, p.att.block, p.att.lds, p.tail, p.pool, p.readout, p.fuse_pose ? 1 : 0};
  std::memcpy(fields18, f, sizeof(f));
  const int t[3] = {p.tail_tiles, (int)p.tail_grid, p.tail_lds};
  std::memcpy(tail3, t, sizeof(t));
  return 0;
}
// HOST-ONLY (no HIP call: runs without a GPU, tests/test_trunk_plan_cpu.py): what plan_trunk decides for the 15 rows of the trunk.  dt: DT_F16 /
// DT_BF16; qdt: DT_FP8 / DT_I8 or -1 (a 2-byte network); mask: the stages on 8-bit operands; i8_stream: the 8-bit residual stream;
// img_comp / comp_rows: the per-image compensation is available / bit r = row r's layer carries its tap sums; N hypotheses and n_b
// observed crops.  fields17 [15][17] = the fields of TrunkStep in their order (slots: TrunkSlot; -1 = none).  Returns 0, or 1 when the
// query is refused.
int fpt_plan_trunk(int dt, int qdt, int mask, int i8_stream, int img_comp, unsigned comp_rows, int N, int n_b, int *fields17) {
  fp::TrunkQuery q;
  q.dt = dt; q.qdt = qdt; q.mask = mask; q.i8_stream = i8_stream != 0; q.img_comp = img_comp != 0; q.comp_rows = comp_rows; q.N = N; q.n_b = n_b;
  fp::TrunkPlan p;
  if (fp::plan_trunk(q, &p)) return 1;
  for (int r = 0; r < fp::N_TRUNK; r++) {
    const fp::TrunkStep &s = p.step[r];
    const int f[17] = {s.op_dt, s.in, s.in_q, s.res, s.res_q, s.rscale, s.out16, s.outq, s.oinv, s.img_bias, s.bcast16, s.bcastq, s.qcopy,
                       s.rec, s.rec_q, s.rec_dt, s.rec_scale};
    std::memcpy(fields17 + (size_t)r * 17, f, sizeof(f));
  }
  return 0;
}
// HOST-ONLY (no HIP call: runs without a GPU, tests/test_depth_filter_cpu.py): plan_track_window (fp_geometry.hip) of n poses.
// K9 row-major intrinsics, poses16 [n][16] column-major -> out5 [n][5] = {kind (TrackWindowKind), row0, row1, col0, col1}
void fpt_plan_track_window(const float *K9, float diameter, const float *poses16, int H, int W, int reach, int *out5, int n) {
  for (int i = 0; i < n; i++) {
    const fp::TrackWindow w = fp::plan_track_window(K9, diameter, poses16 + (size_t)i * 16, H, W, reach);
    const int f[5] = {w.kind, w.row0, w.row1, w.col0, w.col1};
    for (int k = 0; k < 5; k++) out5[(size_t)i * 5 + k] = f[k];
  }
}
void fpt_depth_filter_tile(int *tile_w, int *tile_h) { *tile_w = fp::DEPTH_FILTER_TILE_W; *tile_h = fp::DEPTH_FILTER_TILE_H; }
void fpt_set_conv_variant(int v) { fp::g_conv_variant = v; }
void fpt_set_conv_ragged(int v) { fp::g_conv_ragged = v != 0; }   // (a captured graph keeps the schedule it was captured with: an A/B must re-capture)
void fpt_set_i8_stream(int v) { fp::g_i8_stream = v; }
void fpt_set_q8_blocks(int v) { fp::g_q8_blocks = v & fp::Q8_BLOCKS_ALL; }   // [r6] stage mask of 8-bit networks loaded from now on (tools/q8_blocks.py)
void fpt_set_conv_ablate(int v) { fp::g_conv_ablate = v; }
void fpt_set_splitk_ablate(int v) { fp::g_splitk_ablate = v; }

// clock probe: allocate room for `blocks` records, run convs, then read back mean shader MHz and mean main-loop cycles
int fpt_clk_probe(int blocks, double *mhz_out, double *loop_cycles_out) {
  using namespace fp;
  if (blocks > 0) {
    if (g_clk_probe) (void)hipFree(g_clk_probe);
    FP_HIP_OK(hipMalloc((void **)&g_clk_probe, (size_t)blocks * 32));
    FP_HIP_OK(fp::memset_sync(g_clk_probe, 0, (size_t)blocks * 32));
    return 0;
  }
  FP_CHECK(g_clk_probe, "no probe");
  int n = -blocks;
  std::vector<unsigned long long> h((size_t)n * 4);
  FP_HIP_OK(hipDeviceSynchronize());
  FP_HIP_OK(fp::memcpy_sync(h.data(), g_clk_probe, h.size() * 8, hipMemcpyDeviceToHost));
  double sc = 0, sr = 0; int cnt = 0;
  for (int i = 0; i < n; i++) {
    if (h[i * 4 + 3] > h[i * 4 + 1]) { sc += (double)(h[i * 4 + 2] - h[i * 4]); sr += (double)(h[i * 4 + 3] - h[i * 4 + 1]); cnt++; }
  }
  if (mhz_out) *mhz_out = sr > 0 ? sc / sr * 100.0 : 0;  // wall_clock64 ticks at 100 MHz
  if (loop_cycles_out) *loop_cycles_out = cnt ? sc / cnt : 0;
  (void)hipFree(g_clk_probe);
  g_clk_probe = nullptr;
  return 0;
}

// x [NB,H,W,Cin] NHWC f32, w [Cout,KH,KW,Cin] f32, bias [Cout], res (optional) [NB,OH,OW,Cout]
// -> out f32 [NB,OH,OW,Cout] (or, with split_imgs > 0, [NB-split,OH,OW,2*Cout]).  iters > 1: returns mean ms in *ms_out.
// dt = element type of x / w / res on the device (DT_F16 / DT_BF16), out_dt = element type of the output; the scale arguments are
// ignored (kept for the callers' signature).  8-bit layers: fpt_conv_q8.  The output buffer carries CONV_DT_GUARD canary bytes in front
// and behind: returns 2 when the launches changed one (a store outside the output rows).
static constexpr size_t CONV_DT_GUARD = 64 * 1024;
int fpt_conv_dt(const float *x, const float *w, const float *bias, const float *res, int NB, int H, int W, int Cin, int Cout,
                int KH, int KW, int stride, int pad, int OH, int OW, int relu, int split_imgs, float *out, int iters,
                float *ms_out, int dt, int out_dt, float in_scale, float res_scale, float out_scale) {
  using namespace fp;
  const int ip = pad;  // physical input border
  const int Hp = H + 2 * ip, Wp = W + 2 * ip;
  const int es = elem_bytes(dt), oes = elem_bytes(out_dt);
  size_t nx = (size_t)NB * Hp * Wp * Cin, nw = (size_t)Cout * KH * KW * Cin;
  size_t M = (size_t)NB * OH * OW;
  size_t nout = M * Cout;
  const size_t G = CONV_DT_GUARD;
  DevBuf<unsigned char> dx(nx * es), dres(nout * es), dguard(nout * oes + 2 * G);
  FP_CHECK(dx.p && dres.p && dguard.p, "fpt_conv: allocation failed");
  struct { unsigned char *p; } dout{dguard.p + G};
  FP_HIP_OK(fp::memset_sync(dguard.p, 0xA5, nout * oes + 2 * G));
  std::vector<float> xp(nx, 0.f);
  for (int n = 0; n < NB; n++)
    for (int y = 0; y < H; y++)
      for (int xx = 0; xx < W; xx++)
        for (int c = 0; c < Cin; c++)
          xp[(((size_t)n * Hp + y + ip) * Wp + xx + ip) * Cin + c] = x[(((size_t)n * H + y) * W + xx) * Cin + c];
  auto hx = encode(xp.data(), nx, dt, in_scale);
  FP_HIP_OK(fp::memcpy_sync(dx.p, hx.data(), hx.size(), hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memset_sync(dout.p, 0, nout * oes));
  if (res) {
    auto hr = encode(res, nout, dt, res_scale);
    FP_HIP_OK(fp::memcpy_sync(dres.p, hr.data(), hr.size(), hipMemcpyHostToDevice));
  }
  Net net;
  ConvLayer L;
  L.Cin = Cin; L.Cout = Cout; L.KH = KH; L.KW = KW; L.stride = stride; L.pad = pad;
  FP_CHECK(finish_layer(&net, std::vector<float>(w, w + nw), std::vector<float>(bias, bias + Cout), Cout, KH * KW, Cin, dt, &L), "fpt_conv: weight upload failed");
  FP_CHECK(!is_q8(dt) && !is_q8(out_dt), "fpt_conv_dt: 2-byte element types only (8-bit layers: fpt_conv_q8)");
  Ctx c{nullptr, nullptr, &net};
  (void)OH; (void)OW;
  const Act ares{dres.p, dt, res_scale};
  ConvArgs g;
  g.in = Act{dx.p, dt, in_scale}; g.NB = NB; g.H = H; g.W = W; g.ipad = ip;
  g.out = Act{dout.p, out_dt, out_scale}; g.relu = relu != 0; g.res = res ? &ares : nullptr; g.split_imgs = split_imgs;
  hipEvent_t e0, e1;
  FP_HIP_OK(hipEventCreate(&e0));
  FP_HIP_OK(hipEventCreate(&e1));
  if (run_conv(c, "t", L, g)) return 1;
  FP_HIP_OK(hipDeviceSynchronize());
  if (iters > 1) {
    FP_HIP_OK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; i++)
      if (run_conv(c, "t", L, g)) return 1;
    FP_HIP_OK(hipEventRecord(e1, nullptr));
    FP_HIP_OK(hipEventSynchronize(e1));
    float ms = 0;
    FP_HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  std::vector<unsigned char> ho(nout * oes);
  FP_HIP_OK(fp::memcpy_sync(ho.data(), dout.p, ho.size(), hipMemcpyDeviceToHost));
  decode(ho.data(), nout, out_dt, out_scale, out);
  std::vector<unsigned char> hg(2 * G);
  FP_HIP_OK(fp::memcpy_sync(hg.data(), dguard.p, G, hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(hg.data() + G, dout.p + nout * oes, G, hipMemcpyDeviceToHost));
  for (unsigned char v : hg)
    if (v != 0xA5) { fp::set_error("fpt_conv_dt: the kernels wrote outside the output buffer"); return 2; }
  return 0;
}
// One 8-bit convolution exactly as the 8-bit trunk runs it (net_apply_q8 / plan_trunk).
//   x [NB,H,W,Cin] f32 (>= 0 for DT_I8), s_in [Cin] per-channel activation scales: the device input is e4m3(x / s) or
//   (clamp(rint(x / s), 0, 255) ^ 0x80) with a border of "zero" bytes; w [Cout,KH,KW,Cin] f32 is quantised per row AFTER s_in is folded
//   in; res (optional) [NB,OH,OW,Cout] is f16 on the device.
//   mode 0: 8-bit output only, the consumer's scales s_out [Cout] folded into the epilogue tables -> outq (de-quantised values)
//   mode 1: f16 output only -> out16;  mode 2: f16 output + its 8-bit copy (value / s_out[c]) -> out16, outq
//   mode 3: the 8-bit copy alone, scaled in the epilogue (a layer with a residual whose f16 output nobody reads) -> outq
//   mode 4 / 5 (DT_I8): the residual is an 8-bit tensor itself, clamp(rint(res / s_res), 0, 255) ^ 0x80 (plan_trunk: i8_stream); 4: scaled 8-bit
//   output -> outq, 5: f16 output -> out16
// split_imgs > 0: the a|b channel concat ([NB - split, OH, OW, 2 * Cout]; s_out still indexed by the layer's output channel).
// wq_out (optional) [Cout*KH*KW*Cin]: the de-quantised weights the device used (w' / s_in, i.e. comparable with w), sw_out [Cout].
int fpt_conv_q8(const float *x, const float *s_in, const float *w, const float *bias, const float *res, int NB, int H, int W, int Cin, int Cout,
                int KH, int KW, int stride, int pad, int OH, int OW, int relu, int split_imgs, int mode, const float *s_out, float *out16,
                float *outq, int iters, float *ms_out, int dt, float *wq_out, const float *s_res) {
  using namespace fp;
  FP_CHECK(is_q8(dt) && mode >= 0 && mode <= 5 && (mode < 4 || (dt == DT_I8 && res && s_res)), "fpt_conv_q8: invalid arguments");
  const int ip = pad, Hp = H + 2 * ip, Wp = W + 2 * ip;
  const size_t nx = (size_t)NB * Hp * Wp * Cin, nw = (size_t)Cout * KH * KW * Cin, M = (size_t)NB * OH * OW, nout = M * Cout;
  DevBuf<unsigned char> dx(nx), dres(nout * 2), d16(nout * 2), dq(nout);
  FP_CHECK(dx.p && dres.p && d16.p && dq.p, "fpt_conv_q8: allocation failed");
  std::vector<unsigned char> hx(nx, dt == DT_I8 ? 0x80 : 0x00);
  for (int n = 0; n < NB; n++)
    for (int y = 0; y < H; y++)
      for (int xx = 0; xx < W; xx++)
        for (int c = 0; c < Cin; c++) {
          const float v = x[(((size_t)n * H + y) * W + xx) * Cin + c] / s_in[c];
          unsigned char b;
          if (dt == DT_FP8) b = f32_to_e4m3_bits(v);
          else b = (unsigned char)((int)std::max(0.f, std::min(255.f, std::nearbyint(v))) ^ 0x80);
          hx[(((size_t)n * Hp + y + ip) * Wp + xx + ip) * Cin + c] = b;
        }
  FP_HIP_OK(fp::memcpy_sync(dx.p, hx.data(), nx, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memset_sync(d16.p, 0, nout * 2));
  FP_HIP_OK(fp::memset_sync(dq.p, dt == DT_I8 ? 0x80 : 0, nout));
  float *rscale_dev = nullptr;
  if (res && mode >= 4) {
    std::vector<unsigned char> hr(nout);
    for (size_t i = 0; i < nout; i++) hr[i] = (unsigned char)((int)std::max(0.f, std::min(255.f, std::nearbyint(res[i] / s_res[i % Cout]))) ^ 0x80);
    FP_HIP_OK(fp::memcpy_sync(dres.p, hr.data(), nout, hipMemcpyHostToDevice));
  } else if (res) {
    auto hr = encode(res, nout, DT_F16, 1.f);
    FP_HIP_OK(fp::memcpy_sync(dres.p, hr.data(), hr.size(), hipMemcpyHostToDevice));
  }
  Net net;
  net.prec = dt == DT_FP8 ? PREC_FP8 : PREC_INT8;
  net.qdt = dt;
  ConvLayer L;
  L.Cin = Cin; L.Cout = Cout; L.KH = KH; L.KW = KW; L.stride = stride; L.pad = pad;
  FP_CHECK(finish_layer(&net, std::vector<float>(w, w + nw), std::vector<float>(bias, bias + Cout), Cout, KH * KW, Cin, dt, &L), "fpt_conv_q8: weight upload failed");
  if (apply_q8_layer(&net, L, dt, s_in, nullptr, mode == 0 ? s_out : nullptr, true)) return 1;
  if (wq_out) {  // what the device multiplies with, de-quantised and with s_in divided out again
    std::vector<float> sw; std::vector<double> qs;
    const auto e = quantise_q8(L, dt, s_in, &sw, &qs);
    for (size_t i = 0; i < nw; i++) {
      const int co = (int)(i / ((size_t)KH * KW * Cin)), ci = (int)(i % Cin);
      const float q = dt == DT_FP8 ? e4m3_to_f32(e[i]) : (float)(signed char)e[i];
      wq_out[i] = q * sw[co] / s_in[ci];
    }
  }
  float *oinv_dev = nullptr;
  if (mode >= 4) {
    rscale_dev = upload(&net, std::vector<float>(s_res, s_res + Cout));
    FP_CHECK(rscale_dev, "fpt_conv_q8: allocation failed");
  }
  if (mode >= 2 && mode != 5) {
    std::vector<float> inv(Cout);
    for (int c2 = 0; c2 < Cout; c2++) inv[c2] = 1.f / s_out[c2];
    oinv_dev = upload(&net, inv);
    FP_CHECK(oinv_dev, "fpt_conv_q8: allocation failed");
  }
  Ctx c{nullptr, nullptr, &net};
  (void)OH; (void)OW;
  const Act a16{d16.p, DT_F16, 1.f}, aq{dq.p, dt, 1.f}, ares{dres.p, mode >= 4 ? DT_I8 : DT_F16, 1.f};
  ConvArgs g;
  g.in = Act{dx.p, dt, 1.f}; g.NB = NB; g.H = H; g.W = W; g.ipad = ip;
  g.relu = relu != 0; g.res = res ? &ares : nullptr; g.split_imgs = split_imgs;
  g.out = (mode == 1 || mode == 2 || mode == 5) ? a16 : aq;   // the f16 tensor, or the 8-bit one alone
  g.out2 = mode == 2 ? &aq : nullptr; g.oinv = oinv_dev; g.rscale = rscale_dev;   // (the tables are null in the modes without them)
  auto once = [&]() { return run_conv(c, "t", L, g); };
  if (once()) return 1;
  FP_HIP_OK(hipDeviceSynchronize());
  if (iters > 1) {
    hipEvent_t e0, e1;
    FP_HIP_OK(hipEventCreate(&e0));
    FP_HIP_OK(hipEventCreate(&e1));
    FP_HIP_OK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; i++)
      if (once()) return 1;
    FP_HIP_OK(hipEventRecord(e1, nullptr));
    FP_HIP_OK(hipEventSynchronize(e1));
    float ms = 0;
    FP_HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  if ((mode == 1 || mode == 2 || mode == 5) && out16) {
    std::vector<unsigned char> ho(nout * 2);
    FP_HIP_OK(fp::memcpy_sync(ho.data(), d16.p, ho.size(), hipMemcpyDeviceToHost));
    decode(ho.data(), nout, DT_F16, 1.f, out16);
  }
  if (mode != 1 && mode != 5 && outq) {
    std::vector<unsigned char> ho(nout);
    FP_HIP_OK(fp::memcpy_sync(ho.data(), dq.p, nout, hipMemcpyDeviceToHost));
    // output layout [.., 2*Cout] with the concat: channel index modulo Cout selects the scale
    for (size_t i = 0; i < nout; i++) {
      const int ch = (int)(i % (split_imgs > 0 ? 2 * (size_t)Cout : (size_t)Cout)) % Cout;
      const float q = dt == DT_FP8 ? e4m3_to_f32(ho[i]) : (float)(ho[i] ^ 0x80);
      outq[i] = q * s_out[ch];
    }
  }
  return 0;
}
// The f16 -> 8-bit boundary layer (encodeA.1 of the 8-bit networks): f16 operands, f16 stream output + 8-bit copy (value / s_out[c]);
// out16 == null: the 8-bit copy alone (the INT8 trunk).
int fpt_conv_f16_dual(const float *x, const float *w, const float *bias, int NB, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int OH, const float *s_out, float *out16, float *outq, int qdt) {
  using namespace fp;
  FP_CHECK(is_q8(qdt), "fpt_conv_f16_dual: qdt must be an 8-bit type");
  const int ip = pad, Hp = H + 2 * ip, Wp = W + 2 * ip, OW = OH;
  const size_t nx = (size_t)NB * Hp * Wp * Cin, nw = (size_t)Cout * KH * KW * Cin, nout = (size_t)NB * OH * OW * Cout;
  DevBuf<unsigned char> dx(nx * 2), d16(nout * 2), dq(nout);
  FP_CHECK(dx.p && d16.p && dq.p, "fpt_conv_f16_dual: allocation failed");
  std::vector<float> xp(nx, 0.f);
  for (int n = 0; n < NB; n++)
    for (int y = 0; y < H; y++)
      for (int xx = 0; xx < W; xx++)
        for (int c = 0; c < Cin; c++) xp[(((size_t)n * Hp + y + ip) * Wp + xx + ip) * Cin + c] = x[(((size_t)n * H + y) * W + xx) * Cin + c];
  auto hx = encode(xp.data(), nx, DT_F16, 1.f);
  FP_HIP_OK(fp::memcpy_sync(dx.p, hx.data(), hx.size(), hipMemcpyHostToDevice));
  Net net;
  ConvLayer L;
  L.Cin = Cin; L.Cout = Cout; L.KH = KH; L.KW = KW; L.stride = stride; L.pad = pad;
  FP_CHECK(finish_layer(&net, std::vector<float>(w, w + nw), std::vector<float>(bias, bias + Cout), Cout, KH * KW, Cin, DT_F16, &L), "fpt_conv_f16_dual: weight upload failed");
  std::vector<float> inv(Cout);
  for (int c2 = 0; c2 < Cout; c2++) inv[c2] = 1.f / s_out[c2];
  float *oinv_dev = upload(&net, inv);
  FP_CHECK(oinv_dev, "fpt_conv_f16_dual: allocation failed");
  Ctx c{nullptr, nullptr, &net};
  const Act a16{d16.p, DT_F16, 1.f}, aq{dq.p, qdt, 1.f};
  ConvArgs g;
  g.in = Act{dx.p, DT_F16, 1.f}; g.NB = NB; g.H = H; g.W = W; g.ipad = ip;
  g.out = out16 ? a16 : aq; g.relu = true; g.out2 = out16 ? &aq : nullptr; g.oinv = oinv_dev;
  if (run_conv(c, "t", L, g)) return 1;
  FP_HIP_OK(hipDeviceSynchronize());
  std::vector<unsigned char> h16(nout * 2), hq(nout);
  FP_HIP_OK(fp::memcpy_sync(h16.data(), d16.p, h16.size(), hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(hq.data(), dq.p, nout, hipMemcpyDeviceToHost));
  if (out16) decode(h16.data(), nout, DT_F16, 1.f, out16);
  for (size_t i = 0; i < nout; i++) outq[i] = (qdt == DT_FP8 ? e4m3_to_f32(hq[i]) : (float)(hq[i] ^ 0x80)) * s_out[i % Cout];
  return 0;
}
// Host-only check of the weight layouts (no GPU): every (tile, K-step, lane) address a kernel forms into fragment_order /
// pack_stage_w / pack_stage_w128 must hold the bytes the same lane would have fetched from the row-major copy.
// Returns the number of mismatching 16-byte pieces (0 = all layouts agree), -1 for unsupported sizes.
long long fpt_check_weight_layouts(int Cout, int row_bytes) {
  using namespace fp;
  if (Cout % 256 || row_bytes % 128) return -1;
  std::vector<unsigned char> rows((size_t)Cout * row_bytes);
  unsigned st = 12345u;
  for (auto &b : rows) { st = st * 1664525u + 1013904223u; b = (unsigned char)(st >> 24); }
  long long bad = 0;
  auto same = [&](const unsigned char *a, const unsigned char *b) { return std::memcmp(a, b, 16) == 0; };
  const size_t KT = row_bytes / 128, S = row_bytes / 64;
  {  // conv_smallx_kernel: wrow = frag + (n0 >> 4) * 16 * krow_b + lane * 16;  + ni * 16 * krow_b + kt * 2048 + ks * 1024
    const auto f = fragment_order(rows, Cout, row_bytes);
    for (size_t t = 0; t < (size_t)Cout / 16; t++)
      for (size_t kt = 0; kt < KT; kt++)
        for (int ks = 0; ks < 2; ks++)
          for (int l = 0; l < 64; l++)
            bad += !same(&f[t * 16 * row_bytes + kt * 2048 + (size_t)ks * 1024 + (size_t)l * 16],
                         &rows[(t * 16 + (l & 15)) * row_bytes + kt * 128 + (size_t)ks * 64 + (size_t)(l >> 4) * 16]);
  }
  {  // enc_tail_kernel / qkv_tile_kernel: wave w, group q of 512 rows: base + (s * Cout/16 + q * 32 + 4 w + ni) KB + lane * 16 holds rows
     // (q * 32 + 4 w + ni) * 16 + (lane & 15), bytes s * 64 + (lane >> 4) * 16 of the row-major copy
    const auto f = fragment_order_step_major(rows, Cout, row_bytes);
    const size_t T = (size_t)Cout / 16;
    for (size_t q = 0; q < T / 32; q++)
      for (size_t s2 = 0; s2 < S; s2++)
        for (int wv = 0; wv < 8; wv++)
          for (int ni = 0; ni < 4; ni++)
            for (int l = 0; l < 64; l++)
              bad += !same(&f[(s2 * T + q * 32 + 4 * wv + ni) * 1024 + (size_t)l * 16],
                           &rows[((q * 32 + 4 * wv + ni) * 16 + (l & 15)) * row_bytes + s2 * 64 + (size_t)(l >> 4) * 16]);
  }
  for (int TILE : {256, 128}) {  // gemm_k32_kernel (4 pieces per wave) / conv_halo_kernel (2): row = lane >> 2, swizzled chunk
    const auto pk = pack_stage_w(rows, Cout, row_bytes, TILE);
    const int PW = TILE / 64;
    for (size_t nt = 0; nt < (size_t)Cout / TILE; nt++)
      for (size_t s2 = 0; s2 < S; s2++)
        for (int wv = 0; wv < 4; wv++)
          for (int i = 0; i < PW; i++)
            for (int l = 0; l < 64; l++) {
              const int prow = l >> 2, gch = (l & 3) ^ ((0x78 >> (((prow >> 2) & 3) * 2)) & 3);
              // the kernel: base of (nt, wave) + s2 * (4 waves * PW KB) + i * 1024 + lane * 16
              const size_t at = ((nt * S * 4 + wv) * PW) * 1024 + s2 * (size_t)(4 * PW * 1024) + (size_t)i * 1024 + (size_t)l * 16;
              bad += !same(&pk[at], &rows[(nt * TILE + (size_t)(wv * PW + i) * 16 + prow) * row_bytes + s2 * 64 + (size_t)gch * 16]);
            }
  }
  for (int cfg = 0; cfg < 2; cfg++) {  // conv_big_pp_kernel (256 rows, 8 waves) / conv_deep_kernel, conv_halo8_kernel (128 rows, 4 waves)
    const int TILE = cfg ? 128 : 256, NW = cfg ? 4 : 8;
    const auto pk = pack_stage_w128(rows, Cout, row_bytes, TILE, NW);
    for (size_t nt = 0; nt < (size_t)Cout / TILE; nt++)
      for (size_t kt = 0; kt < KT; kt++)
        for (int wv = 0; wv < NW; wv++)
          for (int i = 0; i < 4; i++)
            for (int l = 0; l < 64; l++) {
              const int srow = l >> 3, g = (l & 7) ^ srow;
              const size_t at = ((nt * KT * NW + wv) * 4096) + kt * (size_t)(NW * 4096) + (size_t)i * 1024 + (size_t)l * 16;
              bad += !same(&pk[at], &rows[(nt * TILE + (size_t)(wv * 4 + i) * 8 + srow) * row_bytes + kt * 128 + (size_t)g * 16]);
              // conv_pp_kernel<128> reads the 128-row form as 8 waves x 2 pieces: piece P = 2 * wave + i at P KB of the (nt, kt) block
              if (cfg && i < 2) {
                for (int w8 = wv * 2; w8 < wv * 2 + 2; w8++) {
                  const size_t at8 = (nt * KT * 16 + (size_t)w8 * 2) * 1024 + kt * 16384 + (size_t)i * 1024 + (size_t)l * 16;
                  bad += !same(&pk[at8], &rows[(nt * 128 + (size_t)(w8 * 2 + i) * 8 + srow) * row_bytes + kt * 128 + (size_t)g * 16]);
                }
              }
            }
  }
  return bad;
}

int fpt_conv(const float *x, const float *w, const float *bias, const float *res, int NB, int H, int W, int Cin, int Cout,
             int KH, int KW, int stride, int pad, int OH, int OW, int relu, int split_imgs, float *out, int iters,
             float *ms_out) {
  return fpt_conv_dt(x, w, bias, res, NB, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, relu, split_imgs, out, iters, ms_out,
                     fp::DT_F16, fp::DT_F16, 1.f, 1.f, 1.f);
}

// qkv f32 [B,T,1536] -> out f32 [B,T,512]; dt = DT_F16 / DT_BF16
int fpt_attention_dt(const float *qkv, int B, int T, float *out, int dt) {
  using namespace fp;
  size_t nq = (size_t)B * T * 1536, no = (size_t)B * T * 512;
  DevBuf<unsigned char> dq(nq * 2), dout(no * 2);
  FP_CHECK(dq.p && dout.p, "fpt_attention: allocation failed");
  auto hq = encode(qkv, nq, dt, 1.f);
  FP_HIP_OK(fp::memcpy_sync(dq.p, hq.data(), nq * 2, hipMemcpyHostToDevice));
  Ctx c{nullptr, nullptr, nullptr};
  if (run_attention(c, dt, plan_attention(B, T, T, heads_override()), dq.p, dout.p)) return 1;
  FP_HIP_OK(hipDeviceSynchronize());
  std::vector<unsigned char> ho(no * 2);
  FP_HIP_OK(fp::memcpy_sync(ho.data(), dout.p, no * 2, hipMemcpyDeviceToHost));
  decode(ho.data(), no, dt, 1.f, out);
  return 0;
}
int fpt_attention(const float *qkv, int B, int T, float *out) { return fpt_attention_dt(qkv, B, T, out, fp::DT_F16); }

// The attention kernels on raw element patterns (tests/test_attention_gpu.py): qkv_bits [B * pitch][1536] and out_bits [B * pitch][512] are
// 2-byte patterns of dt (DT_F16 / DT_BF16).  out_bits is uploaded before the launch and downloaded after it, so what the caller put where
// the kernel does not write (rows T..pitch-1 of a sequence) comes back as it went in.  kernel: -1 = what plan_attention chooses with the
// product's defaults, 0 / 1 = attention32_kernel / attention32_skv_kernel forced, in the product's instantiation and with the launch
// arithmetic of the plan (attention_launch).  info3 = {kernel that ran, query tiles, grid}.  Both device buffers carry ATT_RAW_GUARD guard
// rows in front and behind: quiet NaNs around the input, a canary around the output.  Returns 0, 1 on failure (fp_last_error), 2 when an
// output guard row changed, 3 when an input guard row changed.
static constexpr int ATT_RAW_GUARD = 128;
int fpt_attention_raw(const uint16_t *qkv_bits, int B, int T, int pitch, int dt, int kernel, uint16_t *out_bits, int *info3) {
  using namespace fp;
  FP_CHECK(qkv_bits && out_bits && info3, "fpt_attention_raw: null argument");
  FP_CHECK(dt == DT_F16 || dt == DT_BF16, "fpt_attention_raw: the attention kernels run on 2-byte elements");
  FP_CHECK(kernel >= -1 && kernel <= ATT_32_SKV, "fpt_attention_raw: kernel is -1 (planned), 0 (attention32_kernel) or 1 (attention32_skv_kernel)");
  FP_CHECK(B >= 1 && T >= 1 && pitch >= T && (long long)B * pitch <= (1 << 22), "fpt_attention_raw: invalid shape");
  const AttLaunch a = kernel < 0 ? plan_attention(B, T, pitch, HeadsOverride{}) : attention_launch(kernel, 0, B, T, pitch);
  const size_t G = ATT_RAW_GUARD, rows = (size_t)B * pitch;
  const uint16_t qnan = dt == DT_BF16 ? 0x7FC0 : 0x7E00, canary = 0xA5C3;
  std::vector<uint16_t> hq((rows + 2 * G) * 1536, qnan), ho((rows + 2 * G) * 512, canary);
  std::memcpy(hq.data() + G * 1536, qkv_bits, rows * 1536 * 2);
  std::memcpy(ho.data() + G * 512, out_bits, rows * 512 * 2);
  DevBuf<uint16_t> dq(hq.size()), dout(ho.size());
  FP_CHECK(dq.p && dout.p, "fpt_attention_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dq.p, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dout.p, ho.data(), ho.size() * 2, hipMemcpyHostToDevice));
  Ctx c{nullptr, nullptr, nullptr};
  if (run_attention(c, dt, a, dq.p + G * 1536, dout.p + G * 512)) return 1;
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  std::vector<uint16_t> hq2(hq.size());
  FP_HIP_OK(fp::memcpy_sync(hq2.data(), dq.p, hq2.size() * 2, hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost));
  std::memcpy(out_bits, ho.data() + G * 512, rows * 512 * 2);
  info3[0] = a.kernel; info3[1] = a.nq; info3[2] = (int)a.grid;
  for (size_t i = 0; i < G * 512; i++)
    if (ho[i] != canary || ho[(G + rows) * 512 + i] != canary) { fp::set_error("fpt_attention_raw: the kernel wrote outside its output rows"); return 2; }
  if (hq2 != hq) { fp::set_error("fpt_attention_raw: the input buffer changed"); return 3; }
  return 0;
}

// ---- the tile kernels of the heads on raw operands (tests/test_enc_tail_gpu.py; cases, reference and bounds: tests/enc_tail_cases.py) ----
// Conventions of fpt_attention_raw: device inputs between TILE_RAW_GUARD guard rows of quiet NaNs, outputs between rows of a canary, the inputs
// downloaded again after the launch and compared; returns 0, 1 on failure (fp_last_error), 2 when an output guard changed, 3 when an input
// (or one of its guard rows) changed.
static constexpr int TILE_RAW_GUARD = 128;            // rows of 512 elements
static constexpr uint32_t TILE_RAW_CANARY32 = 0xA5C3A5C3u;
namespace {
// [guard | rows | guard] of `width` 2-byte elements on the device; the host keeps what it uploaded
struct GuardedRows {
  std::vector<uint16_t> host;
  DevBuf<uint16_t> dev;
  size_t rows, width;
  GuardedRows(const uint16_t *bits, size_t rows_, size_t width_, uint16_t fill)
      : host((rows_ + 2 * TILE_RAW_GUARD) * width_, fill), dev(host.size()), rows(rows_), width(width_) {
    std::memcpy(host.data() + TILE_RAW_GUARD * width, bits, rows * width * 2);
  }
  bool upload() { return dev.p && fp::memcpy_sync(dev.p, host.data(), host.size() * 2, hipMemcpyHostToDevice) == hipSuccess; }
  uint16_t *data() const { return dev.p + TILE_RAW_GUARD * width; }
  int changed() const {   // 0 same, 1 changed, -1 the download failed
    std::vector<uint16_t> now(host.size());
    if (fp::memcpy_sync(now.data(), dev.p, now.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return now != host;
  }
};
// f32 parameter blocks in ONE device buffer, TILE_RAW_GUARD * 4 quiet NaNs in front of the first, between any two and behind the last: a read
// past a block lands in NaNs, not in its neighbour.  add() before upload(); at(i) = device address of block i.
struct GuardedF32 {
  static constexpr size_t G = (size_t)TILE_RAW_GUARD * 4;
  std::vector<uint32_t> host = std::vector<uint32_t>(G, 0x7FC00000u);
  std::vector<size_t> off;
  uint32_t *dev = nullptr;
  ~GuardedF32() { if (dev) (void)hipFree(dev); }
  int add(const float *src, size_t n) {
    off.push_back(host.size());
    host.resize(host.size() + n + G, 0x7FC00000u);
    std::memcpy(host.data() + off.back(), src, n * 4);
    return (int)off.size() - 1;
  }
  bool upload() {
    return hipMalloc((void **)&dev, host.size() * 4) == hipSuccess && fp::memcpy_sync(dev, host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  }
  const float *at(int i) const { return reinterpret_cast<const float *>(dev + off[(size_t)i]); }
  int changed() const {
    std::vector<uint32_t> now(host.size());
    if (fp::memcpy_sync(now.data(), dev, now.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return now != host;
  }
};
}  // namespace

// One enc_tail_kernel<dt, MI> problem (MI = 1: 16-token tiles, MI = 5: 80-token tiles) of `tiles` tiles per head, launched P times on the same
// operands -- once per probe set -- through the product's launch site (launch_enc_tail) with the grid and LDS bytes of enc_tail_launch, the
// arithmetic plan_heads uses; one synchronisation.
//   att_bits [2][16 MI tiles][512] (per head) and x_bits [16 MI tiles][512]: 2-byte patterns of dt
//   w [2][3][512][512] f32 (per head: out_proj, lin1, lin2; through finish_layer, so the step-major copy is the loader's), bias [2][3][512],
//   ln_g / ln_b [2][2][512], head_w [P][2][3][512] f32
//   pdot [P][2][tiles][4]: uploaded as given (the caller's canary) and downloaded after the launches: slot 3 of every tile must come back as sent
//   info4 = {MI, tiles, grid, LDS bytes}
int fpt_enc_tail_raw(int dt, int MI, int tiles, const uint16_t *att_bits, const uint16_t *x_bits, const float *w, const float *bias, const float *ln_g,
                     const float *ln_b, const float *head_w, int P, float *pdot, int *info4) {
  using namespace fp;
  FP_CHECK(att_bits && x_bits && w && bias && ln_g && ln_b && head_w && pdot && info4, "fpt_enc_tail_raw: null argument");
  FP_CHECK(dt == DT_F16 || dt == DT_BF16, "fpt_enc_tail_raw: the kernel runs on 2-byte elements");
  FP_CHECK(MI == 1 || MI == 5, "fpt_enc_tail_raw: MI is 1 (16-token tiles) or 5 (80-token tiles)");
  FP_CHECK(tiles >= 1 && tiles <= 5 * MAX_BATCH && P >= 1 && P <= 1024, "fpt_enc_tail_raw: invalid shape");
  HeadsPlan hp;
  enc_tail_launch(MI == 1 ? TAIL_ONE_1 : TAIL_ONE_5, tiles, &hp);
  const size_t rows = (size_t)tiles * 16 * MI, G = TILE_RAW_GUARD;
  const uint16_t qnan = dt == DT_BF16 ? 0x7FC0 : 0x7E00;
  GuardedRows a0(att_bits, rows, EMBED, qnan), a1(att_bits + rows * EMBED, rows, EMBED, qnan), xr(x_bits, rows, EMBED, qnan);
  FP_CHECK(a0.upload() && a1.upload() && xr.upload(), "fpt_enc_tail_raw: allocation failed");
  const size_t np = (size_t)P * 2 * tiles * 4, gp = G * 4;
  std::vector<uint32_t> hp_out(np + 2 * gp, TILE_RAW_CANARY32);
  std::memcpy(hp_out.data() + gp, pdot, np * 4);
  DevBuf<uint32_t> dp(hp_out.size());
  FP_CHECK(dp.p, "fpt_enc_tail_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dp.p, hp_out.data(), hp_out.size() * 4, hipMemcpyHostToDevice));
  Net net;
  net.act_dt = dt;
  ConvLayer L[2][3];
  EncTailParams q{};
  q.x = (const unsigned char *)xr.data();
  q.att[0] = (const unsigned char *)a0.data(); q.att[1] = (const unsigned char *)a1.data();
  q.tiles = tiles;
  q.head_out = 3;
  const size_t WW = (size_t)EMBED * EMBED;
  for (int h = 0; h < 2; h++) {
    for (int i = 0; i < 3; i++) {
      ConvLayer &l = L[h][i];
      l.Cout = l.Cin = EMBED; l.KH = l.KW = 1;
      const float *wp = w + (size_t)(h * 3 + i) * WW, *bp = bias + (size_t)(h * 3 + i) * EMBED;
      FP_CHECK(finish_layer(&net, std::vector<float>(wp, wp + WW), std::vector<float>(bp, bp + EMBED), EMBED, 1, EMBED, dt, &l) && l.wstep, "fpt_enc_tail_raw: weight upload failed");
      q.w[h][i] = l.wstep; q.bias[h][i] = l.bias;
    }
  }
  GuardedF32 par;   // LayerNorm parameters and every (probe set, head) block of read-out rows, NaNs between them (the biases are the loader's uploads)
  for (int j = 0; j < 4; j++) { par.add(ln_g + (size_t)j * EMBED, EMBED); par.add(ln_b + (size_t)j * EMBED, EMBED); }
  for (int j = 0; j < 2 * P; j++) par.add(head_w + (size_t)j * 3 * EMBED, (size_t)3 * EMBED);
  FP_CHECK(par.upload(), "fpt_enc_tail_raw: allocation failed");
  for (int h = 0; h < 2; h++)
    for (int i = 0; i < 2; i++) { q.ln_g[h][i] = par.at(2 * (h * 2 + i)); q.ln_b[h][i] = par.at(2 * (h * 2 + i) + 1); }
  Ctx c{nullptr, nullptr, &net};
  for (int pi = 0; pi < P; pi++) {
    q.head_w[0] = par.at(8 + pi * 2);
    q.head_w[1] = par.at(8 + pi * 2 + 1);
    q.pdot = reinterpret_cast<float *>(dp.p + gp) + (size_t)pi * 2 * tiles * 4;
    launch_enc_tail(c, dt, hp, q);
  }
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  FP_HIP_OK(fp::memcpy_sync(hp_out.data(), dp.p, hp_out.size() * 4, hipMemcpyDeviceToHost));
  std::memcpy(pdot, hp_out.data() + gp, np * 4);
  info4[0] = MI; info4[1] = hp.tail_tiles; info4[2] = (int)hp.tail_grid; info4[3] = hp.tail_lds;
  for (size_t i = 0; i < gp; i++)
    if (hp_out[i] != TILE_RAW_CANARY32 || hp_out[gp + np + i] != TILE_RAW_CANARY32) { fp::set_error("fpt_enc_tail_raw: the kernel wrote outside pdot"); return 2; }
  const int ch[4] = {a0.changed(), a1.changed(), xr.changed(), par.changed()};
  FP_CHECK(ch[0] >= 0 && ch[1] >= 0 && ch[2] >= 0 && ch[3] >= 0, "fpt_enc_tail_raw: download failed");
  if (ch[0] || ch[1] || ch[2] || ch[3]) { fp::set_error("fpt_enc_tail_raw: an input buffer changed"); return 3; }
  return 0;
}

// qkv_tile_kernel<dt> on `tiles` 80-token tiles through the product's launch (run_qkv) with the grid and LDS bytes of qkv_tile_launch.
//   x_bits [80 tiles][512] 2-byte patterns, w [1536][512] f32 and bias [1536] (through finish_layer)
//   out_bits [80 tiles][1536]: uploaded as given and downloaded after the launch;  info3 = {tiles, grid, LDS bytes}
int fpt_qkv_tile_raw(int dt, int tiles, const uint16_t *x_bits, const float *w, const float *bias, uint16_t *out_bits, int *info3) {
  using namespace fp;
  FP_CHECK(x_bits && w && bias && out_bits && info3, "fpt_qkv_tile_raw: null argument");
  FP_CHECK(dt == DT_F16 || dt == DT_BF16, "fpt_qkv_tile_raw: the kernel runs on 2-byte elements");
  FP_CHECK(tiles >= 1 && tiles <= 5 * MAX_BATCH, "fpt_qkv_tile_raw: invalid shape");
  const size_t rows = (size_t)tiles * QKV_TILE_TOKENS;
  HeadsPlan hp;
  qkv_tile_launch((int)rows, &hp);
  GuardedRows xr(x_bits, rows, EMBED, dt == DT_BF16 ? 0x7FC0 : 0x7E00), out(out_bits, rows, 3 * EMBED, 0xA5C3);
  FP_CHECK(xr.upload() && out.upload(), "fpt_qkv_tile_raw: allocation failed");
  Net net;
  net.act_dt = dt;
  ConvLayer L;
  L.Cout = 3 * EMBED; L.Cin = EMBED; L.KH = L.KW = 1;
  FP_CHECK(finish_layer(&net, std::vector<float>(w, w + (size_t)3 * EMBED * EMBED), std::vector<float>(bias, bias + 3 * EMBED), 3 * EMBED, 1, EMBED, dt, &L) && L.wstep,
           "fpt_qkv_tile_raw: weight upload failed");
  Ctx c{nullptr, nullptr, &net};
  if (run_qkv(c, hp, L, xr.data(), (int)rows, out.data())) return 1;
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  std::vector<uint16_t> ho(out.host.size());
  FP_HIP_OK(fp::memcpy_sync(ho.data(), out.dev.p, ho.size() * 2, hipMemcpyDeviceToHost));
  const size_t go = (size_t)TILE_RAW_GUARD * 3 * EMBED;
  std::memcpy(out_bits, ho.data() + go, rows * 3 * EMBED * 2);
  info3[0] = tiles; info3[1] = (int)hp.qkv_grid; info3[2] = hp.qkv_lds;
  for (size_t i = 0; i < go; i++)
    if (ho[i] != 0xA5C3 || ho[go + rows * 3 * EMBED + i] != 0xA5C3) { fp::set_error("fpt_qkv_tile_raw: the kernel wrote outside its output rows"); return 2; }
  const int ch = xr.changed();
  FP_CHECK(ch >= 0, "fpt_qkv_tile_raw: download failed");
  if (ch) { fp::set_error("fpt_qkv_tile_raw: the input buffer changed"); return 3; }
  return 0;
}

// enc_heads_kernel on a caller's pdot [2][n * parts][4] f32 through the product's launch (launch_enc_heads): bias [2][3], tokens.
//   y [2][n][3]: both heads' outputs.  fused == 0: the product's unfused launch -- a pose (pose_io [16]) and a completion flag (flag_io) sit
//   on the device all the same, and what the caller put there must come back.  fused != 0 (n == 1): the kernel applies RefinePostProcess to
//   pose_io [16] (in: the pose, out: the updated pose) with `diameter` and raises the flag; pose_ref [16] = the product's own
//   pose_update launch (launch_pose_update) on the SAME pose and the y the kernel returned.
//   y sits between canary floats on the device, pdot and the biases between quiet NaNs.  Returns 0 / 1 / 2 (a guard of y changed) / 3 (pdot,
//   the biases or a guard of theirs changed).
int fpt_enc_heads_raw(const float *pdot, const float *bias6, int n, int parts, float tokens, int fused, float diameter, float *pose_io, unsigned *flag_io,
                      float *pose_ref, float *y) {
  using namespace fp;
  FP_CHECK(pdot && bias6 && y && pose_io && flag_io && pose_ref, "fpt_enc_heads_raw: null argument");
  FP_CHECK(n >= 1 && n <= MAX_BATCH && parts >= 1 && parts <= 25 && tokens > 0.f && (!fused || n == 1), "fpt_enc_heads_raw: invalid shape");
  const size_t np = (size_t)2 * n * parts * 4, ny = (size_t)2 * n * 3, G = 256;
  std::vector<uint32_t> hy(ny + 2 * G, TILE_RAW_CANARY32);
  DevBuf<float> dpose(32);
  DevBuf<uint32_t> dy(hy.size()), dflag(1);
  GuardedF32 in;   // block 0: pdot, block 1: the biases, quiet NaNs around both
  in.add(pdot, np); in.add(bias6, 6);
  FP_CHECK(dpose.p && dy.p && dflag.p && in.upload(), "fpt_enc_heads_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dy.p, hy.data(), hy.size() * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dpose.p, pose_io, 64, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dpose.p + 16, pose_io, 64, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dflag.p, flag_io, 4, hipMemcpyHostToDevice));
  float *const y0 = reinterpret_cast<float *>(dy.p + G);
  const EncHeadsParams p{in.at(0), {in.at(1), in.at(1) + 3}, {y0, y0 + (size_t)n * 3}, n, parts, 3, tokens};
  const PoseUpdateFuse fuse{dpose.p, diameter, nullptr, nullptr, dflag.p};
  Ctx c{nullptr, nullptr, nullptr};
  launch_enc_heads(c, p, fused ? &fuse : nullptr);
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  if (fused) {   // the product's unfused RefinePostProcess on the other copy of the pose and the y just written
    launch_pose_update(nullptr, dpose.p + 16, y0, y0 + 3, 1, diameter, nullptr, nullptr);
    FP_HIP_OK(hipGetLastError());
    FP_HIP_OK(hipDeviceSynchronize());
  }
  FP_HIP_OK(fp::memcpy_sync(hy.data(), dy.p, hy.size() * 4, hipMemcpyDeviceToHost));
  std::memcpy(y, hy.data() + G, ny * 4);
  FP_HIP_OK(fp::memcpy_sync(pose_io, dpose.p, 64, hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(pose_ref, dpose.p + 16, 64, hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(flag_io, dflag.p, 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < G; i++)
    if (hy[i] != TILE_RAW_CANARY32 || hy[G + ny + i] != TILE_RAW_CANARY32) { fp::set_error("fpt_enc_heads_raw: the kernel wrote outside y"); return 2; }
  const int ch = in.changed();
  FP_CHECK(ch >= 0, "fpt_enc_heads_raw: download failed");
  if (ch) { fp::set_error("fpt_enc_heads_raw: an input buffer changed"); return 3; }
  return 0;
}

// ---- the 8-bit convolutions and their helper kernels on raw bit patterns (tests/test_q8_conv_gpu.py, tests/test_q8_helpers_gpu.py) ----
// One 3x3 / pad-1 convolution of the 8-bit trunk through run_conv, every operand in device form.
//   cfg13 = {Cin, Cout, stride, NB, H (= W), dt, odt, relu, split_imgs, res_kind (0 none, 1 f16, 2 8-bit codes + rscale), opad, rpad, guard_imgs}
//   dt / odt: the pair run_conv dispatches on (fp_nn.h DT_*); the call is refused when run_conv derives another ODT from the operands.
//   x        dt 8-bit: codes [NB, H, H, Cin] (e4m3 bits, or u ^ 0x80); DT_F16 (encodeA.1): f16 bits.  The border of zero-codes is added here.
//   w        f32 [Cout, 3, 3, Cin], bias f32 [Cout], s_in [Cin] (8-bit dt), s_out_fold [Cout] or null: through finish_layer and
//            apply_q8_layer, layout copies included.
//   res      [NB, OH + 2 rpad, OW + 2 rpad, Cout] f16 bits or 8-bit codes, border as the caller filled it; rscale [Cout] (res_kind 2)
//   bias_img [NB][Cout] or null (DT_I8); oinv [Cout] (dual / scaled outputs); post f16 bits [OH * OW][Cout] or null (offered table)
//   out16 / out8: [NBo + guard_imgs][OH + 2 opad][OW + 2 opad][out_ld] 2-byte / 1-byte patterns, NBo = split_imgs ? split_imgs : NB,
//            out_ld = split_imgs ? 2 Cout : Cout.  Uploaded as given (the caller's canary) and downloaded whole after the launch; the one
//            the output type does not write may be null.
//   tables (8-bit dt; each may be null): wq [Cout][9 Cin] the codes quantise_q8 produced, sw [Cout], cscale [Cout] and bias [Cout] as
//            uploaded (read back from the device; DT_I8: with the 128-offset fold), tmat_t [Cin][Cout] (DT_I8)
//   plan26 = {steps, post_fused, then per step {kernel (ConvKernel), m_begin, M, post, grid, mi}} of the plan run_conv executed
// Returns 0, 1 on failure (fp_last_error).
int fpt_conv_q8_raw(const int *cfg13, const void *x, const float *w, const float *bias, const float *s_in, const float *s_out_fold, const void *res,
                    const float *rscale, const float *bias_img, const float *oinv, const uint16_t *post, uint16_t *out16, unsigned char *out8,
                    unsigned char *wq, float *sw, float *cscale, float *bias_up, float *tmat_t, int *plan26) {
  using namespace fp;
  FP_CHECK(cfg13 && x && w && bias && plan26, "fpt_conv_q8_raw: null argument");
  const int Cin = cfg13[0], Cout = cfg13[1], stride = cfg13[2], NB = cfg13[3], H = cfg13[4], dt = cfg13[5], odt = cfg13[6], relu = cfg13[7],
            split = cfg13[8], res_kind = cfg13[9], opad = cfg13[10], rpad = cfg13[11], guard = cfg13[12];
  FP_CHECK((is_q8(dt) || dt == DT_F16) && odt >= 0 && odt <= DT_F16RQ_I8 && odt != DT_BF16 && (is_q8(dt) ? s_in != nullptr : !s_out_fold), "fpt_conv_q8_raw: invalid element types");
  FP_CHECK(Cin >= 64 && Cin % 64 == 0 && Cin <= 512 && Cout >= 128 && Cout % 128 == 0 && Cout <= 512 && (stride == 1 || stride == 2) && NB >= 1 && NB <= 4096 && H >= 2 && H <= 80 &&
               H % 2 == 0 && split >= 0 && split < NB && (split == 0 || NB <= 2 * split) && opad >= 0 && opad <= 1 && rpad >= 0 && rpad <= 1 && guard >= 1, "fpt_conv_q8_raw: invalid shape");
  FP_CHECK(res_kind >= 0 && res_kind <= 2 && (res_kind == 0) == (res == nullptr) && (res_kind == 2) == (rscale != nullptr) && (res_kind == 2) == odt_rq(odt), "fpt_conv_q8_raw: residual arguments do not match the output type");
  FP_CHECK((oinv != nullptr) == (odt_dual(odt) || odt_qs(odt)) && (!post || (odt_16(odt) == DT_F16 && !odt_dual(odt) && opad == 0 && split == 0)) && (!bias_img || dt == DT_I8),
           "fpt_conv_q8_raw: table arguments do not match the output type");
  const int es = elem_bytes(dt), Hp = H + 2, OH = (H + 2 - 3) / stride + 1, OHp = OH + 2 * opad, RHp = OH + 2 * rpad;
  const int NBo = split ? split : NB, out_ld = split ? 2 * Cout : Cout;
  const size_t nx = (size_t)NB * Hp * Hp * Cin * es, nw = (size_t)Cout * 9 * Cin, nout = (size_t)(NBo + guard) * OHp * OHp * out_ld;
  const size_t nres = res ? (size_t)NB * RHp * RHp * Cout * (res_kind == 2 ? 1 : 2) : 0;
  FP_CHECK((out16 != nullptr) == (odt_16(odt) >= 0) && (out8 != nullptr) == (odt_q(odt) >= 0), "fpt_conv_q8_raw: output buffers do not match the output type");
  DevBuf<unsigned char> dx(nx), dres(nres), d16(out16 ? nout * 2 : 0), d8(out8 ? nout : 0), dpost(post ? (size_t)OH * OH * Cout * 2 : 0);
  FP_CHECK(dx.p && dres.p && d16.p && d8.p && dpost.p, "fpt_conv_q8_raw: allocation failed");
  {
    std::vector<unsigned char> hx(nx, dt == DT_I8 ? 0x80 : 0x00);
    const size_t row = (size_t)H * Cin * es;
    for (int n = 0; n < NB; n++)
      for (int y = 0; y < H; y++)
        std::memcpy(&hx[(((size_t)n * Hp + y + 1) * Hp + 1) * Cin * es], (const unsigned char *)x + ((size_t)n * H + y) * row, row);
    FP_HIP_OK(fp::memcpy_sync(dx.p, hx.data(), nx, hipMemcpyHostToDevice));
  }
  if (res) FP_HIP_OK(fp::memcpy_sync(dres.p, res, nres, hipMemcpyHostToDevice));
  if (post) FP_HIP_OK(fp::memcpy_sync(dpost.p, post, (size_t)OH * OH * Cout * 2, hipMemcpyHostToDevice));
  if (out16) FP_HIP_OK(fp::memcpy_sync(d16.p, out16, nout * 2, hipMemcpyHostToDevice));
  if (out8) FP_HIP_OK(fp::memcpy_sync(d8.p, out8, nout, hipMemcpyHostToDevice));
  Net net;
  if (is_q8(dt)) { net.prec = dt == DT_FP8 ? PREC_FP8 : PREC_INT8; net.qdt = dt; }
  ConvLayer L;
  L.Cin = Cin; L.Cout = Cout; L.KH = 3; L.KW = 3; L.stride = stride; L.pad = 1;
  FP_CHECK(finish_layer(&net, std::vector<float>(w, w + nw), std::vector<float>(bias, bias + Cout), Cout, 9, Cin, dt, &L), "fpt_conv_q8_raw: weight upload failed");
  if (is_q8(dt)) {
    if (apply_q8_layer(&net, L, dt, s_in, nullptr, s_out_fold, true)) return 1;
    if (wq || sw) {   // the same quantiser call apply_q8_layer made (no calibration means): the codes in the caller's [Cout][tap][Cin] order
      std::vector<float> hsw, tm; std::vector<double> qs;
      const auto e = quantise_q8(L, dt, s_in, &hsw, &qs, nullptr, 0, dt == DT_I8 ? &tm : nullptr);
      FP_CHECK(hsw == L.q_sw, "fpt_conv_q8_raw: the quantiser is not reproducible");
      if (wq) std::memcpy(wq, e.data(), nw);
      if (sw) std::memcpy(sw, hsw.data(), (size_t)Cout * 4);
    }
    if (cscale) FP_HIP_OK(fp::memcpy_sync(cscale, L.cscale, (size_t)Cout * 4, hipMemcpyDeviceToHost));
    if (bias_up) FP_HIP_OK(fp::memcpy_sync(bias_up, L.bias, (size_t)Cout * 4, hipMemcpyDeviceToHost));
    if (tmat_t && dt == DT_I8) FP_HIP_OK(fp::memcpy_sync(tmat_t, L.tmat_t, (size_t)Cin * Cout * 4, hipMemcpyDeviceToHost));
  }
  float *rscale_dev = nullptr, *oinv_dev = nullptr, *bimg_dev = nullptr;
  if (rscale) { rscale_dev = upload(&net, std::vector<float>(rscale, rscale + Cout)); FP_CHECK(rscale_dev, "fpt_conv_q8_raw: allocation failed"); }
  if (oinv) { oinv_dev = upload(&net, std::vector<float>(oinv, oinv + Cout)); FP_CHECK(oinv_dev, "fpt_conv_q8_raw: allocation failed"); }
  if (bias_img) { bimg_dev = upload(&net, std::vector<float>(bias_img, bias_img + (size_t)NB * Cout)); FP_CHECK(bimg_dev, "fpt_conv_q8_raw: allocation failed"); }
  Ctx c{nullptr, nullptr, &net};
  const int qo = odt_q(odt);
  const Act a16{d16.p, DT_F16, 1.f}, aq{d8.p, qo >= 0 ? qo : DT_I8, 1.f}, ares{dres.p, res_kind == 2 ? DT_I8 : DT_F16, 1.f};
  const bool two = odt_16(odt) >= 0;   // a 2-byte tensor is written (alone, or with its 8-bit copy)
  bool fused = false;
  g_last_conv_plan = ConvPlan{}; g_last_conv_odt = -1;
  ConvArgs g;
  g.in = Act{dx.p, dt, 1.f}; g.NB = NB; g.H = H; g.W = H; g.ipad = 1; g.opad = opad; g.rpad = rpad;
  g.out = two ? a16 : aq; g.relu = relu != 0; g.res = res ? &ares : nullptr; g.split_imgs = split;
  g.post = post ? dpost.p : nullptr; g.post_fused = &fused; g.out2 = odt_dual(odt) ? &aq : nullptr;
  g.oinv = oinv_dev; g.rscale = rscale_dev; g.bias_img = bimg_dev;
  if (run_conv(c, "t", L, g)) return 1;
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  FP_CHECK(g_last_conv_odt == odt, "fpt_conv_q8_raw: run_conv dispatched another output type than the case names");
  if (out16) FP_HIP_OK(fp::memcpy_sync(out16, d16.p, nout * 2, hipMemcpyDeviceToHost));
  if (out8) FP_HIP_OK(fp::memcpy_sync(out8, d8.p, nout, hipMemcpyDeviceToHost));
  const ConvPlan &pl = g_last_conv_plan;
  FP_CHECK(pl.post_fused == fused, "fpt_conv_q8_raw: the recorded plan is not the one that ran");
  std::memset(plan26, 0, 26 * sizeof(int));
  plan26[0] = pl.n; plan26[1] = pl.post_fused ? 1 : 0;
  for (int i = 0; i < pl.n; i++) {
    const ConvStep &st = pl.step[i];
    const int f[6] = {st.kernel, st.m_begin, st.M, st.post ? 1 : 0, (int)st.grid, st.mi};
    std::memcpy(plan26 + 2 + 6 * i, f, sizeof(f));
  }
  return 0;
}

// q8_copy_kernel<qdt> through the product's launch (launch_q8_copy): x16 [imgs][HW + 2][HW + 2][C] f16 bits, q the 1-byte buffer of the same
// shape plus guard_imgs images, uploaded as given and downloaded after the launch; oinv [C].  info2 = {grid, block}.
int fpt_q8_copy_raw(const uint16_t *x16, const float *oinv, int imgs, int HW, int C, int qdt, int guard_imgs, unsigned char *q, int *info2) {
  using namespace fp;
  FP_CHECK(x16 && oinv && q && info2 && is_q8(qdt) && imgs >= 1 && HW >= 1 && C >= 8 && C % 8 == 0 && guard_imgs >= 1, "fpt_q8_copy_raw: invalid arguments");
  const size_t px = (size_t)(HW + 2) * (HW + 2), nin = (size_t)imgs * px * C, nq = (size_t)(imgs + guard_imgs) * px * C;
  DevBuf<uint16_t> dx(nin);
  DevBuf<unsigned char> dq(nq);
  DevBuf<float> doi(C);
  FP_CHECK(dx.p && dq.p && doi.p, "fpt_q8_copy_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dx.p, x16, nin * 2, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dq.p, q, nq, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(doi.p, oinv, (size_t)C * 4, hipMemcpyHostToDevice));
  info2[0] = (int)launch_q8_copy(nullptr, qdt, dx.p, dq.p, doi.p, imgs, HW, C); info2[1] = 256;
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  FP_HIP_OK(fp::memcpy_sync(q, dq.p, nq, hipMemcpyDeviceToHost));
  return 0;
}

// q8_img_bias_fused_kernel through the product's launch (launch_q8_img_bias_fused): xq [n_img][HW + 2][HW + 2][Cin] bytes (u ^ 0x80, border
// included as the caller filled it), tmat_t [Cin][Cout], cscale / bias [Cout]; form 0 = the lattice sums, 1 = every pixel (wp2 = 0),
// 2 = the three-launch form (q8_img_sum_kernel, q8_img_bias_kernel, clear).  out [n_img + guard_imgs][Cout] f32 bit patterns, uploaded as
// given and downloaded after the launch.  info2 = {grid, block} (form 2: of the sum kernel's x dimension).
int fpt_q8_img_bias_raw(const unsigned char *xq, const float *tmat_t, const float *cscale, const float *bias, int n_img, int HW, int Cin, int Cout,
                        int form, int guard_imgs, uint32_t *out, int *info2) {
  using namespace fp;
  FP_CHECK(xq && tmat_t && cscale && bias && out && info2 && n_img >= 1 && (HW == 40 || HW == 20) && Cin >= 128 && Cin <= 512 && Cin % 128 == 0 && Cout >= 128 &&
               Cout <= 512 && Cout % 128 == 0 && form >= 0 && form <= 2 && guard_imgs >= 1, "fpt_q8_img_bias_raw: invalid arguments");
  const size_t nx = (size_t)n_img * (HW + 2) * (HW + 2) * Cin, no = (size_t)(n_img + guard_imgs) * Cout;
  DevBuf<unsigned char> dx(nx);
  DevBuf<float> dt_((size_t)Cin * Cout), dcs(Cout), dbi(Cout);
  DevBuf<uint32_t> dout(no);
  DevBuf<int> dsum((size_t)n_img * Cin);
  FP_CHECK(dx.p && dt_.p && dcs.p && dbi.p && dout.p && dsum.p, "fpt_q8_img_bias_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dx.p, xq, nx, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dt_.p, tmat_t, (size_t)Cin * Cout * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dcs.p, cscale, (size_t)Cout * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dbi.p, bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dout.p, out, no * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memset_sync(dsum.p, 0, (size_t)n_img * Cin * sizeof(int)));
  ConvLayer L;
  L.Cin = Cin; L.Cout = Cout; L.tmat_t = dt_.p; L.cscale = dcs.p; L.bias = dbi.p;
  if (form == 2) { launch_q8_img_bias_3(nullptr, L, dx.p, n_img, HW, dsum.p, (float *)dout.p); info2[0] = n_img; info2[1] = 256; }
  else { info2[0] = (int)launch_q8_img_bias_fused(nullptr, L, dx.p, n_img, HW, form == 0, (float *)dout.p); info2[1] = 1024; }
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  FP_HIP_OK(fp::memcpy_sync(out, dout.p, no * 4, hipMemcpyDeviceToHost));
  if (form == 2) {
    std::vector<int> hs((size_t)n_img * Cin);
    FP_HIP_OK(fp::memcpy_sync(hs.data(), dsum.p, hs.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int v : hs) FP_CHECK(v == 0, "fpt_q8_img_bias_raw: the three-launch form left its sums non-zero");
  }
  return 0;
}

// chan_stats_kernel<dt> through the product's launch (launch_chan_stats): x [pixels][C] raw elements of dt, scale [C] or null;
// amax [C] f32 (null = not collected) and sum [C] 2^-20 fixed point, both uploaded as given (the kernel accumulates into them).
// info2 = {grid, block}: grid * block / (C / 8) threads walk every channel.
int fpt_chan_stats_raw(const void *x, long long pixels, int C, int dt, const float *scale, float *amax, long long *sum, int *info2) {
  using namespace fp;
  FP_CHECK(x && sum && info2 && pixels >= 1 && C >= 8 && C % 8 == 0 && dt >= DT_F16 && dt <= DT_I8, "fpt_chan_stats_raw: invalid arguments");
  const size_t nb = (size_t)pixels * C * elem_bytes(dt);
  DevBuf<unsigned char> dx(nb);
  DevBuf<float> dsc(C), dam(C);
  DevBuf<long long> dsum(C);
  FP_CHECK(dx.p && dsc.p && dam.p && dsum.p, "fpt_chan_stats_raw: allocation failed");
  FP_HIP_OK(fp::memcpy_sync(dx.p, x, nb, hipMemcpyHostToDevice));
  if (scale) FP_HIP_OK(fp::memcpy_sync(dsc.p, scale, (size_t)C * 4, hipMemcpyHostToDevice));
  if (amax) FP_HIP_OK(fp::memcpy_sync(dam.p, amax, (size_t)C * 4, hipMemcpyHostToDevice));
  FP_HIP_OK(fp::memcpy_sync(dsum.p, sum, (size_t)C * 8, hipMemcpyHostToDevice));
  info2[0] = (int)launch_chan_stats(nullptr, dt, dx.p, (size_t)pixels, C, scale ? dsc.p : nullptr, amax ? dam.p : nullptr, dsum.p); info2[1] = 256;
  FP_HIP_OK(hipGetLastError());
  FP_HIP_OK(hipDeviceSynchronize());
  if (amax) FP_HIP_OK(fp::memcpy_sync(amax, dam.p, (size_t)C * 4, hipMemcpyDeviceToHost));
  FP_HIP_OK(fp::memcpy_sync(sum, dsum.p, (size_t)C * 8, hipMemcpyDeviceToHost));
  return 0;
}


// concurrency stress: `nthreads` host threads, each with its own stream and buffers, run the same convolution `iters`
// times and compare every result bit-for-bit with their first one (device-side).  Returns the number of mismatching
// elements summed over all threads (0 = deterministic under contention), negative on failure.
__global__ void fpt_count_diff_kernel(const uint32_t *a, const uint32_t *b, size_t n, unsigned long long *cnt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned local = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) local += a[i] != b[i];
  if (local) atomicAdd(cnt, (unsigned long long)local);
}

long long fpt_conv_stress(int NB0, int H0, int Cin0, int Cout0, int with_res, int iters, int nthreads, int mix) {
  using namespace fp;
  std::vector<long long> bad(nthreads, -1);
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; t++)
    th.emplace_back([&, t]() {
      // mix: odd threads run a different layer (the 256x256-tile kernel on 20x20 maps) next to the first thread's
      int NB = NB0, H = H0, Cin = Cin0, Cout = Cout0;
      if (mix && (t & 1)) { NB = 2 * NB0; H = 20; Cin = 512; Cout = 512; }
      const int Hp = H + 2, Wp = H + 2;
      size_t nx = (size_t)NB * Hp * Wp * Cin, nw = (size_t)Cout * 9 * Cin, nout = (size_t)NB * Hp * Wp * Cout;
      DevBuf<__half> dx(nx), dw(nw), dres(nout), dout(nout), dref(nout);
      DevBuf<float> db(Cout);
      DevBuf<unsigned long long> dcnt(1);
      if (!dx.p || !dw.p || !dres.p || !dout.p || !dref.p || !db.p || !dcnt.p) return;
      uint32_t st = 1234567u + 977u * t;
      auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 65536.0f - 0.5f; };
      std::vector<__half> hx(nx, __float2half(0.f)), hw(nw), hr(nout, __float2half(0.f));
      for (int n = 0; n < NB; n++)
        for (int y = 1; y <= H; y++)
          for (int x = 1; x <= H; x++)
            for (int c = 0; c < Cin; c++) hx[(((size_t)n * Hp + y) * Wp + x) * Cin + c] = __float2half(rnd());
      for (auto &v : hw) v = __float2half(rnd() * 0.05f);
      for (auto &v : hr) v = __float2half(rnd());
      std::vector<float> hb(Cout);
      for (auto &v : hb) v = rnd();
      hipStream_t s;
      if (hipStreamCreate(&s) != hipSuccess) return;
      (void)fp::memcpy_sync(dx.p, hx.data(), nx * 2, hipMemcpyHostToDevice);
      (void)fp::memcpy_sync(dw.p, hw.data(), nw * 2, hipMemcpyHostToDevice);
      (void)fp::memcpy_sync(dres.p, hr.data(), nout * 2, hipMemcpyHostToDevice);
      (void)fp::memcpy_sync(db.p, hb.data(), (size_t)Cout * 4, hipMemcpyHostToDevice);
      (void)fp::memset_sync(dout.p, 0, nout * 2);
      (void)fp::memset_sync(dref.p, 0, nout * 2);
      (void)fp::memset_sync(dcnt.p, 0, 8);
      Net net;
      ConvLayer L;
      L.w = (unsigned char *)dw.p; L.bias = db.p; L.Cin = Cin; L.Cout = Cout; L.KH = 3; L.KW = 3; L.stride = 1; L.pad = 1;
      NNScratch ws;
      Ctx c{s, nullptr, &net, &ws};
      const Act ares{dres.p, DT_F16, 1.f};
      ConvArgs g;
      g.in = Act{dx.p, DT_F16, 1.f}; g.NB = NB; g.H = H; g.W = H; g.ipad = 1; g.opad = 1; g.rpad = 1;
      g.out = Act{dref.p, DT_F16, 1.f}; g.relu = true; g.res = with_res ? &ares : nullptr;
      if (run_conv(c, "t", L, g)) return;
      (void)hipStreamSynchronize(s);
      for (int i = 0; i < iters; i++) {
        g.out.p = dout.p;
        if (run_conv(c, "t", L, g)) return;
        hipLaunchKernelGGL(fpt_count_diff_kernel, dim3(1024), dim3(256), 0, s, (const uint32_t *)dout.p, (const uint32_t *)dref.p,
                           nout / 2, dcnt.p);
      }
      unsigned long long cnt = 0;
      (void)hipMemcpyAsync(&cnt, dcnt.p, 8, hipMemcpyDeviceToHost, s);
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
      bad[t] = (long long)cnt;
    });
  for (auto &x : th) x.join();
  long long tot = 0;
  for (auto b : bad) {
    if (b < 0) return -1;
    tot += b;
  }
  return tot;
}

// LDS canary: workgroups that own `words` dwords of LDS each fill them with a pattern and keep re-checking it while a
// convolution runs on another stream; a non-zero return means some kernel wrote outside its own LDS allocation.
__global__ void fpt_lds_canary_kernel(int words, int spins, unsigned long long *bad) {
  extern __shared__ unsigned canary[];
  const unsigned pat = 0xC0FFEE00u ^ (blockIdx.x * 2654435761u);
  for (int i = threadIdx.x; i < words; i += blockDim.x) canary[i] = pat + i;
  __syncthreads();
  unsigned local = 0;
  for (int r = 0; r < spins; r++) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) local += canary[i] != pat + i;
    __builtin_amdgcn_s_sleep(64);
  }
  if (local) atomicAdd(bad, (unsigned long long)local);
}

long long fpt_lds_canary(int NB, int H, int Cin, int Cout, int iters, int canary_bytes) {
  using namespace fp;
  unsigned long long *dbad = nullptr;
  if (hipMalloc((void **)&dbad, 8) != hipSuccess || fp::memset_sync(dbad, 0, 8) != hipSuccess) return -1;
  std::atomic<int> stop{0};
  std::thread canary([&]() {
    hipStream_t s;
    if (hipStreamCreate(&s) != hipSuccess) return;
    while (!stop.load()) {
      hipLaunchKernelGGL(fpt_lds_canary_kernel, dim3(2048), dim3(64), (size_t)canary_bytes, s, canary_bytes / 4, 200, dbad);
      (void)hipStreamSynchronize(s);
    }
    (void)hipStreamDestroy(s);
  });
  long long rc = fpt_conv_stress(NB, H, Cin, Cout, 1, iters, 1, 0);
  stop.store(1);
  canary.join();
  unsigned long long bad = 0;
  (void)fp::memcpy_sync(&bad, dbad, 8, hipMemcpyDeviceToHost);
  (void)hipFree(dbad);
  return rc < 0 ? rc : (long long)bad;
}

// Inter-kernel visibility under concurrency: every thread owns a stream and a buffer and alternates
//   writer (buf[i] = f(i, iteration))  ->  checker (counts buf[i] != f(i, iteration))
// on it.  Same-stream ordering makes any non-zero count a platform-level visibility failure (stale data from the
// previous iteration), independent of this library's kernels.
__global__ void fpt_vis_write_kernel(float4 *buf, size_t n, unsigned it) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { float v = (float)((i * 7u + it * 13u) & 0xffff); buf[i] = make_float4(v, v + 1.f, v + 2.f, v + 3.f); }
}
__global__ void fpt_vis_check_kernel(const float4 *buf, size_t n, unsigned it, unsigned long long *bad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // gather-style read (like the rasteriser reading vertex attributes): a different workgroup than the writer's
  size_t j = (i * 2654435761ull) % n;
  float v = (float)((j * 7u + it * 13u) & 0xffff);
  float4 x = buf[j];
  if (x.x != v || x.y != v + 1.f || x.z != v + 2.f || x.w != v + 3.f) atomicAdd(bad, 1ull);
}
long long fpt_visibility_stress(int nthreads, int iters, int mbytes) {
  std::vector<long long> bad(nthreads, -1);
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; t++)
    th.emplace_back([&, t]() {
      const size_t n = (size_t)mbytes * (1 << 20) / 16;
      float4 *buf = nullptr;
      unsigned long long *dbad = nullptr;
      hipStream_t s;
      if (hipMalloc((void **)&buf, n * 16) != hipSuccess || hipMalloc((void **)&dbad, 8) != hipSuccess || hipStreamCreate(&s) != hipSuccess) return;
      (void)hipMemsetAsync(dbad, 0, 8, s);
      const unsigned grid = (unsigned)((n + 255) / 256);
      for (int it = 0; it < iters; it++) {
        hipLaunchKernelGGL(fpt_vis_write_kernel, dim3(grid), dim3(256), 0, s, buf, n, (unsigned)(it + 1000 * t));
        hipLaunchKernelGGL(fpt_vis_check_kernel, dim3(grid), dim3(256), 0, s, buf, n, (unsigned)(it + 1000 * t), dbad);
      }
      unsigned long long b = 0;
      (void)hipMemcpyAsync(&b, dbad, 8, hipMemcpyDeviceToHost, s);
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
      (void)hipFree(buf);
      (void)hipFree(dbad);
      bad[t] = (long long)b;
    });
  for (auto &x : th) x.join();
  long long tot = 0;
  for (auto b : bad) {
    if (b < 0) return -1;
    tot += b;
  }
  return tot;
}

// timing hook: random QKV resident in HBM, `iters` launches, returns ms per launch (negative on failure)
float fpt_attention_bench(int B, int T, int iters, int variant) {
  using namespace fp;
  const char *pe = getenv("FPT_QKV_LD");   // row pitch experiment (attention32_kernel only)
  const int ld = pe ? atoi(pe) : 1536;
  size_t nq = (size_t)B * T * ld, no = (size_t)B * T * 512;
  DevBuf<__half> dq(nq), dout(no);
  if (!dq.p || !dout.p) return -1.f;
  std::vector<__half> hq(nq);
  uint32_t st = 12345u;
  for (size_t i = 0; i < nq; i++) { st = st * 1664525u + 1013904223u; hq[i] = __float2half(((st >> 8) & 0xffff) / 65536.0f - 0.5f); }
  if (fp::memcpy_sync(dq.p, hq.data(), nq * 2, hipMemcpyHostToDevice) != hipSuccess) return -1.f;
  Ctx c{nullptr, nullptr, nullptr};
  HeadsOverride ov;
  ov.att_variant = variant;   // (a row of ATT_VARIANTS; any other id times the shipped kernel)
  const AttLaunch att = plan_attention(B, T, T, ov);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  for (int i = 0; i < 3; i++) run_attention(c, DT_F16, att, dq.p, dout.p, ld);
  (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters; i++) run_attention(c, DT_F16, att, dq.p, dout.p, ld);
  (void)hipEventRecord(e1, nullptr);
  float ms = -1.f;
  if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = -(float)iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms / iters;
}

// sustained dense fp16 MFMA rate in TFLOP/s (whole chip, `waves_per_simd` waves on every SIMD); negative on failure
// the same with v_mfma_f32_32x32x16_f16 (4 independent 32x32 accumulators): half the instructions and half the operand reads per flop
__global__ __launch_bounds__(256) void mfma_peak32_kernel(float *out, int iters, int zero_operands, unsigned long long *clk) {
  using fp::h8;
  typedef float f16v __attribute__((ext_vector_type(16)));
  const int lane = threadIdx.x & 63;
  h8 a, b;
  unsigned st = 2654435761u * (unsigned)(blockIdx.x * 256 + threadIdx.x + 1);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    st = st * 1664525u + 1013904223u;
    a[i] = (_Float16)(((st >> 8) & 0xffff) / 65536.0f - 0.5f);
    st = st * 1664525u + 1013904223u;
    b[i] = (_Float16)(((st >> 8) & 0xffff) / 65536.0f - 0.5f);
    if (zero_operands) { a[i] = 0; b[i] = 0; }
  }
  unsigned long long c0 = 0, w0 = 0;
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) { c0 = __builtin_readcyclecounter(); w0 = wall_clock64(); }
  f16v acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc[j]) : "v"(a), "v"(b));
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int e = 0; e < 16; e++) sum += acc[j][e];
  if (sum == 12345.678f) out[lane] = sum;
  if (clk && blockIdx.x == 0 && threadIdx.x == 0) { clk[0] = __builtin_readcyclecounter() - c0; clk[1] = wall_clock64() - w0; }
}

float fpt_mfma_peak(int iters, int waves_per_simd, int zero_operands, double *mhz) {
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return -1.f;
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1.f;
  const int wgs = prop.multiProcessorCount * waves_per_simd;  // 256 threads = one wave per SIMD of a CU
  DevBuf<float> out(64);
  DevBuf<unsigned long long> clk(2);
  hipEvent_t e0, e1;
  if (!out.p || !clk.p || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  const bool big = (zero_operands & 2) != 0;   // bit 1: the 32x32x16 form (same flops per iteration: 4 x 32768 = 8 x 16384)
  zero_operands &= 1;
  if (big) hipLaunchKernelGGL(mfma_peak32_kernel, dim3(wgs), dim3(256), 0, s, out.p, iters / 4, zero_operands, (unsigned long long *)nullptr);
  else hipLaunchKernelGGL(mfma_peak_kernel, dim3(wgs), dim3(256), 0, s, out.p, iters / 4, zero_operands, (unsigned long long *)nullptr);  // warm-up / clock ramp
  (void)hipEventRecord(e0, s);
  if (big) hipLaunchKernelGGL(mfma_peak32_kernel, dim3(wgs), dim3(256), 0, s, out.p, iters, zero_operands, clk.p);
  else hipLaunchKernelGGL(mfma_peak_kernel, dim3(wgs), dim3(256), 0, s, out.p, iters, zero_operands, clk.p);
  (void)hipEventRecord(e1, s);
  float ms = -1.f;
  const bool ok = hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipStreamDestroy(s);
  if (!ok || ms <= 0.f) return -1.f;
  if (mhz) {  // shader clock during the run: cycle counter against the 100 MHz wall clock
    unsigned long long h[2] = {0, 0};
    if (fp::memcpy_sync(h, clk.p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    *mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
  }
  const double flops = (double)wgs * 4.0 * (double)iters * 8.0 * 16384.0;
  return (float)(flops / (ms * 1e-3) / 1e12);
}

}  // extern "C"
