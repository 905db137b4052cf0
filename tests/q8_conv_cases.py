"""The cases of tests/test_q8_conv_gpu.py and the one comparison function they use: which steps of an 8-bit convolution plan run different
code, the smallest batch that reaches each, the input families, the float64 reference and the rule a device result is held to.  The
enumeration asks the library's own plan_conv on the host (fpt_plan_conv); nothing here needs a GPU, and the reference and the comparison
run on whatever device their tensors live on (tests/test_q8_conv_cases_cpu.py: the CPU; tests/test_q8_conv_gpu.py: the GPU).

step_class -- the properties of one STEP of a plan that select code (fp_nn.hip plan_conv / launch_conv_step, fp_nn_conv_kernels.inc
conv_epilogue_px and the kernels' row loops):
  * the layer shape (Cin, Cout, map, stride): K-steps per tap chunk, channel tiles, the stride-2 addressing, the f16 -> 8-bit boundary;
  * the kernel, and for conv_smallx_kernel its <MI> instantiation (16- or 32-pixel tiles; read from the step's LDS bytes);
  * the (dt, odt) instantiation;
  * the residual: none, f16, or 8-bit codes with `rscale` (RQ);
  * the concat: none, own crops (2 N images), one shared crop (N + 1 images: the b-half of image 0 alone is written);
  * the step starts at row 0 or behind another step (m_begin enters every row index);
  * the last tile of the step is ragged (rows % tile height; the halo kernels and the 256x256 rounds only ever get whole tiles);
  * the positional table is fused (POST instantiation);
  * a per-image bias is present (INT8 operands in the 8-bit trunk, plan_trunk: passes of 16 hypotheses and more).
Classified per step, not per plan: "256x256 rounds with nothing left over" first happens at 1024 / 2048 images, but its step is the
same code as the rounds of a plan that has a left-over.  No class's smallest member exceeds 96 images (test_q8_conv_cases_cpu.py).

The accepted space is the one of tests/test_conv_plan_cpu.py (its Planner, TRUNK and pair lists), less the combinations run_conv refuses:
an RQ output type (DT_QSR_I8, DT_F16RQ_I8) reads an 8-bit residual, so it exists for the layers that have a residual only.
"""
import functools
import zlib

import numpy as np
import torch

from test_conv_plan_cpu import F16, FP8, I8, DUAL_FP8, DUAL_I8, QS_FP8, QS_I8, QSR_I8, F16RQ_I8, KERNELS, N_MAX, PAIRS_A1_Q8, PAIRS_Q8, TRUNK

DT_NAME = {F16: "f16", FP8: "fp8", I8: "i8", DUAL_FP8: "dual_fp8", DUAL_I8: "dual_i8", QS_FP8: "qs_fp8", QS_I8: "qs_i8", QSR_I8: "qsr_i8",
           F16RQ_I8: "f16rq_i8"}
TILE_ROWS = {"PP": 256, "DEEP64": 64, "IGEMM128": 128}       # kernels whose last tile can be ragged (conv_smallx_kernel: 16 * MI)
SMALLX_LDS_MI2 = 4 * 3 * 2 * 2048 + 3 * 4 * 2 * 1024         # plan_conv: the LDS bytes of conv_smallx_kernel<2, 4>
IMG_BIAS_MIN_N = 16                                          # plan_trunk (Q8_IMG_BIAS_MIN_N): passes of fewer hypotheses run without the per-image bias
Q8_LAYERS = [ly for ly in TRUNK if ly.name == "encodeA.1" or ly.Cin >= 128]
CLASS_FIELDS = ("layer shape", "kernel", "MI", "dt", "odt", "residual", "concat", "m_begin > 0", "ragged last tile", "table fused", "per-image bias")


def odt_q(odt):
    """the 8-bit type an output type writes, or None (fp_nn.hip odt_q)"""
    return {FP8: FP8, DUAL_FP8: FP8, QS_FP8: FP8, I8: I8, DUAL_I8: I8, QS_I8: I8, QSR_I8: I8}.get(odt)


def odt_16(odt):
    """does the output type write the f16 tensor (fp_nn.hip odt_16)"""
    return odt in (F16, DUAL_FP8, DUAL_I8, F16RQ_I8)


def odt_scaled(odt):
    return odt in (DUAL_FP8, DUAL_I8, QS_FP8, QS_I8, QSR_I8)


def odt_rq(odt):
    return odt in (QSR_I8, F16RQ_I8)


def pairs_of(ly):
    if ly.name == "encodeA.1":
        return list(PAIRS_A1_Q8)
    return [(dt, odt) for dt, odt in PAIRS_Q8 if ly.res or not odt_rq(odt)]


def residual_kind(ly, odt):
    return "none" if not ly.res else "q8" if odt_rq(odt) else "f16"


def has_img_bias(N, dt, odt):
    return dt == I8 and odt in (I8, F16, DUAL_I8, QS_I8) and N >= IMG_BIAS_MIN_N


def offers_table(ly, odt):
    return ly.post and odt in (F16, F16RQ_I8)


def step_classes(P, ly, N, NB, dt, odt):
    """the class of every step of the plan the library makes for layer ly at N hypotheses / NB images"""
    steps, fused, _ = P.plan(ly, NB, dt, odt, N if ly.concat else 0, offers_table(ly, odt))
    concat = "none" if not ly.concat else "own" if NB == 2 * N else "shared"
    out = []
    for st in steps:
        m0, m1, pe, kern, lds = st[3], st[4], st[6], KERNELS[st[7]], st[10]
        mi = 0 if kern != "SMALLX" else 2 if lds == SMALLX_LDS_MI2 else 1
        tile = 16 * mi if kern == "SMALLX" else TILE_ROWS.get(kern, 0)
        out.append(((ly.Cin, ly.Cout, ly.HW, ly.stride), kern, mi, DT_NAME[dt], DT_NAME[odt], residual_kind(ly, odt), concat, m0 > 0,
                    bool(tile) and (m1 - m0) % tile != 0, bool(pe), has_img_bias(N, dt, odt)))
    return out


def accepted_space(n_max=N_MAX):
    """(layer, N, NB) of every 8-bit convolution the trunks can run, as tests/test_conv_plan_cpu.py walks it"""
    for N in range(1, n_max + 1):
        for ly in Q8_LAYERS:
            for NB in (sorted({2 * N, N + 1}) if ly.imgs == "ab" else [N]):
                yield ly, N, NB


def reachable_classes(P, n_max=N_MAX):
    """{class: (NB, N, layer name, dt, odt)} of the smallest member (fewest images) of every class"""
    best = {}
    memo = {}
    for ly, N, NB in accepted_space(n_max):
        for dt, odt in pairs_of(ly):
            # the plan of a layer depends on N only through NB, the split and the per-image bias threshold: ask once per distinct question
            key = (ly.Cin, ly.Cout, ly.HW, ly.stride, ly.res, ly.concat, ly.post, NB, dt, odt, N if ly.concat else 0, has_img_bias(N, dt, odt))
            if key in memo:
                continue
            memo[key] = True
            for c in step_classes(P, ly, N, NB, dt, odt):
                if c not in best or (NB, N) < best[c][:2]:
                    best[c] = (NB, N, ly.name, dt, odt)
    return best


LAYER = {ly.name: ly for ly in Q8_LAYERS}
FAMILIES = ("relu", "dead", "top", "zero_imgs", "cancel", "bias_rows")
# every family on a short fixed list of (layer, N, NB, dt, odt): small-problem kernel, resident halo with an 8-bit residual stream, the concat
# with a shared crop and a per-image bias, 256x256 rounds + a ragged ping-pong left-over, rounds + deep ring writing scaled codes, and the
# fused table behind rounds + deep ring
FAMILY_CASES = [("encodeA.2.conv2", 2, 4, I8, DUAL_I8), ("encodeA.2.conv2", 2, 4, FP8, DUAL_FP8), ("encodeA.2.conv2", 15, 30, I8, QSR_I8),
                ("encodeA.3.conv2", 33, 34, I8, DUAL_I8), ("encodeA.3.conv2", 33, 34, FP8, DUAL_FP8),
                ("encodeAB.0.conv2", 47, 47, I8, F16), ("encodeAB.0.conv2", 47, 47, FP8, F16), ("encodeAB.3.conv2", 84, 84, I8, QS_I8),
                ("encodeAB.4.conv2", 84, 84, I8, F16), ("encodeAB.4.conv2", 84, 84, FP8, F16)]
# per-image bias on a multi-step plan (rounds plus left-over) with a different bias row per image: the rows of FAMILY_CASES at N = 47 / 84 and
# the shared-crop concat at N = 33 carry one (has_img_bias); test_q8_conv_cases_cpu.py holds that


# The smallest member (layer: [(N, NB)]) of every step class of the accepted space, as plan_conv stood when this list was written; every
# (dt, odt) pair of the layer runs at each.  FROZEN on purpose: test_q8_conv_cases_cpu.py enumerates the library's own plan and names every
# class no member of this list reaches -- what a changed threshold of plan_conv produces until the list follows it.
CLASS_MEMBERS = {
    "encodeA.1": [(1, 2), (3, 6), (10, 11), (6, 12), (15, 30)],
    "encodeA.2.conv1": [(1, 2), (3, 6), (10, 11), (6, 12), (16, 17), (17, 18), (30, 60)],
    "encodeA.2.conv2": [(1, 2), (3, 6), (10, 11), (6, 12), (16, 17), (17, 18), (30, 60)],
    "encodeA.3.conv2": [(1, 2), (2, 3), (3, 6), (5, 6), (10, 11), (6, 12), (11, 12), (16, 17), (17, 18), (16, 32), (30, 60), (59, 60)],
    "encodeAB.0.conv1": [(1, 1), (3, 3), (6, 6), (8, 8), (16, 16), (17, 17), (21, 21), (30, 30), (41, 41), (47, 47), (48, 48)],
    "encodeAB.0.conv2": [(1, 1), (3, 3), (6, 6), (8, 8), (16, 16), (17, 17), (21, 21), (30, 30), (41, 41), (47, 47), (48, 48)],
    "encodeAB.2": [(1, 1), (2, 2), (3, 3), (6, 6), (8, 8), (11, 11), (16, 16), (17, 17), (21, 21), (32, 32), (41, 41), (44, 44), (82, 82), (93, 93), (96, 96)],
    "encodeAB.3.conv1": [(1, 1), (2, 2), (3, 3), (6, 6), (8, 8), (16, 16), (17, 17), (21, 21), (32, 32), (41, 41), (44, 44), (82, 82), (93, 93), (96, 96)],
    "encodeAB.3.conv2": [(1, 1), (2, 2), (3, 3), (6, 6), (8, 8), (16, 16), (17, 17), (21, 21), (32, 32), (41, 41), (44, 44), (82, 82), (93, 93), (96, 96)],
    "encodeAB.4.conv2": [(1, 1), (2, 2), (3, 3), (82, 82), (84, 84)],
}


def case_list():
    """[(layer name, N, NB, dt, odt, family)]: CLASS_MEMBERS x the layer's pairs with the plain family, then FAMILY_CASES x FAMILIES"""
    out = [(name, N, NB, dt, odt, "relu") for name, members in CLASS_MEMBERS.items() for N, NB in members for dt, odt in pairs_of(LAYER[name])]
    for name, N, NB, dt, odt in FAMILY_CASES:
        out += [(name, N, NB, dt, odt, fam) for fam in FAMILIES]
    return list(dict.fromkeys(out))


def case_id(case):
    name, N, NB, dt, odt, fam = case
    return f"{name}-N{N}-NB{NB}-{DT_NAME[dt]}-{DT_NAME[odt]}-{fam}"


def covered_classes(P, cases):
    got = set()
    for name, N, NB, dt, odt, _ in cases:
        got.update(step_classes(P, LAYER[name], N, NB, dt, odt))
    return got


# =====================================================================================================================================
# number formats
# =====================================================================================================================================
def _e4m3_table():
    """value of every e4m3 bit pattern (OCP fn: bias 7, no infinities; 0x7f / 0xff are NaN)"""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    v = np.where(b & 0x80, -v, v)
    v[[0x7f, 0xff]] = np.nan
    return v


E4M3 = _e4m3_table()
E4M3_MAX = 448.0


def q_e4m3(x):
    """round a float64 tensor to e4m3 values: to nearest even, saturating (the twin of the library's f32_to_e4m3_bits and of
    tests/test_precision_gpu.py q_e4m3)"""
    a = x.abs().clamp_max(E4M3_MAX)
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -20))).clamp_min(-6.0)     # subnormals share the exponent of the smallest normal
    quantum = torch.exp2(e - 3)
    return torch.sign(x) * (torch.round(a / quantum) * quantum).clamp_max(E4M3_MAX)     # torch.round: half to even


def e4m3_bits(v):
    """bit patterns of an array of exact e4m3 VALUES"""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    bits = np.where(a < 2.0 ** -6, np.rint(a * 512), (e + 7) * 8 + np.rint(a / 2.0 ** e * 8 - 8)).astype(np.uint8)
    return bits | np.where(np.signbit(v), 0x80, 0).astype(np.uint8)


def q_u8(x):
    """the unsigned 8-bit rounding of the epilogues: to nearest even, saturating"""
    return torch.round(x).clamp(0, 255)


def act_values(codes, dt):
    """device bytes of an 8-bit activation tensor -> float64 values in units of the per-channel scale (INT8: the unsigned u)"""
    if dt == I8:
        return (codes ^ 0x80).to(torch.float64)
    return torch.from_numpy(E4M3).to(codes.device)[codes.long()]


# =====================================================================================================================================
# inputs: seeded by (layer, NB, dt, family); everything in device form
# =====================================================================================================================================
C_ACC = 1e-6              # tests/layer_ref.py: the suite's f32 accumulation constant
# The FP8 matrix pipe (v_mfma_f32_16x16x128_f8f6f4) does not sum its 128 products like an f32 fmaf chain: measured against float64 on the
# MI355X over every case of tests/test_q8_conv_gpu.py (its printed table, "accumulation constant needed"), the error beyond the output's own
# rounding reaches 13.5 C_ACC * sum |x w| -- conv_smallx_kernel 13.5, conv_igemm_kernel<128> 8.2, conv_big_pp_kernel 7.5, conv_halo8_kernel
# 6.0, conv_pp_kernel 5.0, conv_deep_kernel<64> 4.9 -- in a handful of outputs per million, and most where one channel sits at 448 in
# every pixel (family "top": the peak; 7.1 without it): an error that follows the LARGEST product of a dot product, not the sum of their
# magnitudes, as a pipe that aligns the products to the largest exponent before adding would make.  The INT8 instantiations of the same
# kernels on the same schedules are exact, so it is the pipe's arithmetic, not the kernels' data movement.  The constant is 1.5 times
# the measured peak; the negative controls of tests/test_q8_conv_cases_cpu.py still fail under it.
C_ACC_FP8 = 20 * C_ACC
U24 = 2.0 ** -24
CAP_CODES = {I8: 5e-4, FP8: 2e-3}     # share of outputs whose interval may hold more than one code
CAP_TIES = 5e-3                       # share of 2-byte outputs that may sit within e of an f16 tie
CANARY16 = 0xFE5A                     # an f16 NaN: no finite input makes a kernel write it


@functools.lru_cache(maxsize=2)
def canary8(n):
    """position-dependent byte pattern (read-only): a kernel's 8-byte store reproduces it by chance once in 2^64"""
    i = np.arange(n, dtype=np.uint32)
    pat = ((i * np.uint32(2654435761)) >> np.uint32(13)).astype(np.uint8)
    pat.setflags(write=False)
    return pat


def quant_scale(amax, dt):
    """per-channel activation scale as net_apply_q8 sets it: dead channels get the floor tensor-|max| / 1024"""
    amax = np.maximum(amax, amax.max() / 1024.0)
    return (amax / 224.0 if dt == FP8 else amax * 1.25 / 255.0).astype(np.float32)


def encode_act(x, s, dt):
    """real activations x (>= 0), per-channel scales -> device bytes"""
    t = x / s
    if dt == I8:
        return (np.clip(np.rint(t), 0, 255).astype(np.uint8)) ^ np.uint8(0x80)
    return e4m3_bits(q_e4m3(torch.from_numpy(t.astype(np.float64))).numpy())


def make_operands(name, NB, dt, family, qo=None):
    """x codes [NB, H, H, Cin] (or f16 bits for encodeA.1), s_in, w [Cout, 3, 3, Cin], bias, and the epilogue tables a case may use;
    qo = the 8-bit type of the output copy (encodeA.1 only: its operands are f16 either way)"""
    ly = LAYER[name]
    qo = dt if qo is None else qo
    assert qo in (FP8, I8) and (dt == F16 or qo == dt)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{NB}/{dt}/{qo}/{family}".encode()))
    Cin, Cout, H, OH = ly.Cin, ly.Cout, ly.HW, ly.out_hw()
    n32 = lambda *s: rng.standard_normal(s, dtype=np.float32)
    x = np.maximum(n32(NB, H, H, Cin), 0) * rng.uniform(0.3, 3.0, Cin).astype(np.float32)       # post-ReLU, channels of different ranges
    w = n32(Cout, 3, 3, Cin) / np.float32(np.sqrt(9 * Cin))
    if dt == FP8:
        # FP8: e carries C_ACC_FP8 * sum |x w|.  With zero-mean weights that is ~0.25 sqrt(K) times the layer's value, and the e4m3 interval of
        # far more than CAP_CODES of the outputs holds two codes.  So the weights get a mean of one standard deviation (84 % positive: sum
        # |x w| is ~1.2 times the value), a gain per output channel, and the activations a smooth gain per pixel, which spreads the values --
        # otherwise nearly constant, a sum of K mostly positive terms -- over a decade: up to ~9, few below 0 (family "cancel" has those).
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="ij")
        ph = rng.uniform(0, 6.28, (NB, 4)).astype(np.float32)
        gain = 0.55 + 0.45 * np.sin(yy[None] * (ph[:, 0, None, None] * 0.05 + 0.1) + ph[:, 1, None, None]) * np.cos(xx[None] * (ph[:, 2, None, None] * 0.05 + 0.1) + ph[:, 3, None, None])
        x *= gain[..., None].astype(np.float32)
        w = (n32(Cout, 3, 3, Cin) + 1) * (rng.uniform(0.5, 3.0, Cout).astype(np.float32) * np.float32(3.0 / (0.66 * 1.65 * 9 * Cin)))[:, None, None, None]
    bias = 0.1 * n32(Cout)
    if family == "dead":
        x[..., 3::8] = 0
    elif family == "zero_imgs":          # all-zero images in the middle of the batch (a single image: its lower half)
        if NB >= 3:
            x[NB // 2:NB // 2 + 2] = 0
        else:
            x[NB - 1, H // 2:] = 0
    elif family == "bias_rows":
        w[1::16] *= np.float32(0.02)
        bias[1::16] = 2.0 + np.abs(n32(len(bias[1::16])))
    elif family not in ("relu", "top", "cancel"):
        raise ValueError(family)
    o = {"layer": ly, "NB": NB, "dt": dt, "family": family, "bias": bias.astype(np.float32)}
    if ly.name == "encodeA.1":
        o["x"] = x.astype(np.float16).view(np.uint16)
        o["s_in"] = None
    else:
        o["s_in"] = quant_scale(x.reshape(-1, Cin).max(0), dt)
        o["x"] = encode_act(x, o["s_in"], dt)
        if family == "top":
            o["x"][..., 7] = 0x7F if dt == I8 else 0x7E        # u = 255 / e4m3 448 in every pixel
        # The INT8 epilogue sees the accumulator of the OFFSET activations and a bias that carries 128 * sw * (sum of the row's codes): with
        # i.i.d. weights that sum is ~sqrt(K) * 20 codes and both terms are ten times the layer's value -- and so is e, which makes the rule
        # vacuous (CAP_TIES).  So every row's folded weights w * s_in sum to a chosen small value: a code sum of N(0, 60), enough for a fold
        # that is off by one code (128 -> 127) to move the value by several f16 ulps (test_q8_conv_cases_cpu.py).
        if dt == I8:
            sv = np.broadcast_to(o["s_in"], (3, 3, Cin)).astype(np.float64)
            wf = w.astype(np.float64) * sv
            target = 60.0 * rng.standard_normal(Cout) * np.abs(wf).reshape(Cout, -1).max(1) / 127.0
            w = (w - ((wf.reshape(Cout, -1).sum(1) - target) / (sv * sv).sum())[:, None, None, None] * sv).astype(np.float32)
    if family == "dead":
        w[5] = 0
    o["w"] = w
    del x
    # coarse enough that no output saturates: the pre-rounding values stay below ~12 (bias_rows: below ~16)
    top = (20.0, 28.0) if family == "bias_rows" else (12.0, 20.0)
    o["s_out"] = (rng.uniform(*top, Cout) / (255.0 if qo == I8 else 224.0)).astype(np.float32)
    o["oinv"] = (np.float32(1) / o["s_out"]).astype(np.float32)
    o["delta_img"] = (0.05 * n32(NB, Cout)).astype(np.float32)                  # a different per-image bias row for every image
    if ly.res:
        r = np.maximum(n32(NB, OH, OH, Cout), 0)
        o["res16"] = r.astype(np.float16)
        o["rscale"] = (r.reshape(-1, Cout).max(0) * 1.25 / 255.0).astype(np.float32)
        o["res8"] = np.clip(np.rint(r / o["rscale"]), 0, 255).astype(np.uint8) ^ np.uint8(0x80)
    if ly.post:
        # a table in [0, 1]: where a negative entry cancels the token the mean-ulp statistic of stage_error is a mean over a few huge ratios
        o["pe"] = (0.5 + 0.5 * np.sin(np.arange(OH * OH, dtype=np.float32)[:, None] * np.exp(-np.arange(Cout, dtype=np.float32) / 60.0)[None, :])).astype(np.float16)
    return o


def quantise(L, o, fold):
    """the tables of the layer as apply_q8_layer uploads them (host arithmetic of the library: fpt_quantise_q8 + the fold of fp_nn.hip):
    wq codes [Cout, 9, Cin], sw, qsum, cscale, bias_up; fold = the consumer's scales are folded in (8-bit output alone)"""
    import ctypes as C
    ly, dt = o["layer"], o["dt"]
    rows = np.ascontiguousarray(o["w"].reshape(ly.Cout, 9, ly.Cin), np.float32)
    if dt == F16:     # encodeA.1: f16 weights, f32 bias, no tables
        return {"w16": rows.astype(np.float16), "fold": False}
    wq, sw = np.zeros(rows.shape, np.uint8), np.zeros(ly.Cout, np.float32)
    L.fpt_quantise_q8.argtypes = [C.c_int] + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3
    assert L.fpt_quantise_q8(dt, rows.ctypes.data, ly.Cout, 9, ly.Cin, o["s_in"].ctypes.data, wq.ctypes.data, sw.ctypes.data) == 0
    qsum = wq.view(np.int8).reshape(ly.Cout, -1).sum(1, dtype=np.int64).astype(np.float64) if dt == I8 else np.zeros(ly.Cout)
    b = o["bias"].astype(np.float64) + (128.0 * sw.astype(np.float64)) * qsum
    c = sw.astype(np.float64)
    if fold:
        inv = 1.0 / o["s_out"].astype(np.float64)
        b, c = b * inv, c * inv
    return {"wq": wq, "sw": sw, "qsum": qsum, "cscale": c.astype(np.float32), "bias_up": b.astype(np.float32), "fold": fold}


# =====================================================================================================================================
# float64 reference (torch, on the device of its inputs)
# =====================================================================================================================================
def conv_sums(o, tab, device, per=8):
    """sum x w and sum |x w| over the 3x3 window in float64 on the de-quantised operands the device holds, in code units
    (INT8: x = the unsigned u, w = the signed code; FP8: e4m3 values; encodeA.1: f16 values) -> [NB, OH, OH, Cout] each"""
    ly, dt = o["layer"], o["dt"]
    s, OH = ly.stride, ly.out_hw()
    if dt == F16:
        wv = torch.from_numpy(tab["w16"].astype(np.float64)).to(device)
    elif dt == I8:
        wv = torch.from_numpy(tab["wq"].view(np.int8).astype(np.float64)).to(device)
    else:
        wv = torch.from_numpy(E4M3[tab["wq"]]).to(device)
    wk = [wv[:, t, :].T.contiguous() for t in range(9)]
    wa = [m.abs() for m in wk]
    a = torch.empty((o["NB"], OH, OH, ly.Cout), dtype=torch.float64, device=device)
    aa = torch.empty_like(a)
    for i in range(0, o["NB"], per):
        xc = torch.from_numpy(o["x"][i:i + per]).to(device)
        xs = xc.view(torch.float16).to(torch.float64) if dt == F16 else act_values(xc, dt)
        xs = torch.nn.functional.pad(xs, (0, 0, 1, 1, 1, 1))
        y = torch.zeros((xs.shape[0], OH, OH, ly.Cout), dtype=torch.float64, device=device)
        ya = torch.zeros_like(y)
        for t in range(9):
            kh, kw = divmod(t, 3)
            xv = xs[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OH - 1) + 1:s, :]
            y += xv @ wk[t]
            ya += xv.abs() @ wa[t]
        a[i:i + per], aa[i:i + per] = y, ya
    return a, aa


def cancelling_residual(o, tab, a, seed=0):
    """family "cancel": a residual that cancels the layer's sum up to N(0, 2) (FP8: N(0, 4)) -- f16 (may be negative) and, clipped at 0, 8-bit codes.
    What is left is noise the convolution has no part in, and no smaller than that: e stays that of the operands that cancelled, so a
    smaller remainder puts every f16 output within e of a tie and two codes into every e4m3 interval (CAP_TIES, CAP_CODES)"""
    g = torch.Generator().manual_seed(zlib.crc32(f"cancel/{o['layer'].name}/{o['NB']}/{o['dt']}/{seed}".encode()))
    t64 = lambda k: torch.from_numpy(np.asarray(k, np.float64)).to(a.device)
    lin = a * t64(tab["sw"]) + t64(o["bias"])
    r = -lin + (2.0 if o["dt"] == I8 else 4.0) * torch.randn(lin.shape, generator=g, dtype=torch.float64).to(a.device)
    o["res16"] = r.to(torch.float16).cpu().numpy()
    rs = t64(o["rscale"])
    o["res8"] = (torch.round(r.clamp_min(0) / rs).clamp(0, 255).to(torch.uint8) ^ 0x80).cpu().numpy()


def expected(o, tab, a, aa, N, odt):
    """the float64 pre-rounding value v and the error e the device may be off by, for output type odt: -> dict
    INT8:  e = 6 * 2^-24 * (|acc * cscale| + |bias| + |bias_img| + |res|), acc the int32 accumulator the epilogue sees and bias as uploaded
           (both carry the 128-offset fold) -- at most five f32 roundings of conv_epilogue_px (cvt, fma, + per-image bias, + residual, x oinv)
           and the f32 rounding of the uploaded tables; the accumulation itself is exact.  The VALUE uses the layer's original f32 bias.
    FP8:   e as above + C_ACC_FP8 * cscale * sum |x w|.      encodeA.1 (f16 operands): C_ACC * (sum |x w| + |bias|), as tests/layer_ref.py."""
    ly, dt, dev = o["layer"], o["dt"], a.device
    t64 = lambda k: torch.from_numpy(np.asarray(k, np.float64)).to(dev)
    bias = t64(o["bias"])
    if dt == F16:
        v = a + bias
        e = C_ACC * (aa + bias.abs())
        e_epi = 3 * U24 * (a.abs() + bias.abs())      # + bias, x oinv, and the conversion
    else:
        cs, bup = t64(tab["cscale"]), t64(tab["bias_up"])
        inv = 1.0 / t64(o["s_out"]) if tab["fold"] else torch.ones_like(cs)
        v = a * cs + bias * inv
        mag = ((a - 128.0 * t64(tab["qsum"])) * cs).abs() + bup.abs()
        if has_img_bias(N, dt, odt):     # the device adds bias_img = f32(bias as uploaded + delta) in place of the bias
            d = t64(o["delta_img"])[:, None, None, :]
            v = v + d
            mag = mag + t64((tab["bias_up"][None, :] + o["delta_img"]).astype(np.float32)).abs()[:, None, None, :]
        if ly.res:
            r = (t64((o["res8"] ^ 0x80)) * t64(o["rscale"])) if odt_rq(odt) else t64(o["res16"])
            v = v + r
            mag = mag + r.abs()
        e = e_epi = 6 * U24 * mag
        if dt == FP8:
            e = e + C_ACC_FP8 * cs * aa
    return {"v": v, "e": e, "e_epi": e_epi, "aw": cs * aa if dt == FP8 else None, "oinv": t64(o["oinv"]) if odt_scaled(odt) else None, "q": odt_q(odt), "two": odt_16(odt),
            "pe": t64(o["pe"].astype(np.float64)) if offers_table(ly, odt) else None}


def bias_img_rows(o, tab):
    """what the caller uploads as ConvParams::bias_img"""
    return (tab["bias_up"][None, :] + o["delta_img"]).astype(np.float32)


# =====================================================================================================================================
# the comparison
# =====================================================================================================================================
def geometry(o, N, odt, guard=1):
    ly = o["layer"]
    split = N if ly.concat else 0
    opad = 0 if ly.post else 1
    OH = ly.out_hw()
    return {"NB": o["NB"], "split": split, "NBo": split or o["NB"], "ld": ly.Cout * (2 if split else 1), "Cout": ly.Cout, "OH": OH, "opad": opad,
            "OHp": OH + 2 * opad, "guard": guard}


def canaries(g):
    """fresh output buffers [NBo + guard, OHp, OHp, ld], all canary"""
    shape = (g["NBo"] + g["guard"], g["OHp"], g["OHp"], g["ld"])
    n = int(np.prod(shape))
    return np.full(shape, CANARY16, np.uint16), canary8(n).reshape(shape).copy()


def _logical(buf, g):
    """device buffer -> (values in the layer's own layout [NB, OH, OH, Cout], mask of the buffer elements the layer must write)"""
    p, OH, C, s, NB = g["opad"], g["OH"], g["Cout"], g["split"], g["NB"]
    inner = buf[:, p:p + OH, p:p + OH, :]
    must = np.zeros(buf.shape, bool)
    mi = must[:, p:p + OH, p:p + OH, :]
    if not s:
        mi[:NB] = True
        return inner[:NB], must
    mi[:s, ..., :C] = True
    mi[:NB - s, ..., C:] = True          # a shared crop (NB = N + 1) writes the b-half of image 0 alone
    return np.concatenate([inner[:s, ..., :C], inner[:NB - s, ..., C:]], 0), must


def _ulp16(t):
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14))) - 10)


def check_outputs(raw16, raw8, ex, g, steps, fused, stage_error, device=None):
    """The one comparison of a device result (raw buffers as downloaded, canary where nothing was written) with the reference `ex`
    (expected()).  steps = [(kernel name, m_begin, M)], fused = the plan added the positional table.
    -> (fails [str], rows [(kernel, form, err / bound or None, mean ulp or None, share)]): a case passes when fails is empty.
      2-byte output: layer_ref.stage_error per step (bound 0.5 ulp + e, exactly 0 behind the ReLU; second_rounding with a fused table), its
                     mean error within BIAS_ULP over the case, and at most CAP_TIES of the outputs within the epilogue term of e (FP8: e
                     without the accumulation term, which is the `acc` of the 2-byte bound only) of an f16 tie;
      8-bit codes:   Q(relu(v - e) oinv) <= code <= Q(relu(v + e) oinv), Q = the type's rounding (RNE, saturating); at most CAP_CODES[type]
                     of the outputs may have an interval of more than one code;
      canaries:      every element the layer owns was written, every other one (borders, guard images, the b-half a shared crop leaves to
                     broadcast_b) still holds the canary."""
    from layer_ref import BIAS_ULP, F16 as LR_F16
    fails, rows = [], []
    v, e = ex["v"], ex["e"]
    dev = v.device
    C = g["Cout"]
    flat = lambda t: t.reshape(-1, C)
    if (raw16 is not None) != ex["two"] or (raw8 is not None) != (ex["q"] is not None):
        return ["the buffers do not match the output type"], rows
    if raw16 is not None:
        got_np, must = _logical(raw16, g)
        wrong = int((raw16[~must] != CANARY16).sum())
        unwritten = int((raw16[must] == CANARY16).sum())
        if wrong:
            fails.append(f"2-byte output: {wrong} elements outside the layer's rows changed (borders / guard images / foreign halves)")
        if unwritten:
            fails.append(f"2-byte output: {unwritten} owned elements were never written")
        got = torch.from_numpy(np.ascontiguousarray(got_np)).to(dev).view(torch.float16).to(torch.float64)
        got = torch.nan_to_num(got, nan=65504.0 * 4)                       # an unwritten element fails the bound, it does not poison the maximum
        c = v.clamp_min(0.0)
        ref = c if not (fused and ex["pe"] is not None) else c + ex["pe"].reshape(1, g["OH"], g["OH"], C)
        sr = c if (fused and ex["pe"] is not None) else None
        tot_bias, n = 0.0, 0
        for kern, m0, m1 in steps:
            sl = slice(m0, m1)
            worst, b = stage_error(flat(got)[sl], flat(ref)[sl], flat(e)[sl], LR_F16, pre=flat(v)[sl], second_rounding=None if sr is None else flat(sr)[sl])
            rows.append((kern, "f16", worst, b, None))
            if ex["aw"] is not None:     # FP8: the accumulation constant this step needs, in units of C_ACC (a measurement, asserted nowhere)
                gs, vs, rs = flat(got)[sl], flat(v)[sl], flat(ref)[sl]
                d = (gs - rs).abs() if sr is not None else torch.where(gs > 0, (gs - vs).abs(), vs.clamp_min(0.0))
                slack = 0.5 * _ulp16(rs) + flat(ex["e_epi"])[sl] + (0.5 * _ulp16(flat(sr)[sl]) if sr is not None else 0.0)
                rows.append((kern, "C needed", float(((d - slack).clamp_min(0.0) / flat(ex["aw"])[sl].clamp_min(1e-300)).max()) / C_ACC, None, None))
            tot_bias, n = tot_bias + b * (m1 - m0), n + (m1 - m0)
            if not worst <= 1.0:
                fails.append(f"{kern} rows [{m0}, {m1}): 2-byte output err / bound = {worst:.3f}")
        if n and not abs(tot_bias / n) <= BIAS_ULP:
            fails.append(f"2-byte output: mean error {tot_bias / n:.4f} ulp")
        u = _ulp16(ref)
        frac = ref.abs() / u
        ties = float((((frac - torch.floor(frac) - 0.5).abs() * u <= ex["e_epi"]) & (v > e)).double().mean())
        rows.append(("all", "f16 ties", None, None, ties))
        if not ties <= CAP_TIES:
            fails.append(f"{ties:.2e} of the 2-byte outputs sit within e of an f16 tie (cap {CAP_TIES:.0e}): the inputs make the bound vacuous")
    if raw8 is not None:
        pat = canary8(raw8.size).reshape(raw8.shape)
        got_np, must = _logical(raw8, g)
        same = raw8 == pat
        wrong = int((~same[~must]).sum())
        unwritten = int(same[must].reshape(-1, 8).all(1).sum()) * 8            # the epilogues store 8 channels at a time
        if wrong:
            fails.append(f"8-bit output: {wrong} bytes outside the layer's rows changed (borders / guard images / foreign halves)")
        if unwritten:
            fails.append(f"8-bit output: {unwritten} owned bytes were never written")
        codes = torch.from_numpy(np.ascontiguousarray(got_np)).to(dev)
        gotv = act_values(codes, ex["q"])
        oinv = ex["oinv"] if ex["oinv"] is not None else torch.ones(C, dtype=torch.float64, device=dev)
        Q = q_u8 if ex["q"] == I8 else q_e4m3
        lo, hi = Q((v - e).clamp_min(0.0) * oinv), Q((v + e).clamp_min(0.0) * oinv)
        bad = ~((gotv >= lo) & (gotv <= hi))                                   # (a NaN code is bad)
        for kern, m0, m1 in steps:
            nb = int(flat(bad)[m0:m1].sum())
            rows.append((kern, "codes", float(nb), None, None))
            if nb:
                i = int(torch.nonzero(flat(bad)[m0:m1].any(1))[0]) + m0
                fails.append(f"{kern} rows [{m0}, {m1}): {nb} codes outside [Q(v - e), Q(v + e)], first in row {i}")
        share = float((lo != hi).double().mean())
        sat = float((hi >= (255.0 if ex["q"] == I8 else E4M3_MAX)).double().mean())
        rows.append(("all", "ambiguous", None, None, share))
        rows.append(("all", "saturated", None, None, sat))
        if not share <= CAP_CODES[ex["q"]]:
            fails.append(f"{share:.2e} of the codes have an interval of more than one code (cap {CAP_CODES[ex['q']]:.0e}): the inputs make the rule vacuous")
    return fails, rows


def ideal_outputs(ex, g, fused):
    """the buffers a correct device would return (every rounding done once, in float64): for the CPU tests of check_outputs"""
    raw16, raw8 = canaries(g)
    v = ex["v"]
    c = v.clamp_min(0.0)
    p, OH, C, s, NB = g["opad"], g["OH"], g["Cout"], g["split"], g["NB"]

    def place(buf, val):
        inner = buf[:, p:p + OH, p:p + OH, :]
        if not s:
            inner[:NB] = val
        else:
            inner[:s, ..., :C] = val[:s]
            inner[:NB - s, ..., C:] = val[s:]
    if ex["two"]:
        h = c.to(torch.float16)
        if fused and ex["pe"] is not None:
            h = (h.to(torch.float64) + ex["pe"].reshape(1, OH, OH, C)).to(torch.float16)
        place(raw16, h.cpu().numpy().view(np.uint16))
    if ex["q"] is not None:
        t = c * (ex["oinv"] if ex["oinv"] is not None else 1.0)
        if ex["q"] == I8:
            codes = q_u8(t).to(torch.uint8).cpu().numpy() ^ np.uint8(0x80)
        else:
            codes = e4m3_bits(q_e4m3(t).cpu().numpy())
        place(raw8, codes)
    return (raw16 if ex["two"] else None), (raw8 if ex["q"] is not None else None)
