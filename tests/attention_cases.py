"""The cases of tests/test_attention_gpu.py: which (B, T, pitch) run different code in the two attention kernels, the input families and
the case list.  Pure Python + torch on the CPU: nothing here loads the library, so tests/test_attention_cases_cpu.py can hold the list to
the library's own plan (fpt_plan_heads) without a GPU.

att_class -- derived from fp_nn_attention_kernels.inc, nkb = ceil(T / 32) key blocks:

attention32_kernel (128 query rows per workgroup, every wave walks ALL key blocks; tile t travels in register set t % 3)
  * min(nkb, 5): the prologue requests tiles 1, 2, 3 under `nkb > 1 / 2 / 3`; block kb stores tile kb + 1 (`kb + 1 < nkb`) after
    wait_tile(min(2, nkb - 2 - kb)) and requests tile kb + 4 (`kb + 4 < nkb`).  1 block: no reload at all; 2, 3, 4: only the up-front
    loads, drained with vmcnt 0 / 2 NJ / 4 NJ first; >= 5: the first in-loop load_tile.
  * nkb % 3 (from 5 blocks on): the loop is unrolled three ways over the register sets, so this picks the tail (`kb + 1 < nkb`,
    `kb + 2 < nkb`) and the set that carries the last tile.
  * T % 32 != 0: the -inf mask of the last block (rows past T are clamped to T - 1 on load, so the mask alone keeps them out).
  * idle waves of the last query tile (0..3): a wave with q0 >= T only stages, skips QK / softmax / PV and returns before the store.
  * nq > 1, B > 1: the (tile, head, sequence) decomposition of the workgroup index;  pitch != T: sequence stride against length.
attention32_skv_kernel (32 query rows per workgroup, wave w owns key blocks w, w + 4, ...; private double buffers; four-way merge)
  * (nkb - 1) % 4: the wave that owns the last, possibly masked, block.
  * min(ceil(nkb / 4), 3) blocks on the busiest wave: 1 = no re-issue inside the loop, 2 = the second buffer, 3 = a buffer reused.
  * nkb < 4: waves without a block enter the merge with m = -inf, l = 0.
  * T % 32 != 0, nq > 1, B > 1, pitch != T as above.
both, found while reading the code:
  * grid % 8 != 0: the XCD remap takes its `xcd < r` branch only when the grid is no multiple of 8 (grids are multiples of 4).
"""
import math
import zlib

import numpy as np
import torch

F16, BF16 = 0, 1                       # fp_nn.h DT_*
ATT_32, ATT_SKV = 0, 1                 # fp_nn.hip AttKernel
N_MAX = 2377                           # FP_MAX_BATCH
SHARDS_MAX = 8                         # a sharded Register gathers up to 8 x FP_MAX_BATCH hypotheses in front of the cross-attention
SEQ_TOKENS, TRACK_PITCH = 400, 512
# the thresholds of plan_attention, restated (test_attention_cases_cpu.py holds them to the library)
ATT_QROWS, ATT_SKV_QROWS, ATT_SKV_MAX_WGS, ATT_SKV_MIN_T, HEADS, HDIM, EMBED = 128, 32, 64, 32, 4, 128, 512
TORCH_DT = {F16: torch.float16, BF16: torch.bfloat16}
QNAN = {F16: 0x7E00, BF16: 0x7FC0}
FAMILIES = ("gauss", "ramp", "onehot", "lastkey", "offset")


def planned_kernel(B, T):
    """plan_attention's choice with the product's defaults"""
    return ATT_SKV if -(-T // ATT_QROWS) * HEADS * B <= ATT_SKV_MAX_WGS and T > ATT_SKV_MIN_T else ATT_32


def launch_shape(kernel, B, T):
    """(query tiles, grid) of attention_launch"""
    nq = -(-T // (ATT_SKV_QROWS if kernel == ATT_SKV else ATT_QROWS))
    return nq, nq * HEADS * B


def att_class(kernel, B, T, pitch):
    """the tuple of properties that select different code paths (module docstring)"""
    nkb = -(-T // 32)
    nq, grid = launch_shape(kernel, B, T)
    common = (T % 32 != 0, nq > 1, B > 1, pitch != T, grid % 8 != 0)
    if kernel == ATT_32:
        idle = 4 - -(-(T - (nq - 1) * ATT_QROWS) // 32)
        return ("attention32", min(nkb, 5), nkb % 3 if nkb >= 5 else -1, idle) + common
    return ("attention32_skv", (nkb - 1) % 4, min(-(-nkb // 4), 3), nkb < 4) + common


CLASS_FIELDS = {"attention32": ("kernel", "min(nkb, 5)", "nkb % 3", "idle waves", "T % 32 != 0", "nq > 1", "B > 1", "pitch != T", "grid % 8 != 0"),
                "attention32_skv": ("kernel", "(nkb - 1) % 4", "min(ceil(nkb / 4), 3)", "nkb < 4", "T % 32 != 0", "nq > 1", "B > 1", "pitch != T",
                                    "grid % 8 != 0")}


def accepted_space():
    """every attention launch of the product: (pass, N, (B, T, pitch)) -- the refiner (Track = both heads grouped at pitch 512) and the scorer's
    feature pass at N = 1..FP_MAX_BATCH, the cross-attention over the hypotheses of up to 8 shards"""
    for N in range(1, N_MAX + 1):
        yield 0, N, ((2, SEQ_TOKENS, TRACK_PITCH) if N == 1 else (N, SEQ_TOKENS, SEQ_TOKENS))
        yield 1, N, (N, SEQ_TOKENS, SEQ_TOKENS)
    for N in range(1, SHARDS_MAX * N_MAX + 1):
        yield 2, N, (1, N, N)


def smallest_per_class(space):
    """{class: (pass, N, (B, T, pitch))} of the smallest member of every class; space yields (pass, N, (B, T, pitch), kernel)"""
    best = {}
    for pas, N, shape, kernel in space:
        c = att_class(kernel, *shape)
        key = (shape[0] * shape[1], shape[0], shape[2])
        if c not in best or key < best[c][0]:
            best[c] = (key, pas, N, shape)
    return {c: v[1:] for c, v in best.items()}


def reachable_classes():
    return smallest_per_class((p, N, s, planned_kernel(s[0], s[1])) for p, N, s in accepted_space())


def _cases():
    out = []
    # (a) the smallest member of every reachable class, the product's path, both element types
    for c, (_, _, (B, T, pitch)) in sorted(reachable_classes().items(), key=lambda kv: (kv[0][0], kv[1][2][0] * kv[1][2][1], kv[1][2])):
        for dt in (F16, BF16):
            out.append((B, T, pitch, dt, -1, "gauss"))
    # (b) every family on a fixed list: attention32_kernel at 2 and 4 key blocks on the product's path (17 sequences: more than 64 workgroups),
    # Track's grouped launch, a refiner batch, both sides of both kernel switches, the largest batch, the largest masked tails, two shards
    for B, T, pitch in [(17, 33, 33), (17, 97, 97), (2, 400, 512), (5, 400, 400), (1, 32, 32), (1, 33, 33), (1, 2048, 2048), (1, 2049, 2049),
                        (1, 2058, 2058), (1, 2352, 2352), (1, 2377, 2377), (1, 4754, 4754)]:
        for dt in (F16, BF16):
            for fam in FAMILIES:
                out.append((B, T, pitch, dt, -1, fam))
    # (c) the ground either kernel would take over if a threshold were retuned
    out += [(1, T, T, dt, ATT_32, "gauss") for T in (33, 64, 65, 96, 97, 128, 129, 160, 161) for dt in (F16, BF16)]
    out += [(1, T, T, dt, ATT_SKV, "gauss") for T in (1, 31, 32, 2049) for dt in (F16, BF16)]
    return list(dict.fromkeys(out))


CASES = _cases()


def case_id(case):
    B, T, pitch, dt, kernel, fam = case
    return f"{fam}-B{B}-T{T}-p{pitch}-{'bf16' if dt == BF16 else 'f16'}-{('plan', 'att32', 'skv')[kernel + 1]}"


def expected_kernel(case):
    B, T, _, _, kernel, _ = case
    return planned_kernel(B, T) if kernel < 0 else kernel


# The mean signed error of a stage is asserted from 16384 output elements on.  At that size it is NOT yet the mean of many half-ulp roundings:
# where |ref| is below acc the error of the rounded P (up to ~acc) is hundreds of ulps of |ref| + acc, and the few dozen such elements of a
# [32, 512] output move the mean by ~0.04 ulp whatever the kernel does (the plain emulation of the kernels' arithmetic: -0.068 ulp on one
# f16 gauss draw at T = 32, +0.042 on one at T = 33).  So a case below BIAS_POOL_ELEMS elements repeats its launch on further draws of the
# same family until that many elements are pooled (at most 16 draws); every draw is held to the per-element bound, the pooled mean to the
# limit.  Over 262144 elements the emulation's mean stays within 0.015 ulp.
BIAS_MIN_ELEMS, BIAS_POOL_ELEMS = 16384, 262144


def n_draws(B, T):
    n = B * T * EMBED
    return 1 if n < BIAS_MIN_ELEMS else -(-BIAS_POOL_ELEMS // n)


def make_inputs(B, T, dt, family, draw=0):
    """-> (qkv [B, T, 1536] in the element type, perm [B, T] or None): seeded by the arguments, rounded to the element type.
    The four heads of a token share nothing but the token: every head has its own 128 channels of q, k and v."""
    rng = np.random.default_rng(zlib.crc32(f"{family}/{B}/{T}/{dt}/{draw}".encode()))
    n = lambda *s: rng.standard_normal(s)
    q, k, v = n(B, T, EMBED), n(B, T, EMBED), 1.5 * n(B, T, EMBED)
    perm = None
    if family == "gauss":          # i.i.d. inputs; one spiked query row moves the running maximum late
        q, k = 1.5 * q, 1.5 * k
        q[0, T // 2] *= 4
    elif family == "ramp":         # scores grow by 12 (natural units) from the first key to the last: every key block raises the maximum
        q = 0.5 * q + 1
        k = 0.5 * k + (12 / math.sqrt(HDIM)) * (np.arange(T) / T)[None, :, None]
    elif family == "onehot":       # query i matches key perm(i) alone: 6 * 128 / sqrt(128) = 68 against |N(0, 6)| for every other key
        k = rng.integers(0, 2, (B, T, EMBED)) * 2.0 - 1.0
        perm = np.stack([rng.permutation(T) for _ in range(B)])
        q = 6 * np.take_along_axis(k, perm[:, :, None], 1)
    elif family == "lastkey":      # a near-uniform softmax over small values, the last key's value towers over their mean
        q, v = 0.05 * q, 0.25 * v / 1.5
        v[:, T - 1] = 64
    elif family == "offset":       # a common-mode score of 16 * 128 / sqrt(128) = 181 under a spread of ~2
        q, k = 0.25 * q + 4, 0.25 * k + 4
    else:
        raise ValueError(family)
    x = torch.from_numpy(np.concatenate([q, k, v], -1)).to(TORCH_DT[dt])
    return x, (None if perm is None else torch.from_numpy(perm))


def split_heads(x):
    """[B, T, 1536] -> q, k, v [B, 4, T, 128]"""
    B, T, _ = x.shape
    y = x.reshape(B, T, 3, HEADS, HDIM).permute(2, 0, 3, 1, 4)
    return y[0], y[1], y[2]


def plain_attention(q, k, v):
    """softmax(q k^T / sqrt(128)) v in float64 for any number of keys: [.., Tq, 128], [.., Tk, 128] x 2 -> [B, Tq, 512]"""
    q, k, v = q.double(), k.double(), v.double()
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(HDIM), -1) @ v
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], EMBED)


def emulate_kernel(x):
    """the kernels' arithmetic, plainly: 32-key blocks, an f32 online softmax in base 2 on the raw f32 scores (p = exp2(fma(s, c, -m c)),
    c = log2(e) / sqrt(128)), the row sum over the UNROUNDED p, P rounded to the element type before the f32 PV product, the output
    rounded once.  -> [B, T, 512] in the element type of x"""
    q, k, v = (t.float() for t in split_heads(x))
    B, H, T, _ = q.shape
    c = np.float32(0.08838834764831845) * np.float32(1.4426950408889634)
    c32, c64 = torch.tensor(c, dtype=torch.float32), float(c)
    m = torch.full((B, H, T, 1), -math.inf)
    l = torch.zeros((B, H, T, 1))
    o = torch.zeros((B, H, T, HDIM))
    for k0 in range(0, T, 32):
        s = q @ k[:, :, k0:k0 + 32].transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        mc = m_new * c32
        alpha = torch.exp2(m * c32 - mc)
        p = torch.exp2((s.double() * c64 - mc.double()).float())     # one rounding, like the fma
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(x.dtype).float() @ v[:, :, k0:k0 + 32]
        m = m_new
    return (o * (1.0 / l)).permute(0, 2, 1, 3).reshape(B, T, EMBED).to(x.dtype)
