"""Float64 reference of every stage of the refine-net / score-net, fed the exact tensors the device stage received.

Weights come from the .fpw the device loaded (weights.read_fpw: BatchNorm already folded) and are rounded to the device element type
(f16 / bf16, round to nearest even) like the library rounds them; biases, LayerNorm parameters and the f32 GEMV weights stay f32.
`dt=None` switches every rounding off: the stages then chain into the float64 network (tests/test_layer_ref_cpu.py holds that chain to
oracle/nets_torch.py).  Stages that the device stores in the element type are rounded at the same place.

Each stage returns (ref, acc): the tests compare a device tensor with the UNROUNDED value (out_dt=None), whose distance to the device
result is at most half an ulp plus the accumulation error.  `acc` is the accumulation term of the error bound, C_ACC * (sum |x * w| + |bias| + |residual|) for a
matmul-shaped stage.  C_ACC = 1e-6: the f32 MFMA accumulation figure of cdna_hip_programming.md section 3 is ~1.5e-7 * sum|a*b| at
K <= 1024 and 3.5e-7 at K = 4096 (a k-ordered fmaf chain); the trunk has K up to 4608 and split-K partial sums add one more rounding
per slice, so the bound takes about 3x the K = 4096 figure.  Convolutions are plain shifted [rows, Cin] @ [Cin, Cout] products in
float64 (no MIOpen), chunked over images.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from foundationpose_cpp_amd import weights as W

F16, BF16 = 0, 1
C_ACC = 1e-6
C_LN = 1e-5       # LayerNorm with f32 statistics over 512 channels: relative error of (x - mean) * rstd, ~sqrt(512) f32 ulps, with margin
EMBED, HEADS = 512, 4
TORCH_DT = {F16: torch.float16, BF16: torch.bfloat16}
MANT = {F16: 10, BF16: 7}
MIN_EXP = {F16: -14, BF16: -126}
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8}    # unit roundoff


def rnd(t, dt):
    """round a float64 tensor to the element type (RNE) and back; dt None = no rounding"""
    return t if dt is None else t.to(TORCH_DT[dt]).to(torch.float64)


def ulp(t, dt):
    """spacing of the element type at |t| (subnormal spacing below the smallest normal)"""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** MIN_EXP[dt])))
    return torch.exp2(e - MANT[dt])


BIAS_ULP = 0.05   # mean signed error of a stage, in ulps (truncation instead of RNE would be ~0.5)


def stage_error(got, ref, acc, dt, pre=None, second_rounding=None):
    """a stage stored in the element type against its UNROUNDED float64 reference: -> (worst |got - ref| / bound over the elements, mean
    signed error in ulps of |ref| + acc), bound = 0.5 ulp(|ref| + acc) + acc.  pre: the reference before a ReLU (where it is below -acc
    the output must be exactly 0); second_rounding: a value that was rounded once more on the way (adds its half ulp)."""
    bound = 0.5 * ulp(ref.abs() + acc, dt) + acc
    if second_rounding is not None:      # ref = rnd(c + pe) with c itself rounded first
        bound = bound + 0.5 * ulp(second_rounding.abs() + acc, dt)
    if pre is not None:
        bound = torch.where(pre <= -acc, torch.zeros_like(bound), bound)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), float(((got - ref) / ulp(ref.abs() + acc, dt)).mean())


def pos_table():
    """PositionalEmbedding(512, 400) in f32, as the library's host code builds it"""
    t = np.arange(400, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, EMBED, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / EMBED))).astype(np.float32)
    pe = np.zeros((400, EMBED), np.float32)
    pe[:, 0::2] = np.sin(t * div)
    pe[:, 1::2] = np.cos(t * div)
    return pe


TRUNK = [  # (fpw prefix, stride, residual activation or None); activation i + 1 = layer i of this list, applied to activation i
    ("encodeA.1", 2, None),
    ("encodeA.2.conv1", 1, None), ("encodeA.2.conv2", 1, 1), ("encodeA.3.conv1", 1, None), ("encodeA.3.conv2", 1, 3),
    ("encodeAB.0.conv1", 1, None), ("encodeAB.0.conv2", 1, 5), ("encodeAB.1.conv1", 1, None), ("encodeAB.1.conv2", 1, 7),
    ("encodeAB.2", 2, None),
    ("encodeAB.3.conv1", 1, None), ("encodeAB.3.conv2", 1, 10), ("encodeAB.4.conv1", 1, None), ("encodeAB.4.conv2", 1, 12),
]


class Weights:
    def __init__(self, fpw_path: str, dt, device="cpu"):
        self.st = W.read_fpw(fpw_path)
        self.dt, self.device = dt, device

    def w(self, name):       # element-type weight (what the MFMA operand holds)
        a = torch.from_numpy(self.st[name])
        if self.dt is not None:
            a = a.to(TORCH_DT[self.dt])
        return a.to(self.device, torch.float64)

    def f(self, name):       # f32 parameter
        return torch.from_numpy(self.st[name]).to(self.device, torch.float64)


def _chunks(n, per):
    for i in range(0, n, per):
        yield slice(i, min(n, i + per))


def conv3x3(w: Weights, prefix, x, stride, res=None, relu=True, out_dt="same", per=16):
    """x [NB, H+2, W+2, Cin] with its zero border (the device tensor) -> (ref, acc, pre) [NB, OH, OW, Cout]; res [NB, OH, OW, Cout].
    pre = the value before ReLU (ref of ReLU-zero checks)."""
    dt = w.dt if out_dt == "same" else out_dt
    wt = w.w(prefix + ".weight")            # [Cout, Cin, 3, 3]
    b = w.f(prefix + ".bias")
    NB, Hp, Wp, Cin = x.shape
    OH, OW = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    taps = [(kh, kw) for kh in range(3) for kw in range(3)]
    wk = [wt[:, :, kh, kw].T.contiguous() for kh, kw in taps]
    wa = [m.abs() for m in wk]
    out = torch.empty((NB, OH, OW, wt.shape[0]), dtype=torch.float64, device=x.device)
    acc = torch.empty_like(out)
    for sl in _chunks(NB, per):
        xs = x[sl].to(torch.float64)
        y = torch.zeros((xs.shape[0], OH, OW, wt.shape[0]), dtype=torch.float64, device=x.device)
        a = torch.zeros_like(y)
        for (kh, kw), m, ma in zip(taps, wk, wa):
            xv = xs[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride, :]
            y += xv @ m
            a += xv.abs() @ ma
        out[sl], acc[sl] = y, a
    out += b
    acc += b.abs()
    if res is not None:
        out += res
        acc += res.abs()
    pre = out
    if relu:
        out = out.clamp_min(0.0)
    return rnd(out, dt), C_ACC * acc, pre


def stem(w: Weights, nn_in, per=16):
    """encodeA.0 as the 7x7 / stride-2 / pad-3 convolution of the 6-channel crops recovered from nn_in [NB, 84, 84, 32] (space-to-depth
    2x2 of [NB, 160, 160, 8] with a border of 2) -> (ref, acc, pre) [NB, 80, 80, 64]"""
    NB = nn_in.shape[0]
    wt = w.w("encodeA.0.weight")            # [64, 6, 7, 7]
    b = w.f("encodeA.0.bias")
    wm = wt.permute(2, 3, 1, 0).reshape(49 * 6, 64)     # [(kh, kw, c), co]
    out = torch.empty((NB, 80, 80, 64), dtype=torch.float64, device=nn_in.device)
    acc = torch.empty_like(out)
    for sl in _chunks(NB, per):
        s2d = nn_in[sl, 2:82, 2:82, :].to(torch.float64).reshape(-1, 80, 80, 2, 2, 8)      # [n, y, x, dy, dx, c]
        img = s2d.permute(0, 1, 3, 2, 4, 5).reshape(-1, 160, 160, 8)[..., :6]
        img = torch.nn.functional.pad(img, (0, 0, 3, 3, 3, 3))
        cols = torch.stack([img[:, kh:kh + 159:2, kw:kw + 159:2, :] for kh in range(7) for kw in range(7)], 3).reshape(-1, 80, 80, 49 * 6)
        out[sl] = cols @ wm
        acc[sl] = cols.abs() @ wm.abs()
    out += b
    acc += b.abs()
    return rnd(out.clamp_min(0.0), w.dt), C_ACC * acc, out


def interior(t):
    return t[:, 1:-1, 1:-1, :]


def concat_ab(full, N, n_b):
    """the last encodeA conv over NB2 = N + n_b images -> the a|b concat [N, ..., 2C] (n_b = 1: the shared observed crop)"""
    b = full[N:] if n_b == N else full[N:N + 1].expand(N, *full.shape[1:])
    return torch.cat([full[:N], b], -1)


def tokens(w: Weights, x13, res12, pe, per=16):
    """the last trunk conv (encodeAB.4.conv2, ReLU) + the positional table -> (ref, acc, conv part) [N, 400, 512]; pe [400, 512]"""
    y, acc, pre = conv3x3(w, "encodeAB.4.conv2", x13, 1, res=res12, relu=True, out_dt=None, per=per)
    N = y.shape[0]
    y, acc = y.reshape(N, 400, EMBED), acc.reshape(N, 400, EMBED)
    return rnd(y + pe, w.dt), acc, y


def linear(w: Weights, wname, bname, x, res=None, relu=False, out_dt="same", f32_weights=False):
    """x [..., K] @ W^T + b (+ res) -> (ref, acc)"""
    dt = w.dt if out_dt == "same" else out_dt
    m = (w.f(wname) if f32_weights else w.w(wname)).T
    b = w.f(bname)
    x = x.to(torch.float64)
    y = x @ m + b
    a = x.abs() @ m.abs() + b.abs()
    if res is not None:
        y = y + res
        a = a + res.abs()
    if relu:
        y = y.clamp_min(0.0)
    return rnd(y, dt), C_ACC * a


def sdpa(qkv, dt, per=32, round_out=True, q_per=None):
    """multi-head attention core of qkv [B, T, 1536] (q | k | v, 4 heads of 128) -> (ref, acc) [B, T, 512].
    acc: P is rounded to the element type before the PV product (relative 2u on numerator and denominator) and the scores carry the
    f32 accumulation error C_ACC * scale * sum|q k| (relative on p) -- (2u + 2 C_ACC scale max_j sum|q k_j|) * sum_j p_j |v_j|, plus the
    PV accumulation.  q_per: queries per pass (a softmax row needs every key but no other query: the [q_per, T] score tiles bound the
    memory of a long sequence)."""
    B, T, _ = qkv.shape
    u = 0.0 if dt is None else UNIT[dt]
    scale = 1.0 / math.sqrt(EMBED // HEADS)
    out = torch.empty((B, T, EMBED), dtype=torch.float64, device=qkv.device)
    acc = torch.empty_like(out)
    for sl in _chunks(B, per):
        x = qkv[sl].to(torch.float64).reshape(-1, T, 3, HEADS, EMBED // HEADS).permute(2, 0, 3, 1, 4)   # [3, b, h, T, d]
        k, v = x[1], x[2]
        kt, kat, va = k.transpose(-1, -2), k.abs().transpose(-1, -2), v.abs()
        for qs in _chunks(T, q_per or T):
            q = x[0][:, :, qs]
            s = (q @ kt) * scale
            sa = (q.abs() @ kat) * scale
            p = torch.softmax(s, -1)
            o = p @ v
            pv = p @ va
            rel = 2 * u + 2 * C_ACC * sa.amax(-1, keepdim=True)
            a = rel * pv + C_ACC * pv
            out[sl, qs] = o.permute(0, 2, 1, 3).reshape(-1, o.shape[2], EMBED)
            acc[sl, qs] = a.permute(0, 2, 1, 3).reshape(-1, o.shape[2], EMBED)
    return (rnd(out, dt) if round_out else out), acc


def layernorm(w: Weights, prefix, x, out_dt="same"):
    """LayerNorm(512, eps 1e-5) -> (ref, acc): f32 statistics, C_LN relative on |x_hat * g| + |b|, plus the f32 error of the mean
    (C_ACC * mean |x|) carried through (x - mean) * rstd * g -- it dominates rows whose mean is large against their spread"""
    dt = w.dt if out_dt == "same" else out_dt
    g, b = w.f(prefix + ".weight"), w.f(prefix + ".bias")
    x = x.to(torch.float64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xh = (x - mu) * rstd
    y = xh * g + b
    return rnd(y, dt), C_LN * ((xh * g).abs() + b.abs()) + C_ACC * g.abs() * rstd * x.abs().mean(-1, keepdim=True)


def refiner_head_names(h):
    p = ("trans_head" if h == 0 else "rot_head")
    L = p + ".0."
    return {"in_w": L + "self_attn.in_proj_weight", "in_b": L + "self_attn.in_proj_bias", "out_w": L + "self_attn.out_proj.weight",
            "out_b": L + "self_attn.out_proj.bias", "l1_w": L + "linear1.weight", "l1_b": L + "linear1.bias", "l2_w": L + "linear2.weight",
            "l2_b": L + "linear2.bias", "ln1": L + "norm1", "ln2": L + "norm2", "head_w": p + ".1.weight", "head_b": p + ".1.bias"}


class TensorWeights:
    """the Weights interface over explicit tensors {name: f32 / float64 tensor} instead of a .fpw file (tests/enc_tail_cases.py)"""

    def __init__(self, tensors, dt, device="cpu"):
        self.st, self.dt, self.device = tensors, dt, device

    def w(self, name):
        a = self.st[name]
        if self.dt is not None:
            a = a.to(TORCH_DT[self.dt])
        return a.to(self.device, torch.float64)

    def f(self, name):
        return self.st[name].to(self.device, torch.float64)


def encoder_chain(w, h, x, att, names=None, readout=True):
    """post-norm TransformerEncoderLayer behind the attention, every intermediate rounded where the five-launch form stores it:
    -> dict y1, x1, hid, y2, ln2 (not rounded), pooled [B, 512] (mean over tokens), out [B, O] (head Linear on the mean).
    w: Weights of a .fpw file or TensorWeights; names: the tensor names of the layer (default: refiner head h of the file);
    readout = False: the chain up to LayerNorm 2, without pooled / out"""
    n = names or refiner_head_names(h)
    r = {}
    r["y1"], _ = linear(w, n["out_w"], n["out_b"], att, res=x.to(torch.float64))
    r["x1"], _ = layernorm(w, n["ln1"], r["y1"])
    r["hid"], _ = linear(w, n["l1_w"], n["l1_b"], r["x1"], relu=True)
    r["y2"], _ = linear(w, n["l2_w"], n["l2_b"], r["hid"], res=r["x1"])
    r["ln2"], _ = layernorm(w, n["ln2"], r["y2"], out_dt=None)
    if not readout:
        return r
    r["pooled"] = r["ln2"].mean(-2)
    r["out"], _ = linear(w, n["head_w"], n["head_b"], r["pooled"], out_dt=None, f32_weights=True)
    return r


def trunk_chain(w: Weights, nn_in, N, n_b, pe):
    """the whole trunk from nn_in: -> [stem, act1 .. act14] with the device's borders (None for rounding-free chains is fine)"""
    def pad(t):
        return torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    s, _, _ = stem(w, nn_in)
    acts = [pad(s)]
    cur = acts[0]
    for i, (prefix, stride, res) in enumerate(TRUNK):
        r = interior(acts[res]) if res is not None else None
        if i == 4:     # the a|b concat: the residual of the last encodeA conv is over all NB2 images
            y, _, _ = conv3x3(w, prefix, cur, stride, res=r)
            y = concat_ab(y, N, n_b)
        elif i == len(TRUNK) - 1:
            y, _, _ = tokens(w, cur, r, pe)
            acts.append(y)
            break
        else:
            y, _, _ = conv3x3(w, prefix, cur, stride, res=r)
        cur = pad(y)
        acts.append(cur)
    return acts
