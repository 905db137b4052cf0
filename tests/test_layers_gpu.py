"""Every stage of the product's own forward pass against a float64 reference of that one stage (tests/layer_ref.py).

The test build's activation taps (fpt_tap_arm, fp_nn.h enum TapPoint) copy each tensor out right after its producer, borders included.
Each stage's reference is fed the exact device tensors the stage read ("teacher-forced"), so a wrong tile, a dropped K-step or a biased
rounding fails a NAMED stage instead of nudging a pooled score.  Weights: the discriminating set (conftest disc_nets).

Bound per element (matmul-shaped stages, output stored in the element type; ref = the exact float64 value, NOT rounded):
    |got - ref| <= 0.5 ulp(|ref| + acc) + acc,   acc = C_ACC * (sum |x * w| + |bias| + |residual|),   C_ACC = 1e-6
(layer_ref.py: ~3x the guide's f32 MFMA accumulation figure at K = 4096).  Where the reference pre-activation is below -acc, a ReLU
output must be exactly 0.  The positional table rounds twice (conv output, then + pe), fused or not: its bound adds a second half ulp.
Attention: P rounded to the element type before PV (layer_ref.sdpa).  LayerNorm: f32 statistics, C_LN = 1e-5 relative.
Bias per stage: the mean signed error got - ref in ulps of |ref| + acc is within 0.05 ulp (truncation instead of RNE would be ~0.5).
f32 outputs (pooled rows, heads, features, scores): acc alone.  The fused encoder tail (enc_tail_kernel: pdot) keeps its intermediates
on chip, so it cannot be teacher-forced stage by stage: pdot is compared against the rounded float64 chain from its own inputs, as a
fraction of the spread of the reference over tiles: PDOT_U = 4 unit roundoffs (the kernel and the chain round their intermediates
independently; measured ~1.2 u in f16 and bf16 alike).
"""
import copy
import ctypes as C
import gc
import os
from unittest import mock

import numpy as np
import pytest
import torch

import layer_ref as LR
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, FP_HOST, FP_PREC_BF16, FP_PREC_F16, FP_PREC_FP8, FP_PREC_INT8, FoundationPoseError, _p

pytestmark = pytest.mark.gpu

# fp_nn.h enum TapPoint
TAP_NN_IN, TAP_STEM, TAP_ACT, TAP_HEAD, TAP_HEAD_STRIDE = 0, 1, 1, 16, 8
TAP_PDOT, TAP_TRANS, TAP_ROT, TAP_FEAT = 32, 33, 34, 35
TAP_XF, TAP_XQKV, TAP_XATT, TAP_XOUT, TAP_O32, TAP_SCORES, TAP_PE = 36, 37, 38, 39, 40, 41, 42
H_QKV, H_ATT, H_Y1, H_X1, H_HID, H_Y2, H_POOL, H_LN2 = range(8)
PDOT_U = 4      # pdot: error <= PDOT_U unit roundoffs of the element type, relative to the spread of the reference over tiles
BIAS_ULP = LR.BIAS_ULP
DEV = "cuda"
TABLE = []
FAILS = []   # stage failures of the running test: every stage is checked, then _flush() reports them all by name


def _typed_test_lib():
    return _lib.test_lib()


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_tap_arm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.fpt_tap_bytes.restype = C.c_longlong
    L.fpt_tap_bytes.argtypes = [C.c_int, C.c_int]
    L.fpt_model_poison.argtypes = [C.c_void_p, C.c_int]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    L.fpt_tap_window.argtypes = [C.c_int, C.c_int]
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    L.fpt_plan_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.fpt_plan_heads.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    yield L
    L.fpt_tap_clear()
    if TABLE:
        lines = [f"{'case':<28} {'stage':<14} {'err/bound':>10} {'mean err (ulp)':>15}"] + \
                [f"{c:<28} {s:<14} {r:>10.3f} {b:>15.4f}" for c, s, r, b in TABLE]
        print("\n" + "\n".join(lines))
        out = os.environ.get("FP_LAYER_TABLE")
        if out:
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def model(tl, disc_nets, syn_mesh):
    with mock.patch.object(_lib, "lib", _typed_test_lib):    # the model on the TEST build: its taps and hooks act on this instance
        m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    yield m
    m.close()


@pytest.fixture(autouse=True)
def _free_cached_blocks():
    """the model grows its own buffers with hipMalloc (N up to FP_MAX_BATCH): hand the blocks torch's caching allocator keeps from the
    previous case's taps back to the runtime, before and after every test"""
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def scene(syn_mesh):
    return syn.make_scene(syn_mesh)


@pytest.fixture(scope="module")
def crops(model, syn_mesh, scene):
    model.upload_frame(scene.rgb, scene.depth)
    poses = model.get_hyp_poses(scene.mask)
    assert len(poses) == 252
    a, b = model.render_and_transform(syn_mesh.name, poses, 1.2)
    return a, b


def _win_imgs(N, NB2, win):
    """(hypotheses, images) a windowed tap holds: win = (img0, nimg) -> the window's hypotheses and, for a tensor on NB2 images, their
    observed crops (one per hypothesis, or the one shared crop)"""
    if win is None:
        return N, NB2
    wn = min(N, win[0] + win[1]) - win[0]
    return wn, wn + (wn if NB2 == 2 * N else NB2 - N)


def _shapes(kind, N, NB2, five, win=None, head=True):
    """tap point -> (shape, element tensor?) of everything one call of this network writes.  With an image window the per-image tensors
    (trunk, QKV, attention, the five-launch tail) hold the window's hypotheses only; the pooled rows, heads, scores and the scorer's
    cross-hypothesis tensors stay whole."""
    n, nb2 = _win_imgs(N, NB2, win)
    s = {TAP_NN_IN: ((nb2, 84, 84, 32), 1), TAP_STEM: ((nb2, 82, 82, 64), 1), TAP_PE: ((400, 512), 1)}
    for i in range(1, 15):
        s[TAP_ACT + i] = (((nb2 if i <= 4 else n), 42, 42, 128 if i <= 4 else 256) if i <= 9 else (n, 22, 22, 512) if i <= 13
                          else (n, 400, 512), 1)
    heads = 2 if kind == 0 else 1
    for h in range(heads):
        b = TAP_HEAD + h * TAP_HEAD_STRIDE
        s[b + H_QKV], s[b + H_ATT] = ((n, 400, 1536), 1), ((n, 400, 512), 1)
        if kind == 1:
            s[b + H_POOL] = ((N, 512), 0)
        elif five:
            for k in (H_Y1, H_X1, H_HID, H_Y2):
                s[b + k] = ((n, 400, 512), 1)
            if 1 < N < 96:
                s[b + H_LN2] = ((n, 400, 512), 1)
            s[b + H_POOL] = ((16, 512) if N == 1 else (N, 512), 0)
    if kind == 0:
        if not five:
            s[TAP_PDOT] = ((2, 25 if N == 1 else 5 * N, 4), 0)
        s[TAP_TRANS], s[TAP_ROT] = ((N, 3), 0), ((N, 3), 0)
    else:
        s[TAP_FEAT] = ((N, 512), 0)
        if head:    # (scorer_head: not part of a Register shard)
            s[TAP_O32], s[TAP_SCORES] = ((N, 512), 0), ((N,), 0)
            s[TAP_XF], s[TAP_XQKV], s[TAP_XATT], s[TAP_XOUT] = ((N, 512), 1), ((N, 1536), 1), ((N, 512), 1), ((N, 512), 1)
    return s


class _Taps(dict):
    """the tapped tensors, kept in their element type on the GPU; every read widens to float64, so that a check holds one stage's
    float64 operands at a time (N = 1008: ~17 GB of f16 taps would be ~70 GB of float64)"""
    def __getitem__(self, pt):
        return dict.__getitem__(self, pt).to(torch.float64)

    def raw(self, pt):
        return dict.__getitem__(self, pt)


def _tapped(tl, kind, N, NB2, five, dt, call, win=None, head=True):
    """arm every tap of one call of network `kind` (win = (img0, nimg): that image window of the per-image tensors; head = False: the
    scorer's cross-hypothesis head does not run), run it, return ({point: tensor on the GPU, widened to float64 when read}, pe fused)"""
    tl.fpt_tap_clear()
    if win is not None:
        assert tl.fpt_tap_window(*win) == 0
    edt = LR.TORCH_DT[dt]
    bufs = {}
    for pt, (shape, elem) in _shapes(kind, N, NB2, five, win, head).items():
        t = torch.empty(shape, dtype=edt if elem else torch.float32, device=DEV)
        bufs[pt] = t
        assert tl.fpt_tap_arm(kind, pt, C.c_void_p(t.data_ptr()), t.numel() * t.element_size()) == 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    call()
    torch.cuda.synchronize()
    out = _Taps()
    for pt, t in bufs.items():
        got = tl.fpt_tap_bytes(kind, pt)
        assert got == t.numel() * t.element_size(), (kind, pt, got, t.shape)    # every tap reached, with the size expected
        out[pt] = t
    pe_fused = tl.fpt_tap_pe_fused(kind)
    tl.fpt_tap_clear()
    return out, pe_fused


def _compare(case, stage, got, ref, acc, dt, pre=None, second_rounding=None, record=True):
    """per-element bound + bias; returns (worst err / bound, mean error in ulps)"""
    worst, bias = LR.stage_error(got, ref, acc, dt, pre=pre, second_rounding=second_rounding)
    if record:
        TABLE.append((case, stage, worst, bias))
    return worst, bias


def _assert_stage(case, stage, got, ref, acc, dt, **kw):
    worst, bias = _compare(case, stage, got, ref, acc, dt, **kw)
    if not worst <= 1.0:
        FAILS.append(f"{case}: stage {stage}: err / bound = {worst:.3f}")
    if not abs(bias) <= BIAS_ULP:
        FAILS.append(f"{case}: stage {stage}: mean error {bias:.4f} ulp")


def _flush():
    msgs = list(FAILS)
    FAILS.clear()
    assert not msgs, "\n".join(msgs)


def _assert_f32(case, stage, got, ref, acc):
    err = (got - ref).abs()
    bound = acc + 2.0 ** -24 * ref.abs()
    worst = float((err / bound.clamp_min(1e-30)).max())
    TABLE.append((case, stage, worst, float("nan")))
    if not worst <= 1.0:
        FAILS.append(f"{case}: stage {stage}: err / bound = {worst:.3f}")


def _borders_zero(case, name, t, b=1):
    ring = torch.cat([t[:, :b].flatten(), t[:, -b:].flatten(), t[:, :, :b].flatten(), t[:, :, -b:].flatten()])
    if int((ring != 0).sum()):
        FAILS.append(f"{case}: {name}: non-zero border")


def _live(case, name, t):
    frac = float((t > 0).double().mean())
    if not 0.05 < frac < 0.95:
        FAILS.append(f"{case}: {name}: fraction of ReLU outputs > 0 = {frac:.3f} (degenerate layer)")


def check_trunk(case, w, T, N, n_b, dt, pin_cpu=False):
    """stem, the 13 3x3 convolutions (a|b concat included), the token tensor; borders and non-degeneracy of every padded tensor"""
    _borders_zero(case, "nn_in", T[TAP_NN_IN], 2)
    ref, acc, pre = LR.stem(w, T[TAP_NN_IN])
    _borders_zero(case, "stem", T[TAP_STEM])
    _live(case, "stem", LR.interior(T[TAP_STEM]))
    _assert_stage(case, "stem", LR.interior(T[TAP_STEM]), pre.clamp_min(0.0), acc, dt, pre=pre)
    if pin_cpu:   # the device reference itself: image 0 again in float64 on the CPU
        wc = LR.Weights.__new__(LR.Weights)
        wc.st, wc.dt, wc.device = w.st, w.dt, "cpu"
        _, _, p0 = LR.stem(wc, T[TAP_NN_IN][:1].cpu())
        assert torch.allclose(p0, pre[:1].cpu(), rtol=0, atol=1e-6 * float(acc[:1].max())), f"{case}: stem: GPU float64 reference differs from the CPU one"
    for i, (prefix, stride, res) in enumerate(LR.TRUNK):
        a = i + 1
        r = LR.interior(T[TAP_ACT + res]) if res is not None else None
        if a == 14:
            pe = T[TAP_PE]
            _, acc, c = LR.tokens(w, T[TAP_ACT + 13], r, pe)
            # rnd(rnd(c) + pe) in both forms: add_pos_embed_kernel after the conv, and the fused epilogues, which round the conv value to
            # the element type before adding the table (same bits as the unfused form) -- the first rounding adds half an ulp of c
            _assert_stage(case, "act14 tokens", T[TAP_ACT + 14], c + pe, acc, dt, second_rounding=c)
            break
        got = T[TAP_ACT + a]
        _borders_zero(case, f"act{a}", got)
        xin = T[TAP_ACT + i] if i > 0 else T[TAP_STEM]
        if a == 5:
            full, acc, pre = LR.conv3x3(w, prefix, xin, stride, res=r, out_dt=None)
            ref, acc, pre = (LR.concat_ab(t, N, n_b) for t in (full, acc, pre))
        else:
            ref, acc, pre = LR.conv3x3(w, prefix, xin, stride, res=r, out_dt=None)
        gi = LR.interior(got)
        _live(case, f"act{a}", gi)
        _assert_stage(case, f"act{a} {prefix}", gi, ref, acc, dt, pre=pre)
        if pin_cpu:
            wc = LR.Weights.__new__(LR.Weights)
            wc.st, wc.dt, wc.device = w.st, w.dt, "cpu"
            j = slice(0, 1) if a != 5 else slice(N, N + 1)   # (the concat: pin its b half, the last image of the conv)
            _, _, p0 = LR.conv3x3(wc, prefix, xin[j].cpu(), stride, res=None if r is None else r[j].cpu())
            _, ag, pg = LR.conv3x3(w, prefix, xin[j], stride, res=None if r is None else r[j])
            assert torch.allclose(p0, pg.cpu(), rtol=0, atol=1e-6 * float(ag.max())), f"{case}: act{a}: GPU float64 reference differs from the CPU one"


def _hyps(t, hs, per=1):
    """rows of the window's hypotheses (hs: slice of hypotheses, None = all) of a tensor tapped whole, `per` rows per hypothesis"""
    return t if hs is None else t[hs.start * per:hs.stop * per]


def check_heads(case, w, T, N, dt, five, hs=None):
    """N = the hypotheses the per-image taps hold; hs = where they sit in the whole tensors (pdot, pooled rows, heads)"""
    x = T[TAP_ACT + 14]
    for h in range(2):
        b = TAP_HEAD + h * TAP_HEAD_STRIDE
        n = LR.refiner_head_names(h)
        nm = ("trans", "rot")[h]
        ref, acc = LR.linear(w, n["in_w"], n["in_b"], x, out_dt=None)
        _assert_stage(case, f"{nm} qkv", T[b + H_QKV], ref, acc, dt)
        ref, acc = LR.sdpa(T[b + H_QKV], dt, round_out=False)
        _assert_stage(case, f"{nm} attention", T[b + H_ATT], ref, acc, dt)
        head_w, head_b = w.f(n["head_w"]), w.f(n["head_b"])
        out = _hyps(T[TAP_TRANS if h == 0 else TAP_ROT], hs)
        if not five:
            chain = LR.encoder_chain(w, h, x, T[b + H_ATT])
            rows = 16 if N == 1 else 80
            pref = (chain["ln2"].reshape(-1, rows, 512).sum(1) @ head_w.T)          # [tiles, O]
            pd = _hyps(T[TAP_PDOT][h], hs, 5)[:, :3]
            spread = pref.std(0).clamp_min(1e-12)
            frac = float(((pd - pref).abs() / spread).max())
            lim = PDOT_U * LR.UNIT[dt]
            TABLE.append((case, f"{nm} pdot", frac / lim, float("nan")))
            if not frac <= lim:
                FAILS.append(f"{case}: stage {nm} pdot: error = {frac:.2e} of the spread over tiles")
            tiles = pd.shape[0] // N
            ref = pd.reshape(N, tiles, 3).sum(1) / 400.0 + head_b
            acc = LR.C_ACC * (pd.abs().reshape(N, tiles, 3).sum(1) / 400.0 + head_b.abs())
            _assert_f32(case, f"{nm} heads", out, ref, acc)
            continue
        ref, acc = LR.linear(w, n["out_w"], n["out_b"], T[b + H_ATT], res=x, out_dt=None)
        _assert_stage(case, f"{nm} y1", T[b + H_Y1], ref, acc, dt)
        ref, acc = LR.layernorm(w, n["ln1"], T[b + H_Y1], out_dt=None)
        _assert_stage(case, f"{nm} ln1", T[b + H_X1], ref, acc, dt)
        ref, acc = LR.linear(w, n["l1_w"], n["l1_b"], T[b + H_X1], relu=True, out_dt=None)
        _assert_stage(case, f"{nm} ffn1", T[b + H_HID], ref, acc, dt)
        ref, acc = LR.linear(w, n["l2_w"], n["l2_b"], T[b + H_HID], res=T[b + H_X1], out_dt=None)
        _assert_stage(case, f"{nm} ffn2", T[b + H_Y2], ref, acc, dt)
        ln2, lacc = LR.layernorm(w, n["ln2"], T[b + H_Y2], out_dt=None)
        if 1 < N < 96:
            _assert_stage(case, f"{nm} ln2", T[b + H_LN2], ln2, lacc, dt)
        per = 0.5 * LR.ulp(ln2.abs() + lacc, dt) + lacc + LR.C_ACC * ln2.abs()   # rounded (or not) LN2 output, f32 sums
        if N == 1:    # layernorm_pmean_kernel: 16 partial column sums of 25 rows
            ref, acc = ln2.reshape(16, 25, 512).sum(1), per.reshape(16, 25, 512).sum(1)
            _assert_f32(case, f"{nm} ln2 psums", T[b + H_POOL], ref, acc)
            pooled = T[b + H_POOL].sum(0, keepdim=True) / 400.0
        else:
            pooled = _hyps(T[b + H_POOL], hs)
            _assert_f32(case, f"{nm} ln2 mean", pooled, ln2.mean(1), per.mean(1))
        ref, acc = LR.linear(w, n["head_w"], n["head_b"], pooled, out_dt=None, f32_weights=True)
        _assert_f32(case, f"{nm} heads", out, ref, acc + LR.C_ACC * (pooled.abs() @ head_w.abs().T))


def check_scorer(case, w, T, N, dt, hs=None, head=True):
    """head = False: the per-hypothesis part alone (a Register shard ends at the pooled features)"""
    x = T[TAP_ACT + 14]
    b = TAP_HEAD
    ref, acc = LR.linear(w, "att.in_proj_weight", "att.in_proj_bias", x, out_dt=None)
    _assert_stage(case, "qkv", T[b + H_QKV], ref, acc, dt)
    ref, acc = LR.sdpa(T[b + H_QKV], dt, round_out=False)
    _assert_stage(case, "attention", T[b + H_ATT], ref, acc, dt)
    att = T[b + H_ATT]
    _assert_f32(case, "token mean", _hyps(T[b + H_POOL], hs), att.mean(1), LR.C_ACC * att.abs().mean(1))
    ref, acc = LR.linear(w, "att.out_proj.weight", "att.out_proj.bias", T[b + H_POOL], out_dt=None, f32_weights=True)
    _assert_f32(case, "feat", T[TAP_FEAT], ref, acc)
    if not head:
        return
    _assert_stage(case, "cast", T[TAP_XF], T[TAP_FEAT], torch.zeros_like(T[TAP_XF]), dt)
    ref, acc = LR.linear(w, "att_cross.in_proj_weight", "att_cross.in_proj_bias", T[TAP_XF], out_dt=None)
    _assert_stage(case, "cross qkv", T[TAP_XQKV], ref, acc, dt)
    ref, acc = LR.sdpa(T[TAP_XQKV][None], dt, round_out=False)
    _assert_stage(case, "cross att", T[TAP_XATT], ref[0], acc[0], dt)
    ref, acc = LR.linear(w, "att_cross.out_proj.weight", "att_cross.out_proj.bias", T[TAP_XATT], out_dt=None)
    _assert_stage(case, "cross out", T[TAP_XOUT], ref, acc, dt)
    assert torch.equal(T[TAP_O32], T[TAP_XOUT]), f"{case}: o32 is not the widened cross-attention output"
    ref, acc = LR.linear(w, "linear.weight", "linear.bias", T[TAP_O32], out_dt=None, f32_weights=True)
    _assert_f32(case, "scores", T[TAP_SCORES], ref.reshape(-1), acc.reshape(-1))


def _weights(path, dt):
    return LR.Weights(path, dt, DEV)


def _pe_matches_table(T, dt):
    pe = torch.from_numpy(LR.pos_table()).to(DEV, torch.float64)
    # the device's table is the PositionalEmbedding table (its f32 arguments differ from numpy's in the last bits: t * w_i up to 399 rad)
    assert float((T[TAP_PE] - pe).abs().max()) <= 2.0 ** -8


def _set_prec(model, prec):
    model.set_precision(prec)


N_MAX = 2377             # include/foundationpose_amd.h FP_MAX_BATCH
STEPS_MAX = 56           # FP_MAX_INPLANE_STEPS
REFINER_CASES = [(FP_PREC_F16, 1, 0), (FP_PREC_F16, 7, 0), (FP_PREC_F16, 33, 0), (FP_PREC_F16, 130, 0), (FP_PREC_F16, 252, 0),
                 (FP_PREC_BF16, 1, 0), (FP_PREC_BF16, 42, 0), (FP_PREC_BF16, 252, 0), (FP_PREC_F16, 1, 1), (FP_PREC_F16, 33, 1),
                 (FP_PREC_F16, 130, 1),
                 # inplane steps 3 / 5 / 7 / 24: other left-over sizes; 1008 = BASELINE configs[3]
                 (FP_PREC_F16, 126, 0), (FP_PREC_F16, 210, 0), (FP_PREC_F16, 294, 0), (FP_PREC_F16, 1008, 0), (FP_PREC_BF16, 1008, 0),
                 # fp_track_multi batches: conv_deep_kernel / conv_igemm_kernel on the small layers (3), split-K (4, 8), the 64-wide
                 # igemm of the stem in bf16 (2), left-overs on conv_pp_kernel in bf16 (6)
                 (FP_PREC_F16, 3, 0), (FP_PREC_F16, 4, 0), (FP_PREC_F16, 8, 0), (FP_PREC_BF16, 2, 0), (FP_PREC_BF16, 3, 0),
                 (FP_PREC_BF16, 4, 0), (FP_PREC_BF16, 6, 0), (FP_PREC_BF16, 8, 0),
                 # the plan over every accepted N: conv_256 on conv_deep_kernel over all K-steps from 21 hypotheses (fp_track_multi)
                 (FP_PREC_F16, 21, 0), (FP_PREC_BF16, 21, 0)]
SCORER_CASES = [(FP_PREC_F16, 1), (FP_PREC_F16, 7), (FP_PREC_F16, 42), (FP_PREC_F16, 252), (FP_PREC_BF16, 42), (FP_PREC_F16, 210),
                (FP_PREC_F16, 1008),
                # bf16 conv_big_pp_kernel rounds (84); the cross-attention projections over 714 / 1386 hypotheses (conv_deep_kernel,
                # conv_igemm_kernel<128>)
                (FP_PREC_BF16, 84), (FP_PREC_BF16, 714), (FP_PREC_F16, 1386), (FP_PREC_BF16, 1386),
                # the plan over every accepted N (fp_scorer_infer, fp_net_infer, Register shards): the small-problem kernels in bf16 (1),
                # the 64-wide stem igemm in bf16 (2), conv_deep_kernel / conv_igemm_kernel<128> (3), 2-slice split-K of conv_256 (4),
                # left-overs on conv_pp_kernel and conv_igemm_kernel<128> in bf16 (6), 2-slice split-K of conv_b2 / conv_512 incl. the
                # reduce that adds the positional table (8), conv_256 on conv_deep_kernel over all K-steps (21)
                (FP_PREC_BF16, 1), (FP_PREC_BF16, 2), (FP_PREC_F16, 3), (FP_PREC_BF16, 3), (FP_PREC_F16, 4), (FP_PREC_BF16, 4),
                (FP_PREC_BF16, 6), (FP_PREC_F16, 8), (FP_PREC_BF16, 8), (FP_PREC_F16, 21), (FP_PREC_BF16, 21)]
REGISTER_STEPS = [6, 24]    # the two shared-crop cases below
# Register shards (begin, count, precision) of the 252 hypotheses: the 8-GPU layout of the headline ([0:32], the ragged [224:252]) and
# the smallest shared-crop batch in bf16 (broadcast_b of the b half)
SHARD_CASES = [(0, 32, FP_PREC_F16), (224, 28, FP_PREC_F16), (224, 28, FP_PREC_BF16), (0, 2, FP_PREC_BF16)]


def _inputs(crops, N):
    """N network inputs: the 252 rendered / observed crop pairs, repeated"""
    a, b = crops
    if N <= len(a):
        return a[:N], b[:N]
    i = np.arange(N) % len(a)
    return a[i], b[i]


def _dt_name(dt):
    return "bf16" if dt == LR.BF16 else "f16"


@pytest.mark.parametrize("prec,N,five", REFINER_CASES)
def test_refiner_stages_match_float64(tl, model, crops, disc_nets, prec, N, five):
    dt = LR.BF16 if prec == FP_PREC_BF16 else LR.F16
    case = f"refiner {_dt_name(dt)} N={N}{' 5-launch' if five else ''}"
    a, b = _inputs(crops, N)
    _set_prec(model, prec)
    try:
        tl.fpt_set_enc_tail(0 if five else 1)
        T, pe_fused = _tapped(tl, 0, N, 2 * N, five, dt, lambda: model.refiner_infer(a, b))
    finally:
        tl.fpt_set_enc_tail(1)
        _set_prec(model, FP_PREC_F16)
    if N == 252 and dt == LR.F16:
        assert pe_fused == 1      # the positional table in the epilogue of conv_big_pp_kernel<..., true> + conv_deep_kernel<64, ..., true>
    _pe_matches_table(T, dt)
    w = _weights(disc_nets[0], dt)
    check_trunk(case, w, T, N, N, dt, pin_cpu=(N == 252 and dt == LR.F16 and not five))
    check_heads(case, w, T, N, dt, five)
    _flush()


@pytest.mark.parametrize("prec,N", SCORER_CASES)
def test_scorer_stages_match_float64(tl, model, crops, disc_nets, prec, N):
    dt = LR.BF16 if prec == FP_PREC_BF16 else LR.F16
    case = f"scorer {_dt_name(dt)} N={N}"
    a, b = _inputs(crops, N)
    _set_prec(model, prec)
    try:
        T, _ = _tapped(tl, 1, N, 2 * N, False, dt, lambda: model.scorer_infer(a, b))
    finally:
        _set_prec(model, FP_PREC_F16)
    w = _weights(disc_nets[1], dt)
    check_trunk(case, w, T, N, N, dt)
    check_scorer(case, w, T, N, dt)
    _flush()


def _register_stages(tl, model, disc_nets, syn_mesh, scene, steps, wins):
    """Register's refiner pass: 42 * steps hypotheses that share ONE observed crop (NB2 = N + 1, the b half of the concat broadcast);
    wins: image windows to check (None = the whole tensors)"""
    N = 42 * steps
    w = _weights(disc_nets[0], LR.F16)
    model.set_inplane_steps(steps)
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        for win in wins:
            T, _ = _tapped(tl, 0, N, N + 1, False, LR.F16, lambda: model.Register(scene.rgb, scene.depth, scene.mask, syn_mesh.name), win)
            n, hs = (N, None) if win is None else (win[1], slice(win[0], win[0] + win[1]))
            case = f"Register refiner N={N} shared-b" + ("" if win is None else f" [{hs.start}:{hs.stop}]")
            check_trunk(case, w, T, n, 1, LR.F16)
            check_heads(case, w, T, n, LR.F16, False, hs)
            cat = LR.interior(T.raw(TAP_ACT + 5))[..., 128:]
            assert torch.equal(cat, cat[:1].expand_as(cat)), case     # every hypothesis holds the same b half
            del T, cat
    finally:
        tl.fpt_model_use_graphs(model._h, 1)
        model.set_inplane_steps(6)
    _flush()


def test_register_shared_crop_stages_match_float64(tl, model, disc_nets, syn_mesh, scene):
    _register_stages(tl, model, disc_nets, syn_mesh, scene, 6, [None])


def test_register_shared_crop_stages_match_float64_at_1008(tl, model, disc_nets, syn_mesh, scene):
    """inplane steps 24 (BASELINE configs[3]): NB2 = 1009 images in encodeA"""
    _register_stages(tl, model, disc_nets, syn_mesh, scene, 24, [None])


def _bitwise(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_windowed_taps_equal_the_slice_of_the_full_taps(tl, model, crops, syn_mesh, scene):
    """fpt_tap_window: a window's tensors are the matching rows of the full taps, bit for bit -- hypotheses with their own observed
    crops (refiner, scorer), the shared crop (Register), and a window clamped at the last hypothesis"""
    a, b = crops
    N = 252
    runs = [(0, 2 * N, lambda: model.refiner_infer(a, b)), (1, 2 * N, lambda: model.scorer_infer(a, b)),
            (0, N + 1, lambda: model.Register(scene.rgb, scene.depth, scene.mask, syn_mesh.name))]
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        for kind, NB2, call in runs:
            full, _ = _tapped(tl, kind, N, NB2, False, LR.F16, call)
            for w0, wn in ((100, 20), (N - 5, 16)):
                win, _ = _tapped(tl, kind, N, NB2, False, LR.F16, call, (w0, wn))
                w1 = min(N, w0 + wn)
                for pt in _shapes(kind, N, NB2, False):
                    f, g = full.raw(pt), win.raw(pt)
                    if g.shape == f.shape:
                        exp = f
                    elif f.shape[0] == NB2 and NB2 == 2 * N:
                        exp = torch.cat([f[w0:w1], f[N + w0:N + w1]])
                    elif f.shape[0] == NB2:
                        exp = torch.cat([f[w0:w1], f[N:N + 1]])
                    else:
                        exp = f[w0:w1]
                    assert torch.equal(_bitwise(g), _bitwise(exp)), (kind, NB2, pt, w0, wn)
    finally:
        tl.fpt_model_use_graphs(model._h, 1)


# ---- which schedules the float64 cases reach -----------------------------------------------------------------------------------

ROWS_PER_IMG = {"conv_stem": 6400, "conv_a1": 1600, "conv_128": 1600, "conv_256": 1600, "conv_b2": 400, "conv_512": 400}


def _log_records(tl):
    n = tl.fpt_launch_log_count()
    f = (C.c_int * (7 * max(n, 1)))()
    names = C.create_string_buffer(96 * max(n, 1))
    assert tl.fpt_launch_log_get_all(f, names, 96, n) == n
    raw = names.raw
    out = []
    for i in range(n):
        net, prec, side, m_begin, M, ksplit, pe = f[7 * i:7 * i + 7]
        tag, _, kern = raw[96 * i:96 * (i + 1)].split(b"\0", 1)[0].decode().rpartition("/")
        out.append(dict(net=("refiner", "scorer")[net], prec=("f16", "bf16", "fp8", "int8")[prec], side=side, m_begin=m_begin, M=M,
                        ksplit=ksplit, pe=pe, tag=tag, kernel=kern))
    return out


def _logged(tl, fn):
    """the launch log of fn(): [record]"""
    tl.fpt_launch_log_arm(1)
    try:
        fn()
    finally:
        tl.fpt_launch_log_arm(0)
    recs = _log_records(tl)
    tl.fpt_launch_log_clear()
    assert recs, "no launch was logged"
    return recs


def _key(r):
    """(net, precision, layer tag, kernel, stream, pe fused, split-K slices)"""
    return (r["net"], r["prec"], r["tag"], r["kernel"], "side" if r["side"] else "main", r["pe"], r["ksplit"])


PLAN_REFINER, PLAN_SCORER, PLAN_SCORER_FEATURES = 0, 1, 2    # fpt_plan_forward kinds


def _plan(tl, model, kind, N, shared=0):
    """the launch log of a plan-only call (fpt_plan_forward) at the model's precision: what the real call would launch"""
    def run():
        assert tl.fpt_plan_forward(model._h, kind, N, shared) == 0, tl.fp_last_error().decode()
    return _logged(tl, run)


def _boundary_windows(recs, N, NB2):
    """image windows (3 hypotheses) around every hypothesis holding the first row of a launch that starts inside a layer"""
    imgs = set()
    for r in recs:
        per = ROWS_PER_IMG.get(r["tag"])
        if per and r["m_begin"] > 0:
            i = r["m_begin"] // per
            imgs.add(min(i, N - 1) if i < N else (i - N if NB2 == 2 * N else N - 1))
    wins, last = [], -1
    for i in sorted(imgs):
        w0 = min(max(0, i - 1), N - 3)
        if w0 > last:
            wins.append((w0, 3))
            last = w0 + 2
    return wins


def test_refiner_stages_match_float64_at_the_batch_limit(tl, model, crops, disc_nets):
    """refiner_infer with FP_MAX_BATCH hypotheses (2 N_MAX images in encodeA): the first 2 and the last 16 hypotheses, which carry the
    largest offsets the kernels form, and a window around every launch boundary, stage by stage in float64"""
    a, b = _inputs(crops, N_MAX)
    recs = _logged(tl, lambda: model.refiner_infer(a, b))
    w = _weights(disc_nets[0], LR.F16)
    for win in [(0, 2), (N_MAX - 16, 16)] + _boundary_windows(recs, N_MAX, 2 * N_MAX):
        T, _ = _tapped(tl, 0, N_MAX, 2 * N_MAX, False, LR.F16, lambda: model.refiner_infer(a, b), win)
        case = f"refiner f16 N={N_MAX} [{win[0]}:{win[0] + win[1]}]"
        check_trunk(case, w, T, win[1], win[1], LR.F16)
        check_heads(case, w, T, win[1], LR.F16, False, slice(win[0], win[0] + win[1]))
        del T
    _flush()


def test_register_stages_match_float64_at_the_largest_inplane_steps(tl, model, disc_nets, syn_mesh, scene):
    N = 42 * STEPS_MAX
    model.set_inplane_steps(STEPS_MAX)
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        recs = _logged(tl, lambda: model.Register(scene.rgb, scene.depth, scene.mask, syn_mesh.name))
    finally:
        tl.fpt_model_use_graphs(model._h, 1)
        model.set_inplane_steps(6)
    wins = [(0, 2), (N - 16, 16)] + _boundary_windows([r for r in recs if r["net"] == "refiner"], N, N + 1)
    _register_stages(tl, model, disc_nets, syn_mesh, scene, STEPS_MAX, wins)


def test_batches_past_the_limit_are_refused(tl, model, disc_nets):
    """one hypothesis past FP_MAX_BATCH: an error that names the limit, and no network launch"""
    def refused(fn):
        with pytest.raises(FoundationPoseError):
            fn()
        msg = tl.fp_last_error().decode()      # (the model runs on the test build: its error is that library's)
        assert "FP_MAX_BATCH" in msg, msg

    tl.fpt_launch_log_arm(1)
    try:
        refused(lambda: model.set_inplane_steps(STEPS_MAX + 1))
        assert model.num_hypotheses == 252
        x = np.zeros((N_MAX + 1, 160, 160, 6), np.float32)
        refused(lambda: model.refiner_infer(x, x))
        refused(lambda: model.scorer_infer(x, x))
        assert tl.fpt_launch_log_count() == 0
    finally:
        tl.fpt_launch_log_arm(0)
    for path, scorer in ((disc_nets[0], 0), (disc_nets[1], 1)):
        assert not tl.fp_net_create(path.encode(), scorer, N_MAX + 1)
        assert "FP_MAX_BATCH" in tl.fp_last_error().decode()
    model.set_inplane_steps(STEPS_MAX)      # the largest accepted value
    model.set_inplane_steps(6)


def test_every_launched_schedule_is_checked_in_float64(tl, model, crops, syn_mesh, scene):
    """every (network, precision, layer, kernel, stream, pe fused, split-K slice count) an accepted batch size launches is launched by
    at least one float64 stage case of this file.  Accepted: the plan (fpt_plan_forward, test_plan_equals_reality) of the refiner with
    its own crops and of the scorer at every N in 1..FP_MAX_BATCH, and of the refiner with Register's shared crop at every N in
    2..42 * FP_MAX_INPLANE_STEPS (a shard of one hypothesis takes its own crop), in f16 and bf16 -- this holds fp_track_multi (1..64
    objects), every Register shard, fp_refiner_infer / fp_scorer_infer and fp_net_infer; and, as real calls, Track, 2..8 objects, 42 * s
    for every accepted inplane step s, and Register at 42 * s in f16.  Distinct keys: 127 over the real calls alone (split-K as a
    boolean; also 127 with the slice count), 180 over the whole accepted space -- the 53 more are the scorer below 42 hypotheses
    (1..8, 21), conv_256 on conv_deep_kernel from 21 hypotheses and broadcast_b in bf16."""
    big = _inputs(crops, 42 * STEPS_MAX)
    covered = set()
    for prec, N, five in REFINER_CASES:
        _set_prec(model, prec)
        tl.fpt_set_enc_tail(0 if five else 1)
        try:
            covered |= {_key(r) for r in _logged(tl, lambda: model.refiner_infer(big[0][:N], big[1][:N]))}
        finally:
            tl.fpt_set_enc_tail(1)
            _set_prec(model, FP_PREC_F16)
    for prec, N in SCORER_CASES:
        _set_prec(model, prec)
        try:
            covered |= {_key(r) for r in _logged(tl, lambda: model.scorer_infer(big[0][:N], big[1][:N]))}
        finally:
            _set_prec(model, FP_PREC_F16)
    a, b = _inputs(crops, N_MAX)
    covered |= {_key(r) for r in _logged(tl, lambda: model.refiner_infer(a, b))}
    del a, b

    def register(steps):
        model.set_inplane_steps(steps)
        tl.fpt_model_use_graphs(model._h, 0)
        try:
            return _logged(tl, lambda: model.Register(scene.rgb, scene.depth, scene.mask, syn_mesh.name))
        finally:
            tl.fpt_model_use_graphs(model._h, 1)
            model.set_inplane_steps(6)
    for steps in REGISTER_STEPS + [STEPS_MAX]:
        covered |= {_key(r) for r in register(steps) if r["net"] == "refiner"}   # (its scorer pass is a scorer case's)
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        for begin, count, prec in SHARD_CASES:      # (both passes of a shard are checked)
            _set_prec(model, prec)
            covered |= {_key(r) for r in _logged(tl, lambda: _shard_begin(model, scene, syn_mesh, begin, count))}
    finally:
        _set_prec(model, FP_PREC_F16)
        tl.fpt_model_use_graphs(model._h, 1)

    first = {}    # key -> smallest served N (and how) that launches it
    def served(keys, how, N):
        for k in keys:
            if k not in first or N < first[k][0]:
                first[k] = (N, how)
    sizes = [1] + list(range(2, 9)) + [42 * s for s in range(1, STEPS_MAX + 1)]
    for prec in (FP_PREC_F16, FP_PREC_BF16):
        _set_prec(model, prec)
        try:
            for N in sizes:
                served({_key(r) for r in _logged(tl, lambda: model.refiner_infer(big[0][:N], big[1][:N]))}, "refiner_infer", N)
                if N % 42 == 0:
                    served({_key(r) for r in _logged(tl, lambda: model.scorer_infer(big[0][:N], big[1][:N]))}, "scorer_infer", N)
        finally:
            _set_prec(model, FP_PREC_F16)
    for s in range(1, STEPS_MAX + 1):
        served({_key(r) for r in register(s)}, "Register", 42 * s)
    n_real, n_bool = len(first), len({k[:-1] + (k[-1] > 1,) for k in first})
    for prec in (FP_PREC_F16, FP_PREC_BF16):      # the plan over everything accepted (largest N first: the buffers grow once)
        _set_prec(model, prec)
        try:
            for N in range(N_MAX, 0, -1):
                served({_key(r) for r in _plan(tl, model, PLAN_REFINER, N)}, "plan refiner", N)
                served({_key(r) for r in _plan(tl, model, PLAN_SCORER, N)}, "plan scorer", N)
                if 1 < N <= 42 * STEPS_MAX:
                    served({_key(r) for r in _plan(tl, model, PLAN_REFINER, N, 1)}, "plan refiner shared-b", N)
        finally:
            _set_prec(model, FP_PREC_F16)
    print(f"\ndistinct launch keys: {n_bool} over the real calls with split-K as a boolean, {n_real} with the slice count, "
          f"{len(first)} over the accepted space")
    print("\n" + "\n".join(f"{'covered' if k in covered else 'MISSING'}  first at N={n:<5} ({how}): {k}"
                           for k, (n, how) in sorted(first.items(), key=lambda kv: (kv[1][0], kv[0]))))
    missing = sorted((n, how, k) for k, (n, how) in first.items() if k not in covered)
    assert not missing, "schedules without a float64 stage case:\n" + "\n".join(f"  {k}: first at N = {n} ({how})" for n, how, k in missing)


PLAN_SIZES = [1, 2, 5, 9, 14, 15, 28, 29, 32, 33, 64, 127, 252, 253, 1009, 2377]
FIELDS = ("net", "prec", "tag", "kernel", "m_begin", "M", "ksplit", "pe", "side")


def _same_launches(what, real, plan):
    real, plan = [tuple(r[f] for f in FIELDS) for r in real], [tuple(r[f] for f in FIELDS) for r in plan]
    assert real == plan, f"{what}: the plan differs from the real call\n" + "\n".join(
        f"  {i}: real {a}  plan {b}" for i, (a, b) in enumerate(zip(real + [None] * len(plan), plan + [None] * len(real))) if a != b)


def _shard_begin(model, scene, mesh, begin, count):
    """fp_register_shard_begin over hypotheses [begin, begin + count) of the model's grid (refine_itr 1)"""
    rgb, depth, mask = model._frame(scene.rgb, scene.depth, scene.mask)
    feat, poses = C.c_void_p(), C.c_void_p()
    model._must(model._L.fp_register_shard_begin(model._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1],
                                                 mesh.name.encode(), 1, begin, count, C.byref(feat), C.byref(poses)))
    model.synchronize()


def _shard_plan(tl, model, count):
    """what a shard of `count` hypotheses launches: the refiner on the shared crop (own crop for one hypothesis), the scorer trunk"""
    return _plan(tl, model, PLAN_REFINER, count, 1 if count > 1 else 0) + _plan(tl, model, PLAN_SCORER_FEATURES, count)


def test_plan_equals_reality(tl, model, crops, disc_nets, syn_mesh, scene):
    """fpt_plan_forward records, field for field, what the real call launches: refiner (own crops, Register's shared crop) and scorer
    at every PLAN_SIZES N in f16 and bf16, and the served entry points fp_track_multi, fp_register_shard_begin and fp_net_infer"""
    da, db = (torch.from_numpy(x).to(DEV) for x in crops)
    t, r, sc = (np.zeros((N_MAX, 3), np.float32), np.zeros((N_MAX, 3), np.float32), np.zeros(N_MAX, np.float32))
    L = model._L
    model.set_inplane_steps(STEPS_MAX)
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        for prec in (FP_PREC_F16, FP_PREC_BF16):
            _set_prec(model, prec)
            for N in PLAN_SIZES:
                i = torch.arange(N, device=DEV) % len(da)
                a, b = da[i].contiguous(), db[i].contiguous()
                torch.cuda.synchronize()
                pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
                real = _logged(tl, lambda: model._must(L.fp_refiner_infer(model._h, pa, pb, FP_DEVICE, N, _p(t), _p(r))))
                _same_launches(f"refiner prec={prec} N={N}", real, _plan(tl, model, PLAN_REFINER, N))
                real = _logged(tl, lambda: model._must(L.fp_scorer_infer(model._h, pa, pb, FP_DEVICE, N, _p(sc))))
                _same_launches(f"scorer prec={prec} N={N}", real, _plan(tl, model, PLAN_SCORER, N))
                del a, b
                if N <= 42 * STEPS_MAX:
                    real = _logged(tl, lambda: _shard_begin(model, scene, syn_mesh, 0, N))
                    _same_launches(f"shard [0:{N}] prec={prec}", real, _shard_plan(tl, model, N))
            _set_prec(model, FP_PREC_F16)
        model.set_inplane_steps(6)
        for begin, count in ((0, 32), (224, 28), (0, 1)):       # the 8-GPU shards of N = 252, a shard of one hypothesis
            real = _logged(tl, lambda: _shard_begin(model, scene, syn_mesh, begin, count))
            _same_launches(f"fp_register_shard_begin({begin}, {count})", real, _shard_plan(tl, model, count))
    finally:
        _set_prec(model, FP_PREC_F16)
        tl.fpt_model_use_graphs(model._h, 1)
        model.set_inplane_steps(6)
    del da, db
    # fp_track_multi: K objects of two meshes in alternating groups = one refiner batch of K with their own crops
    ma, mb = syn.make_mesh(name="a"), syn.make_mesh(textured=False, name="b", subdiv=3)
    with mock.patch.object(_lib, "lib", _typed_test_lib):
        m2 = FoundationPose([ma, mb], syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        tl.fpt_model_use_graphs(m2._h, 0)
        base = syn.perturb_pose(scene.gt_pose)
        for K in (9, 33, 64):
            hyps = np.stack([base] * K)
            hyps[:, 0, 3] += 0.001 * np.arange(K, dtype=np.float32)
            names = [("a", "b")[(k // 3) % 2] for k in range(K)]
            ok = []
            real = _logged(tl, lambda: ok.append(m2.track_multi(scene.rgb, scene.depth, hyps, names)[0]))
            assert ok == [True], m2.last_error
            _same_launches(f"fp_track_multi K={K}", real, _plan(tl, model, PLAN_REFINER, K))
    finally:
        m2.close()
    # fp_net_infer (the InferCore shim, f16) on its device blobs
    for path, scorer in ((disc_nets[0], 0), (disc_nets[1], 1)):
        n = tl.fp_net_create(path.encode(), scorer, 64)
        assert n, tl.fp_last_error().decode()
        try:
            for blob in (b"render_input", b"transf_input"):
                assert tl.fp_net_blob(n, blob, FP_DEVICE)
            for batch in (7, 40):
                real = _logged(tl, lambda: tl.fp_net_infer(n, batch, FP_DEVICE, FP_DEVICE, FP_DEVICE) == 0 or pytest.fail(tl.fp_last_error().decode()))
                _same_launches(f"fp_net_infer scorer={scorer} batch={batch}", real, _plan(tl, model, PLAN_SCORER if scorer else PLAN_REFINER, batch))
        finally:
            tl.fp_net_destroy(n)


@pytest.fixture(scope="module")
def q8_blobs(tl, disc_nets, syn_mesh, scene):
    """one-frame calibration records of FP8 and INT8 (every stage 8-bit), made once on a model of their own: the launches of a trunk
    do not depend on the numbers in its record, so every stage mask below loads these"""
    tl.fpt_set_q8_blocks(15)
    with mock.patch.object(_lib, "lib", _typed_test_lib):
        m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        blobs = {}
        for prec in (FP_PREC_FP8, FP_PREC_INT8):
            m.calibrate(scene.rgb, scene.depth, scene.mask, syn_mesh.name, prec)
            blobs[prec] = m.get_calibration_blob(prec)
    finally:
        m.close()
    return blobs


@pytest.mark.parametrize("mask", (15, 4, 6, 9))
def test_plan_equals_reality_of_the_8bit_trunks(tl, crops, disc_nets, syn_mesh, scene, q8_blobs, mask):
    """test_plan_equals_reality for FP8 and INT8 under the stage masks that between them reach every boundary form of plan_trunk -- a
    dual epilogue (15), q8_copy behind a 2-byte producer in its three places (4: encodeAB.1, 6: the concat, 9: encodeAB.2), 8-bit ->
    f16 only (4, 9) and 8-bit alone (6, 15): refiner and scorer with own crops at N = 1, 15, 16, 33 and the refiner on Register's shared
    crop at N = 15, 16 -- both sides of the per-image-bias threshold, with and without the broadcast"""
    da, db = (torch.from_numpy(x).to(DEV) for x in crops)
    t, r, sc = (np.zeros((33, 3), np.float32), np.zeros((33, 3), np.float32), np.zeros(33, np.float32))
    tl.fpt_set_q8_blocks(mask)          # (networks loaded from now on: the model below)
    try:
        with mock.patch.object(_lib, "lib", _typed_test_lib):
            m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
        try:
            L = m._L
            tl.fpt_model_use_graphs(m._h, 0)
            for blob in q8_blobs.values():
                m.set_calibration_blob(blob)
            for prec in (FP_PREC_FP8, FP_PREC_INT8):
                m.set_precision(prec)
                for N in (1, 15, 16, 33):
                    a, b = da[:N].contiguous(), db[:N].contiguous()
                    torch.cuda.synchronize()
                    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
                    real = _logged(tl, lambda: m._must(L.fp_refiner_infer(m._h, pa, pb, FP_DEVICE, N, _p(t), _p(r))))
                    _same_launches(f"refiner mask={mask} prec={prec} N={N}", real, _plan(tl, m, PLAN_REFINER, N))
                    real = _logged(tl, lambda: m._must(L.fp_scorer_infer(m._h, pa, pb, FP_DEVICE, N, _p(sc))))
                    _same_launches(f"scorer mask={mask} prec={prec} N={N}", real, _plan(tl, m, PLAN_SCORER, N))
                    del a, b
                for N in (15, 16):
                    real = _logged(tl, lambda: _shard_begin(m, scene, syn_mesh, 0, N))
                    _same_launches(f"shard [0:{N}] mask={mask} prec={prec}", real, _shard_plan(tl, m, N))
        finally:
            m.close()
    finally:
        tl.fpt_set_q8_blocks(15)


# fp_nn.hip: QkvForm, TailForm, PoolForm of fpt_plan_heads (fields18[0], [14], [15])
QKV_LINEAR, QKV_TILE, QKV_GROUPED = 0, 1, 2
TAIL_NONE, TAIL_ONE_1, TAIL_ONE_5, TAIL_GROUPED_CHAIN, TAIL_HEAD_CHAIN = range(5)
POOL_TAIL_PDOT, POOL_LN_PMEAN, POOL_LN_MEAN, POOL_LN_TOKEN_MEAN, POOL_TOKEN_MEAN = range(5)


def _heads_plan(tl, kind, N, offer=0):
    f, t = (C.c_int * 18)(), (C.c_int * 3)()
    assert tl.fpt_plan_heads(kind, N, LR.F16, offer, f, t) == 0
    return dict(qkv=f[0], tail=f[14], pool=f[15])


def _head_launches(recs):
    """the launches behind the trunk as the log names them: a Linear layer is its tag (one entry however many steps its plan_conv schedule
    takes), the QKV projection says whether qkv_tile_kernel ran it"""
    last = max(i for i, r in enumerate(recs) if r["tag"] == "conv_512" or r["kernel"] == "add_pos_embed")
    out = []
    for r in recs[last + 1:]:
        if r["kernel"] == "conv_splitk_reduce_kernel" or r["m_begin"] > 0:
            continue
        if r["tag"] == "gemm_qkv":
            out.append("qkv:tile" if r["kernel"] == "qkv_tile_kernel" else "qkv:linear")
        else:
            out.append(r["tag"] or r["kernel"])
    return out


def _launches_of_plan(kind, p):
    """what the forms of a HeadsPlan launch, in order"""
    qkv = "qkv:tile" if p["qkv"] == QKV_TILE else "qkv:linear"
    pool = {POOL_LN_PMEAN: ["layernorm_pmean"], POOL_LN_MEAN: ["layernorm_mean"], POOL_LN_TOKEN_MEAN: ["layernorm", "token_mean"],
            POOL_TOKEN_MEAN: ["token_mean"], POOL_TAIL_PDOT: []}[p["pool"]]
    chain = ["gemm_512", "layernorm", "gemm_512", "gemm_512"]
    if kind == PLAN_SCORER_FEATURES:
        return [qkv, "attention"] + pool + ["small_linear"]
    if p["tail"] in (TAIL_ONE_1, TAIL_ONE_5):
        return [qkv, "attention"] * (1 if p["qkv"] == QKV_GROUPED else 2) + ["enc_tail", "small_linear"]
    if p["tail"] == TAIL_GROUPED_CHAIN:
        return [qkv, "attention"] + chain + pool + ["small_linear"]
    assert p["tail"] == TAIL_HEAD_CHAIN
    return ([qkv, "attention"] + chain + pool + ["small_linear"]) * 2


SCORER_HEAD_LAUNCHES = ["cast", "gemm_cross", "attention", "gemm_cross", "score_linear", "small_linear"]


def test_the_pure_heads_plan_is_what_launches(tl, model):
    """fpt_plan_heads (host arithmetic alone, tests/test_heads_plan_cpu.py holds it to its table) against the launch log of a plan-only
    forward pass (fpt_plan_forward, which test_plan_equals_reality ties to the real calls): the records behind the trunk are the forms the
    pure plan names, at every N where a form changes -- and under enc_tail = 0 at the boundary of layernorm_mean"""
    _set_prec(model, FP_PREC_F16)
    for N in (1, 2, 4, 5, 95, 96, 252):
        p = _heads_plan(tl, 0, N)
        assert p["tail"] == (TAIL_ONE_1 if N == 1 else TAIL_ONE_5) and p["qkv"] == (QKV_GROUPED if N == 1 else QKV_TILE)
        assert _head_launches(_plan(tl, model, PLAN_REFINER, N)) == _launches_of_plan(PLAN_REFINER, p), N
    tl.fpt_set_enc_tail(0)
    try:
        for N in (1, 95, 96):
            p = _heads_plan(tl, 0, N)
            assert p["tail"] == (TAIL_GROUPED_CHAIN if N == 1 else TAIL_HEAD_CHAIN)
            assert p["pool"] == (POOL_LN_PMEAN if N == 1 else POOL_LN_MEAN if N >= 96 else POOL_LN_TOKEN_MEAN)
            assert _head_launches(_plan(tl, model, PLAN_REFINER, N)) == _launches_of_plan(PLAN_REFINER, p), N
    finally:
        tl.fpt_set_enc_tail(1)
    for N in (4, 5, 32, 33, 2048, 2049):
        p = _heads_plan(tl, 1, N)
        assert _heads_plan(tl, 2, N) == dict(qkv=QKV_LINEAR, tail=TAIL_NONE, pool=POOL_TOKEN_MEAN)
        assert _head_launches(_plan(tl, model, PLAN_SCORER, N)) == _launches_of_plan(PLAN_SCORER_FEATURES, p) + SCORER_HEAD_LAUNCHES, N


def _register_shard_stages(tl, model, disc_nets, syn_mesh, scene, begin, count, prec):
    """one Register shard (fp_register_shard_begin over [begin, begin + count) of the 252 hypotheses): its refiner pass on the shared crop
    (NB2 = count + 1) and its scorer trunk, stage by stage in float64 -- and the shard's nn_in is, bit for bit, rows [begin, begin + count)
    of the unsharded Register's nn_in plus the shared crop"""
    dt = LR.BF16 if prec == FP_PREC_BF16 else LR.F16
    c = count
    case = f"shard {_dt_name(dt)} [{begin}:{begin + c}]"
    model.set_inplane_steps(6)
    _set_prec(model, prec)
    tl.fpt_model_use_graphs(model._h, 0)
    try:
        N = model.num_hypotheses
        full = torch.empty((N + 1, 84, 84, 32), dtype=LR.TORCH_DT[dt], device=DEV)
        tl.fpt_tap_clear()
        assert tl.fpt_tap_arm(0, TAP_NN_IN, C.c_void_p(full.data_ptr()), full.numel() * full.element_size()) == 0
        torch.cuda.synchronize()
        _shard_begin(model, scene, syn_mesh, 0, N)
        torch.cuda.synchronize()
        assert tl.fpt_tap_bytes(0, TAP_NN_IN) == full.numel() * full.element_size()
        tl.fpt_tap_clear()
        T, _ = _tapped(tl, 0, c, c + 1, False, dt, lambda: _shard_begin(model, scene, syn_mesh, begin, c))
        exp = torch.cat([full[begin:begin + c], full[N:N + 1]])
        assert torch.equal(_bitwise(T.raw(TAP_NN_IN)), _bitwise(exp)), f"{case}: nn_in is not the unsharded Register's"
        del full, exp
        w = _weights(disc_nets[0], dt)
        check_trunk(case + " refiner", w, T, c, 1, dt)
        check_heads(case + " refiner", w, T, c, dt, False)
        del T
        T, _ = _tapped(tl, 1, c, 2 * c, False, dt, lambda: _shard_begin(model, scene, syn_mesh, begin, c), head=False)
        w = _weights(disc_nets[1], dt)
        check_trunk(case + " scorer", w, T, c, c, dt)
        check_scorer(case + " scorer", w, T, c, dt, head=False)
        del T
    finally:
        tl.fpt_model_use_graphs(model._h, 1)
        _set_prec(model, FP_PREC_F16)
    _flush()


@pytest.mark.parametrize("begin,count,prec", SHARD_CASES)
def test_register_shard_stages_match_float64(tl, model, disc_nets, syn_mesh, scene, begin, count, prec):
    """the 8-GPU layout of the N = 252 headline: the first shard [0:32] and the ragged last one [224:252]; a shard of two in bf16"""
    _register_shard_stages(tl, model, disc_nets, syn_mesh, scene, begin, count, prec)


# trunk layer tag -> the names check_trunk gives its stages
SPLIT_STAGES = {"conv_stem": ["stem"], "conv_a1": ["act1"], "conv_128": [f"act{i}" for i in range(2, 6)],
                "conv_256": [f"act{i}" for i in range(6, 10)], "conv_b2": ["act10"], "conv_512": [f"act{i}" for i in range(11, 15)]}


def _fails(fn):
    FAILS.clear()
    fn()
    msgs = list(FAILS)
    FAILS.clear()
    return msgs


def test_ablations_fail_the_named_stage(tl, model, crops, disc_nets):
    """the checks bite: two wrong-result switches of the test build each fail their stage by name.  Also recorded: whether the
    network-level tolerances of test_nn_gpu.py (rtol 2e-2, atol 2e-3 against the torch oracle) would have noticed."""
    a, b = crops
    w = _weights(disc_nets[0], LR.F16)
    with torch.no_grad():
        net = copy.deepcopy(disc_nets[2]).to(DEV)
        ref_t, ref_r = net(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    ref_t, ref_r = ref_t.cpu().numpy(), ref_r.cpu().numpy()
    notes = []
    # split-K: the trunk layers the plan of N = 8 splits (and with how many slices); dropping the last slice must fail exactly those
    split = {(r["tag"], r["ksplit"]) for r in _plan(tl, model, PLAN_REFINER, 8) if r["ksplit"] > 1 and r["tag"] in SPLIT_STAGES}
    assert split, "no split-K trunk layer at N = 8"
    split_stages = [st for tag, _ in split for st in SPLIT_STAGES[tag]]
    for switch, val, N in (("fpt_set_qkv_ablate", 1, 252), ("fpt_set_conv_ablate", 16, 252), ("fpt_set_splitk_ablate", 1, 8)):
        outs = {}
        try:
            getattr(tl, switch)(val)
            T, _ = _tapped(tl, 0, N, 2 * N, False, LR.F16, lambda: outs.update(zip("tr", model.refiner_infer(a[:N], b[:N]))))
        finally:
            getattr(tl, switch)(0)
        case = f"{switch}({val})"
        if switch == "fpt_set_qkv_ablate":
            msgs = _fails(lambda: check_heads(case, w, T, N, LR.F16, False))
            hit = [m for m in msgs if "qkv" in m]
        elif switch == "fpt_set_splitk_ablate":
            msgs = _fails(lambda: check_trunk(case, w, T, N, N, LR.F16))
            named = [m for m in msgs if any(f"stage {st} " in m or f"stage {st}:" in m for st in split_stages)]
            hit = named
            assert named == msgs, (split, msgs)                                        # only the split layers fail ...
            T0, _ = _tapped(tl, 0, N, 2 * N, False, LR.F16, lambda: model.refiner_infer(a[:N], b[:N]))
            clean = _fails(lambda: check_trunk(case + " off", w, T0, N, N, LR.F16))
            assert not clean, clean                                                    # ... and pass without the switch
            del T0
        else:
            msgs = _fails(lambda: check_trunk(case, w, T, N, N, LR.F16))
            hit = [m for m in msgs if any(f"act{i} " in m for i in range(2, 10))]     # a 40x40 convolution
        assert hit, msgs
        msg = hit[0]
        net_ok = np.allclose(outs["t"], ref_t[:N], rtol=2e-2, atol=2e-3) and np.allclose(outs["r"], ref_r[:N], rtol=2e-2, atol=2e-3)
        notes.append(f"{case}: layer check -> {msg.splitlines()[0][:90]}; network-level tolerance {'PASSES (missed)' if net_ok else 'fails'}")
    print("\n" + "\n".join(notes))


def test_poisoned_scratch_changes_nothing(tl, model, crops, syn_mesh, scene):
    """every interior of the activation arena, the split-K partials, the f32 side buffer and the cross-attention scratch poisoned before
    each call (quiet NaN; +-largest finite, which a max()-ReLU cannot hide): the outputs equal the unpoisoned ones bit for bit, at
    N = 252 -> 7 -> 252 on one model and for Track (eager, then the graph)"""
    a, b = crops
    seq = (252, 7, 252)
    clean = [(model.refiner_infer(a[:n], b[:n]), model.scorer_infer(a[:n], b[:n])) for n in seq]
    hyp = syn.perturb_pose(scene.gt_pose)
    ok, clean_track = model.Track(scene.rgb, scene.depth, hyp, syn_mesh.name)
    assert ok
    for kind in (0, 1):
        for n, ((t0, r0), s0) in zip(seq, clean):
            assert tl.fpt_model_poison(model._h, kind) == 0
            t, r = model.refiner_infer(a[:n], b[:n])
            assert np.array_equal(t, t0) and np.array_equal(r, r0), (kind, n, "refiner")
            assert tl.fpt_model_poison(model._h, kind) == 0
            assert np.array_equal(model.scorer_infer(a[:n], b[:n]), s0), (kind, n, "scorer")
        for k in range(2):
            assert tl.fpt_model_poison(model._h, kind) == 0
            ok, p = model.Track(scene.rgb, scene.depth, hyp, syn_mesh.name)
            assert ok and np.array_equal(p, clean_track), (kind, k, "Track")
