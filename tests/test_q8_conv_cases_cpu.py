"""No GPU: the case list of tests/test_q8_conv_gpu.py against the library's own plan_conv, the inputs against the conditions that keep the
comparison from becoming vacuous, and the comparison function against perturbed reference results it must reject (tests/q8_conv_cases.py).

Completeness bites: with SMALL_DEEP_MAXKT of plan_conv changed from 18 to 17 in a scratch build (the 256-channel layers of a few
hypotheses then leave conv_deep_kernel<64>), test_every_step_class_has_a_gpu_case fails and names 18 classes, the first of them
  N=4    NB=4    encodeAB.0.conv1 ((256, 256, 40, 1), 'IGEMM128', 0, 'fp8', 'f16', 'none', 'none', False, False, False, False)
(conv_igemm_kernel<128> on a whole number of tiles, which no accepted batch reaches today), and test_case_list_is_pinned_to_the_plan
counts 718 classes for 712.
"""
import numpy as np
import pytest
import torch

import layer_ref as LR
import q8_conv_cases as Q
from test_conv_plan_cpu import Planner

F16, FP8, I8 = Q.F16, Q.FP8, Q.I8
MAX_IMAGES = 130


@pytest.fixture(scope="module")
def P():
    return Planner()


@pytest.fixture(scope="module")
def reachable(P):
    return Q.reachable_classes(P)


def test_every_step_class_has_a_gpu_case(P, reachable):
    """every class of the accepted space is a step of some case of the GPU test; a class that is missing is named with its smallest member"""
    covered = Q.covered_classes(P, Q.case_list())
    missing = sorted((v, c) for c, v in reachable.items() if c not in covered)
    print(f"\n{len(reachable)} step classes over the accepted space, {len(Q.case_list())} cases")
    assert not missing, "step classes without a GPU case:\n" + "\n".join(f"  N={N:<4} NB={NB:<4} {name} {c}" for (NB, N, name, _, _), c in missing)


def test_case_list_is_pinned_to_the_plan(P, reachable):
    """the list the GPU test runs is the one plan_conv gives today: a changed threshold changes the smallest members, and the frozen count
    and largest case below then no longer fit (update them together with DESIGN.md section 4.4)"""
    assert len(reachable) == 712, len(reachable)
    assert max(v[0] for v in reachable.values()) == 96
    kernels = {c[1] for c in reachable}
    assert kernels == {"SMALLX", "HALO8", "BIG_PP", "PP", "DEEP64", "IGEMM128", "S2_HALO"}, kernels


def test_no_class_needs_a_large_batch(reachable):
    big = {c: v for c, v in reachable.items() if v[0] > MAX_IMAGES}
    assert not big, big


def test_family_cases_reach_what_they_are_for(P):
    """the fixed list: a multi-step plan (rounds plus left-over) with a per-image bias, the shared-crop concat with one, the fused table
    behind rounds + deep ring, the 8-bit residual stream"""
    seen = {}
    for name, N, NB, dt, odt in Q.FAMILY_CASES:
        seen[(name, N, dt, odt)] = Q.step_classes(P, Q.LAYER[name], N, NB, dt, odt)
    multi = seen[("encodeAB.0.conv2", 47, I8, F16)]
    assert [c[1] for c in multi] == ["BIG_PP", "PP"] and all(c[10] for c in multi) and multi[1][7] and multi[1][8], multi
    codes = seen[("encodeAB.3.conv2", 84, I8, Q.QS_I8)]
    assert [c[1] for c in codes] == ["BIG_PP", "DEEP64"] and all(c[10] for c in codes) and codes[1][7], codes
    shared = seen[("encodeA.3.conv2", 33, I8, Q.DUAL_I8)]
    assert all(c[6] == "shared" and c[10] for c in shared), shared
    tok = seen[("encodeAB.4.conv2", 84, I8, F16)]
    assert [c[1] for c in tok] == ["BIG_PP", "DEEP64"] and all(c[9] and c[10] for c in tok), tok
    assert all(c[5] == "q8" for c in seen[("encodeA.2.conv2", 15, I8, Q.QSR_I8)])


def _reference(P, name, N, NB, dt, odt, family, qo=None, n_for_bias=None):
    o = Q.make_operands(name, NB, dt, family, qo)
    tab = Q.quantise(P.L, o, odt in (I8, FP8))
    a, aa = Q.conv_sums(o, tab, "cpu")
    if family == "cancel" and o["layer"].res:
        Q.cancelling_residual(o, tab, a)
    ex = Q.expected(o, tab, a, aa, N if n_for_bias is None else n_for_bias, odt)
    g = Q.geometry(o, N, odt)
    steps, fused, _ = P.plan(o["layer"], NB, dt, odt, g["split"], Q.offers_table(o["layer"], odt))
    return o, tab, a, ex, g, [(Q.KERNELS[s[7]], s[3], s[4]) for s in steps], bool(fused)


SMALL = [("encodeA.1", 1, 2, F16, Q.DUAL_I8, I8), ("encodeA.1", 1, 2, F16, Q.DUAL_FP8, FP8),
         ("encodeA.2.conv2", 2, 4, I8, Q.DUAL_I8, None), ("encodeA.2.conv2", 2, 4, FP8, Q.DUAL_FP8, None), ("encodeA.2.conv2", 2, 4, I8, Q.QSR_I8, None),
         ("encodeA.3.conv2", 2, 3, I8, Q.DUAL_I8, None), ("encodeAB.0.conv1", 1, 1, I8, I8, None), ("encodeAB.0.conv1", 1, 1, FP8, FP8, None),
         ("encodeAB.2", 2, 2, I8, Q.DUAL_I8, None), ("encodeAB.2", 2, 2, FP8, Q.QS_FP8, None),
         ("encodeAB.4.conv2", 1, 1, I8, F16, None), ("encodeAB.4.conv2", 1, 1, FP8, F16, None), ("encodeAB.4.conv2", 2, 2, I8, Q.F16RQ_I8, None)]
WITH_FAMILIES = {("encodeA.2.conv2", I8, Q.DUAL_I8), ("encodeA.2.conv2", FP8, Q.DUAL_FP8), ("encodeAB.4.conv2", I8, F16), ("encodeAB.4.conv2", FP8, F16)}


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0]}-NB{c[2]}-{Q.DT_NAME[c[3]]}-{Q.DT_NAME[c[4]]}")
def test_the_reference_alone_meets_the_conditions(P, case):
    """a correctly rounded result passes the comparison, and the inputs of every family keep the shares of excused outputs within their caps
    (CAP_CODES, CAP_TIES) and saturate next to nothing -- on the reference alone, whatever a device computes"""
    name, N, NB, dt, odt, qo = case
    for fam in (Q.FAMILIES if (name, dt, odt) in WITH_FAMILIES else ("relu",)):
        o, tab, a, ex, g, steps, fused = _reference(P, name, N, NB, dt, odt, fam, qo)
        r16, r8 = Q.ideal_outputs(ex, g, fused)
        fails, rows = Q.check_outputs(r16, r8, ex, g, steps, fused, LR.stage_error)
        shares = {r[1]: r[4] for r in rows if r[4] is not None}
        print(f"{Q.case_id((name, N, NB, dt, odt, fam))}: " + ", ".join(f"{k} {v:.2e}" for k, v in shares.items()))
        assert not fails, (fam, fails)
        assert shares.get("saturated", 0.0) <= 1e-3, shares


# ---- negative controls: perturbations of a reference result that check_outputs must reject ----
def _rejects(what, ex, g, steps, fused, r16, r8, margin):
    fails, _ = Q.check_outputs(r16, r8, ex, g, steps, fused, LR.stage_error)
    print(f"control: {what}: {margin} -> " + (fails[0] if fails else "ACCEPTED"))
    assert fails, what


def _with_v(ex, v):
    d = dict(ex)
    d["v"] = v
    return d


@pytest.mark.parametrize("dt,odt", [(I8, Q.DUAL_I8), (FP8, Q.DUAL_FP8)], ids=["int8", "fp8"])
def test_controls_on_values(P, dt, odt):
    name, N, NB = "encodeA.2.conv2", 2, 4
    o, tab, a, ex, g, steps, fused = _reference(P, name, N, NB, dt, odt, "relu")
    ok16, ok8 = Q.ideal_outputs(ex, g, fused)
    assert not Q.check_outputs(ok16, ok8, ex, g, steps, fused, LR.stage_error)[0]
    C = g["Cout"]
    # one 128-byte K-step (128 input channels of one tap) dropped in one 16-pixel x 16-channel tile
    xv = Q.act_values(torch.from_numpy(o["x"]), dt)
    wv = torch.from_numpy(tab["wq"].view(np.int8).astype(np.float64) if dt == I8 else Q.E4M3[tab["wq"]])
    img, oh, ow0, co0, tap = 1, 17, 16, 48, 4                                  # the centre tap: input pixel = output pixel
    part = xv[img, oh, ow0:ow0 + 16, :128] @ wv[co0:co0 + 16, tap, :128].T     # [16 px, 16 ch] in code units
    v = ex["v"].clone()
    drop = part * torch.from_numpy(tab["cscale"][co0:co0 + 16].astype(np.float64))
    v[img, oh, ow0:ow0 + 16, co0:co0 + 16] -= drop
    r16, r8 = Q.ideal_outputs(_with_v(ex, v), g, fused)
    bound = 0.5 * LR.ulp(ex["v"][img, oh, ow0:ow0 + 16, co0:co0 + 16].abs(), LR.F16) + ex["e"][img, oh, ow0:ow0 + 16, co0:co0 + 16]
    _rejects("one K-step dropped in one 16 x 16 tile", ex, g, steps, fused, r16, r8, f"median |drop| / bound = {float((drop.abs() / bound).median()):.0f}")
    _rejects("the same, seen by the 8-bit copy alone", ex, g, steps, fused, ok16, r8,
             f"median |drop| = {float((drop.abs() * ex['oinv'][co0:co0 + 16]).median()):.1f} code steps" if dt == I8 else "e4m3 codes")
    # truncation instead of round-to-nearest-even in the codes
    t = ex["v"].clamp_min(0) * ex["oinv"]
    if dt == I8:
        trunc = torch.floor(t).clamp(0, 255).to(torch.uint8).numpy() ^ np.uint8(0x80)
    else:
        q = Q.q_e4m3(t)
        vals = torch.from_numpy(np.sort(Q.E4M3[:0x7f]))
        down = vals[(torch.searchsorted(vals, t.reshape(-1), right=True) - 1).clamp_min(0)].reshape(t.shape)      # towards zero
        trunc = Q.e4m3_bits(torch.minimum(q, down).numpy())
    r8 = ok8.copy()
    r8[:NB, 1:-1, 1:-1, :] = trunc
    _rejects("truncation instead of RNE in the codes", ex, g, steps, fused, ok16, r8, f"{float((torch.from_numpy(r8 != ok8).double().mean())):.2f} of the bytes differ by one code")
    # a ragged last tile left unwritten (rows of the last partial 16-row tile of the step), one border byte overwritten
    r16, r8 = ok16.copy(), ok8.copy()
    pat16, pat8 = Q.canaries(g)
    r16[NB - 1, -2, -9:-1, :] = pat16[NB - 1, -2, -9:-1, :]
    r8[NB - 1, -2, -9:-1, :] = pat8[NB - 1, -2, -9:-1, :]
    _rejects("the last 8 rows left unwritten", ex, g, steps, fused, r16, r8, f"{8 * C} elements hold the canary")
    r8 = ok8.copy()
    r8[1, 0, 5, 3] = 0x80 if dt == I8 else 0x00
    _rejects("one border byte of the 8-bit copy overwritten with the zero-code", ex, g, steps, fused, ok16, r8, "1 byte")
    r16 = ok16.copy()
    r16[NB, 3, 3, 3] = 0
    _rejects("one element of the guard image overwritten", ex, g, steps, fused, r16, ok8, "1 element")


def test_control_offset_fold(P):
    """the -128 offset folded as -127: every tap is off by one code, the value by cscale * (sum of the row's codes)"""
    o, tab, a, ex, g, steps, fused = _reference(P, "encodeAB.4.conv2", 1, 1, I8, F16, "relu")
    shift = torch.from_numpy(tab["cscale"].astype(np.float64) * tab["qsum"])
    r16, r8 = Q.ideal_outputs(_with_v(ex, ex["v"] + shift), g, fused)
    bound = 0.5 * LR.ulp(ex["v"].clamp_min(0) + ex["pe"].reshape(1, 20, 20, -1), LR.F16) + 0.5 * LR.ulp(ex["v"].clamp_min(0), LR.F16) + ex["e"]
    ratio = (shift.abs() / bound)[ex["v"] > 0]
    _rejects("offset fold wrong by one code per tap", ex, g, steps, fused, r16, r8, f"median |shift| / bound = {float(ratio.median()):.1f}, {float((ratio > 1).double().mean()):.2f} of the outputs beyond it")
    assert float((ratio > 1).double().mean()) > 0.25


def test_control_per_image_bias_of_the_neighbour(P):
    """one tile's rows take the per-image bias row of the next image (the multi-step index bug: m_begin left out of the image index)"""
    o, tab, a, ex, g, steps, fused = _reference(P, "encodeAB.3.conv2", 3, 3, I8, Q.DUAL_I8, "relu", n_for_bias=Q.IMG_BIAS_MIN_N)
    d = torch.from_numpy(o["delta_img"].astype(np.float64))
    v = ex["v"].clone()
    v[1, 4:8] += (d[2] - d[1])                                                 # rows 80..159 of image 1: five 16-row tiles
    r16, r8 = Q.ideal_outputs(_with_v(ex, v), g, fused)
    bound = 0.5 * LR.ulp(ex["v"][1, 4:8].abs(), LR.F16) + ex["e"][1, 4:8]
    ratio = ((d[2] - d[1]).abs() / bound)[ex["v"][1, 4:8] > 0]
    _rejects("a tile with the neighbouring image's bias row", ex, g, steps, fused, r16, r8, f"median |difference| / bound = {float(ratio.median()):.0f}")
    _rejects("the same, seen by the 8-bit copy alone", ex, g, steps, fused, Q.ideal_outputs(ex, g, fused)[0], r8,
             f"median |difference| = {float(((d[2] - d[1]).abs() * ex['oinv']).median()):.2f} code steps")


def test_control_concat_one_image_off(P):
    """the b-half of the concat written one image off (own crops), and written at all for the images a shared crop leaves alone"""
    o, tab, a, ex, g, steps, fused = _reference(P, "encodeA.3.conv2", 2, 4, FP8, Q.DUAL_FP8, "relu")
    ok16, ok8 = Q.ideal_outputs(ex, g, fused)
    assert not Q.check_outputs(ok16, ok8, ex, g, steps, fused, LR.stage_error)[0]
    C = g["Cout"]
    r16, r8 = ok16.copy(), ok8.copy()
    r16[:2, ..., C:] = ok16[[1, 0]][..., C:]
    r8[:2, ..., C:] = ok8[[1, 0]][..., C:]
    _rejects("b-half one image off", ex, g, steps, fused, r16, r8, "two unrelated images")
    o, tab, a, ex, g, steps, fused = _reference(P, "encodeA.3.conv2", 2, 3, I8, Q.DUAL_I8, "relu")
    ok16, ok8 = Q.ideal_outputs(ex, g, fused)
    assert not Q.check_outputs(ok16, ok8, ex, g, steps, fused, LR.stage_error)[0]
    r8 = ok8.copy()
    r8[1, 1:-1, 1:-1, C:] = ok8[0, 1:-1, 1:-1, C:]
    _rejects("shared crop: the b-half of image 1 written by the layer", ex, g, steps, fused, ok16, r8, f"{1600 * C} bytes")


def test_dropped_control_table_before_the_first_rounding():
    """NOT a control, on purpose.  A fused epilogue that added the table before rounding the token, rnd(c + pe) for rnd(rnd(c) + pe), is
    within 0.5 ulp of the reference c + pe: the bound 0.5 ulp(ref) + 0.5 ulp(c) + e (layer_ref.stage_error, second_rounding) provably
    cannot see it, because it must admit the first rounding that the shipped form makes.  Which of the two the device computes is pinned
    bit for bit where both forms run: tests/test_layers_gpu.py holds the fused epilogues to add_pos_embed_kernel's bits."""
    c, pe = torch.tensor([0.300048828125], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64)
    before = (c + pe).to(torch.float16).to(torch.float64)
    worst, _ = LR.stage_error(before, c + pe, torch.zeros(1, dtype=torch.float64), LR.F16, second_rounding=c)
    assert worst <= 1.0
