"""tests/attention_cases.py held to the library and to itself, without a GPU.

Completeness: every attention launch fpt_plan_heads plans over the accepted space falls into a class (attention_cases.att_class) that a
`kernel = -1` case of CASES runs, and the case list holds the SMALLEST member of every class as the library plans it -- so moving
ATT_SKV_MAX_WGS or a tile size demands new cases here, by name.
Negative controls: the checks of tests/test_attention_gpu.py can fail.  The float64 reference of a problem with its last key dropped, its
last key counted twice, or the values of two neighbouring keys swapped lies outside the bound of the unmutated problem.
Emulation: the kernels' arithmetic written out plainly (attention_cases.emulate_kernel) stays inside the bound and the bias limit for
every family, so a correct kernel can pass.

Measured with these families (T = 32, 33, 97, 400, 2377; f16 and bf16): the emulation peaks at 0.52 of the bound (f16 ramp, T = 32); its
mean error pooled as the GPU test pools it stays within 0.013 ulp (f16 gauss, T = 33), while single draws of a [33, 512] output reach
0.093 ulp (f16 offset) -- the reason for pooling (attention_cases.n_draws).  The weakest required control is 11.0x the bound (bf16 ramp,
last key counted twice, T = 2377).  `offset` is a numerical case and carries no control: its common-mode score leaves a near-uniform
softmax over 2377 keys, where one key more or less moves the output by about the bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cases as AC
import layer_ref as LR
from foundationpose_cpp_amd import _lib

CONTROL_T = (33, 97, 400, 2377)
DROP_LAST, DOUBLE_LAST, SWAP_VALUES = "last key dropped", "last key counted twice", "values of keys T/2 and T/2 + 1 swapped"
CONTROLS = {DROP_LAST: ("gauss", "ramp", "lastkey", "onehot"), DOUBLE_LAST: ("gauss", "ramp", "lastkey"), SWAP_VALUES: ("gauss", "onehot")}


def _library_space():
    """accepted_space() with the kernel the LIBRARY plans; the launch arithmetic restated in attention_cases is held to it on the way"""
    L = _lib.test_lib()
    L.fpt_plan_heads.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.fpt_plan_heads.restype = C.c_int
    L.fpt_set_att_variant(1)
    f, t = np.zeros(18, np.int32), np.zeros(3, np.int32)
    for dt in (AC.F16, AC.BF16):
        for pas, N, shape in AC.accepted_space():
            assert L.fpt_plan_heads(pas, N, dt, 0, f.ctypes.data, t.ctypes.data) == 0, (pas, N, dt)
            kernel, remap, ablate, B, T, pitch, nq, grid = (int(v) for v in f[4:12])
            assert (B, T, pitch) == shape and (remap, ablate) == (1, 0), (pas, N, dt, f.tolist())
            assert (nq, grid) == AC.launch_shape(kernel, B, T), (pas, N, dt, f.tolist())
            yield pas, N, shape, kernel, dt


def _describe(c):
    return ", ".join(f"{n} = {v}" for n, v in zip(AC.CLASS_FIELDS[c[0]], c))


def test_every_class_the_plan_reaches_has_a_case():
    space = list(_library_space())
    planned = {(s, dt): k for _, _, s, k, dt in space}
    covered = set()
    for B, T, pitch, dt, kernel, _ in AC.CASES:
        if kernel == -1 and ((B, T, pitch), dt) in planned:
            covered.add((AC.att_class(planned[(B, T, pitch), dt], B, T, pitch), dt))
    cases = {c[:5] for c in AC.CASES if c[4] == -1}
    pass_name = ("refiner", "scorer features", "cross-attention")
    missing = []
    for dt in (AC.F16, AC.BF16):
        smallest = AC.smallest_per_class((p, N, s, k) for p, N, s, k, d in space if d == dt)
        for c, (pas, N, shape) in sorted(smallest.items()):
            where = f"{'bf16' if dt else 'f16'} class ({_describe(c)}), smallest at {pass_name[pas]} N = {N}: (B, T, pitch) = {shape}"
            if (c, dt) not in covered:
                missing.append("no kernel = -1 case runs " + where)
            elif shape + (dt, -1) not in cases:
                missing.append("the smallest member is not a case of " + where)
    stale = sorted({(s, k) for (s, _), k in planned.items() if k != AC.planned_kernel(s[0], s[1])})
    if stale:
        (B, T, pitch), k = stale[0]
        missing.append(f"attention_cases.planned_kernel restates another plan than the library's at {len(stale)} shapes, the smallest "
                       f"(B, T, pitch) = ({B}, {T}, {pitch}): the library plans {('attention32_kernel', 'attention32_skv_kernel')[k]}")
    assert not missing, "\n".join(missing)
    assert len({c for c, _ in covered}) == len(AC.reachable_classes()) == 76     # DESIGN.md states the number


def test_the_case_list_is_what_the_issue_lists():
    ids = [AC.case_id(c) for c in AC.CASES]
    assert len(set(ids)) == len(ids)
    for B, T, pitch in [(17, 33, 33), (17, 97, 97), (2, 400, 512), (5, 400, 400), (1, 32, 32), (1, 33, 33), (1, 2048, 2048), (1, 2049, 2049),
                        (1, 2058, 2058), (1, 2352, 2352), (1, 2377, 2377), (1, 4754, 4754)]:
        for dt in (AC.F16, AC.BF16):
            for fam in AC.FAMILIES:
                assert (B, T, pitch, dt, -1, fam) in AC.CASES
    assert AC.planned_kernel(17, 33) == AC.planned_kernel(17, 97) == AC.ATT_32       # the product's attention32_kernel at 2 and 4 key blocks
    for dt in (AC.F16, AC.BF16):
        assert all((1, T, T, dt, AC.ATT_32, "gauss") in AC.CASES for T in (33, 64, 65, 96, 97, 128, 129, 160, 161))
        assert all((1, T, T, dt, AC.ATT_SKV, "gauss") in AC.CASES for T in (1, 31, 32, 2049))
    # the pipeline prologue and the loop tail of attention32_kernel at 1..12 key blocks, forced or planned
    blocks = {-(-c[1] // 32) for c in AC.CASES if AC.expected_kernel(c) == AC.ATT_32}
    assert {1, 2, 3, 4, 5, 6} <= blocks
    assert max(c[0] * c[1] for c in AC.CASES) <= 4754                                 # one small launch each


def _problem(T, dt, fam, draw=0):
    x, perm = AC.make_inputs(1, T, dt, fam, draw)
    return (x, perm) + LR.sdpa(x, dt, round_out=False)


@pytest.fixture(scope="module")
def problems():
    """(T, dt, family) -> (x, perm, ref, acc): one sequence of every family at the control lengths, its float64 reference and bound term"""
    return {(T, dt, fam): _problem(T, dt, fam) for T in CONTROL_T for dt in (AC.F16, AC.BF16) for fam in AC.FAMILIES}


def _mutated(x, how):
    q, k, v = AC.split_heads(x)
    T = q.shape[2]
    if how == DROP_LAST:
        k, v = k[:, :, :T - 1], v[:, :, :T - 1]
    elif how == DOUBLE_LAST:
        k, v = torch.cat([k, k[:, :, T - 1:]], 2), torch.cat([v, v[:, :, T - 1:]], 2)
    else:
        idx = torch.arange(T)
        idx[T // 2], idx[T // 2 + 1] = T // 2 + 1, T // 2
        v = v[:, :, idx]
    return AC.plain_attention(q, k, v)


def test_the_bound_catches_a_miscounted_or_misplaced_key(problems):
    weakest, fails = (float("inf"), None), []
    for (T, dt, fam), (x, _, ref, acc) in problems.items():
        same = AC.plain_attention(*AC.split_heads(x))
        assert float((same - ref).abs().max()) <= 1e-12 * float(ref.abs().max())      # the mutations start from the reference itself
        for how, fams in CONTROLS.items():
            if fam not in fams:
                continue
            worst, _ = LR.stage_error(_mutated(x, how), ref, acc, dt)
            print(f"T {T:5d} {'bf16' if dt else 'f16 '} {fam:8s} {how:40s} err / bound {worst:10.1f}")
            weakest = min(weakest, (worst, (T, dt, fam, how)))
            if not worst > 1.0:
                fails.append(f"T = {T}, dt = {dt}, {fam}: {how} stays inside the bound (err / bound = {worst:.3f})")
    print("weakest control:", weakest)
    assert not fails, "\n".join(fails)


def test_onehot_selects_one_value_exactly(problems):
    for (T, dt, fam), (x, perm, ref, _) in problems.items():
        if fam == "onehot":
            v = x[..., 2 * AC.EMBED:]
            want = torch.take_along_dim(v, perm[:, :, None], 1)
            assert torch.equal(ref.to(x.dtype), want), (T, dt)         # the float64 reference rounds to v[perm] bit for bit


def test_the_kernels_arithmetic_stays_inside_the_bound(problems):
    """... on every draw; the mean error pooled over the draws the GPU test pools (attention_cases.n_draws).  T = 32 joins the control
    lengths here: the smallest output whose mean error is asserted."""
    peak, peak_bias, fails = (0.0, None), (0.0, None), []
    for T in (32,) + CONTROL_T:
        for dt in (AC.F16, AC.BF16):
            for fam in AC.FAMILIES:
                worst, biases = 0.0, []
                for draw in range(AC.n_draws(1, T)):
                    x, perm, ref, acc = problems[T, dt, fam] if draw == 0 and T in CONTROL_T else _problem(T, dt, fam, draw)
                    got = AC.emulate_kernel(x)
                    w, b = LR.stage_error(got.double(), ref, acc, dt)
                    worst = max(worst, w)
                    biases.append(b)
                    if fam == "onehot" and not torch.equal(got, torch.take_along_dim(x[..., 2 * AC.EMBED:], perm[:, :, None], 1)):
                        fails.append(f"T = {T}, dt = {dt}, onehot: not v[perm] bit for bit")
                bias = sum(biases) / len(biases)
                print(f"T {T:5d} {'bf16' if dt else 'f16 '} {fam:8s} err / bound {worst:6.3f}  bias {bias:+.4f} ulp over {len(biases)} draw(s), "
                      f"single draws up to {max(abs(b) for b in biases):.4f}")
                peak, peak_bias = max(peak, (worst, (T, dt, fam))), max(peak_bias, (abs(bias), (T, dt, fam)))
                assert T * AC.EMBED >= AC.BIAS_MIN_ELEMS
                if not worst <= 1.0:
                    fails.append(f"T = {T}, dt = {dt}, {fam}: err / bound = {worst:.3f}")
                if not abs(bias) <= LR.BIAS_ULP:
                    fails.append(f"T = {T}, dt = {dt}, {fam}: mean error {bias:.4f} ulp")
    print("peak err / bound:", peak, " peak |bias|:", peak_bias)
    assert not fails, "\n".join(fails)


def test_inputs_are_seeded_and_in_the_element_type():
    for dt in (AC.F16, AC.BF16):
        for fam in AC.FAMILIES:
            a, pa = AC.make_inputs(2, 45, dt, fam)
            b, pb = AC.make_inputs(2, 45, dt, fam)
            assert a.dtype == AC.TORCH_DT[dt] and a.shape == (2, 45, 1536) and torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
            assert (pa is None) == (fam != "onehot") and (pa is None or torch.equal(pa, pb))
