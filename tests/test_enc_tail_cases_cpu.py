"""tests/enc_tail_cases.py held to the library and to itself, without a GPU.

Completeness: over every batch 1..FP_MAX_BATCH in both element types fpt_plan_heads launches the encoder tail as enc_tail_kernel<., 1> on 25
tiles (Track) or enc_tail_kernel<., 5> on 5 N tiles and nothing else, the QKV projection of two sequences and more as qkv_tile_kernel on 5 N
tiles; grid and LDS bytes are the numbers the cases module restates (and tests/test_enc_tail_gpu.py finds in the hooks' info).  A new form
or instantiation fails here by name.
Constants: the float32 emulation (three summation orders) stays inside every bound on every case, and each K_* lies in [2, 2.5] x the peak
re-measured here.
Negative controls: the comparators reject a float64 chain with one defect, on every case the defect can change; the factors by which each
misses its bound are printed (pytest -s) and the weakest are in DESIGN.md section 3.

Controls that stay inside the bound, listed and not counted:
  * `eps` (1e-6 for 1e-5) wherever a row's variance is not within a few hundred eps: it scales the normalised row by 1 + 4.5e-6 / var,
    below a thousandth of u for var ~ 1.  It is counted on ln_const, whose near-constant rows have a variance of 4 eps.
  * `res3_unrounded` (the residual of GEMM 3 taken before its rounding): it moves y2 by at most half an ulp of x1 -- less than the one unit
    roundoff of the LayerNorm-2 input that U is -- and by a quarter ulp of either sign on average.  Measured below, never required.
  * truncation of y1, x1 or the hidden layer: a truncated intermediate in FRONT of a GEMM or a LayerNorm is mixed by zero-mean weights
    or re-centred and leaves no signed mean in z; truncation of y2 shrinks every row by a factor that LayerNorm 2 divides out again.
    Their figures are printed.  Truncation of the LayerNorm-2 output, the last intermediate in front of the column sums, is counted on
    every case but the common-mode ones (where z's own rounding is a few per cent of U): the signed-mean assertion fires.
  * on the bf16 common-mode case (ulp(30) = 1/8 exceeds the spread of 0.1 that x1 carries) whatever changes y1 or a few channels; the four
    gross defects behind x1 are counted there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import enc_tail_cases as EC
import layer_ref as LR
from foundationpose_cpp_amd import _lib

REFINER, FEATURES = 0, 1
QKV_TILE = 1


def test_the_plan_launches_only_forms_that_have_cases():
    L = _lib.test_lib()
    L.fpt_plan_heads.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.fpt_plan_heads.restype = C.c_int
    L.fpt_set_enc_tail(1); L.fpt_set_ln_pmean(1); L.fpt_set_fuse_pose(1); L.fpt_set_qkv_ablate(0); L.fpt_set_att_variant(1)
    f, t = np.zeros(18, np.int32), np.zeros(3, np.int32)
    enc_classes = {EC.enc_class(MI, dt, tiles) for MI, dt, tiles, _ in EC.CASES}
    qkv_classes = {EC.qkv_class(dt, tiles) for dt, tiles, _ in EC.QKV_CASES}
    seen = set()
    for dt in (EC.F16, EC.BF16):
        for N in range(1, EC.N_MAX + 1):
            for offer in (0, 1):
                assert L.fpt_plan_heads(REFINER, N, dt, offer, f.ctypes.data, t.ctypes.data) == 0, (N, dt)
                MI = 1 if N == 1 else 5
                tiles = N * 400 // EC.TOKENS[MI]
                assert int(f[14]) == EC.TAIL_ONE[MI], f"N = {N}, dt = {dt}: tail form {int(f[14])} has no case in tests/enc_tail_cases.py"
                assert tuple(t) == (tiles, 2 * tiles, EC.LDS_TAIL[MI]), (N, dt, t.tolist())
                assert EC.enc_class(MI, dt, tiles) in enc_classes, (N, dt)
                seen.add((MI, dt))
            for pas in (REFINER, FEATURES):
                assert L.fpt_plan_heads(pas, N, dt, 0, f.ctypes.data, t.ctypes.data) == 0, (pas, N, dt)
                if int(f[0]) == QKV_TILE:
                    assert (int(f[1]), int(f[2]), int(f[3])) == (0, 5 * N, EC.LDS_QKV), (pas, N, dt, f.tolist())
                    assert EC.qkv_class(dt, 5 * N) in qkv_classes, (pas, N, dt)
                else:
                    assert N == 1, f"pass {pas}, N = {N}: the QKV projection left qkv_tile_kernel (form {int(f[0])})"
    assert seen == {(MI, dt) for MI in (1, 5) for dt in (EC.F16, EC.BF16)}          # the four instantiations, all reached
    assert (1, EC.F16, 25, "iid") in EC.CASES and (1, EC.BF16, 25, "iid") in EC.CASES   # the workload's own shape


def test_the_case_list_is_what_the_issue_lists():
    ids = [EC.case_id(c) for c in EC.CASES]
    assert len(set(ids)) == len(ids)
    for dt in (EC.F16, EC.BF16):
        assert {t for MI, d, t, fam in EC.CASES if (MI, d, fam) == (5, dt, "iid")} >= {1, 2, 10, 7}
        assert {t for MI, d, t, fam in EC.CASES if (MI, d, fam) == (1, dt, "iid")} >= {1, 25, 3}
        assert {t for d, t, fam in EC.QKV_CASES if (d, fam) == (dt, "iid")} == {1, 2, 3, 7, 10}
        for MI in (1, 5):
            assert {fam for m, d, _, fam in EC.CASES if (m, d) == (MI, dt)} == set(EC.FAMILIES)      # every family in both types and both MI
        assert {fam for d, _, fam in EC.QKV_CASES if d == dt} == {"iid", "perm", "onehot", "top"}
    assert max(t * EC.TOKENS[MI] for MI, _, t, _ in EC.CASES) == 81 * 80
    assert {(n, parts) for n, parts, _, fused in EC.HEADS_CASES if not fused} == {(n, parts) for n in (1, 2, 3) for parts in (1, 5, 25)}
    assert all(n == 1 for n, _, _, fused in EC.HEADS_CASES if fused)


def test_the_written_out_chain_is_layer_refs_encoder_chain():
    for case in [(5, EC.F16, 2, "iid"), (1, EC.BF16, 8, "ln_const"), (1, EC.F16, 3, "relu_open"), (5, EC.BF16, 2, "ln_spike")]:
        p = EC.make_problem(case)
        for h in range(2):
            a, b = EC.chain(p, h), EC.reference_chain(p, h)
            for k in ("y1", "x1", "hid", "y2", "ln2"):
                assert torch.equal(a[k], b[k]), (case, h, k)


def test_inputs_are_seeded_in_the_element_type_and_below_half_its_range():
    for case in EC.CASES:
        if case[2] > 10:
            continue
        p, q = EC.make_problem(case), EC.make_problem(case)
        assert p.att.dtype == EC.TORCH_DT[case[1]] and torch.equal(p.att, q.att) and torch.equal(p.x, q.x) and torch.equal(p.W, q.W)
        assert torch.equal(p.W, p.W.to(EC.TORCH_DT[case[1]]).float())                       # the weights are values of the element type
        assert not torch.equal(p.W[0], p.W[1]) and not torch.equal(p.g[0], p.g[1]) and not torch.equal(p.b[0], p.b[1])
        assert EC.reference(p)["peak"] <= 0.5 * EC.DT_MAX[case[1]]
    hw = EC.probes(EC.CASES[0])
    assert hw.shape == (EC.N_ONEHOT + EC.N_DENSE, 2, 3, 512) and (hw[:EC.N_ONEHOT].sum((0, 2)) == 1).all()    # every column in exactly one row


def test_family_properties_hold_on_the_reference():
    """the degenerate inputs are what their names say, read off the float64 chain"""
    for dt in (EC.F16, EC.BF16):
        for MI in (1, 5):
            tiles = 2 if MI == 5 else 3
            p = EC.make_problem((MI, dt, tiles, "relu_dead"))
            assert all(c in EC.CASES for c in [(MI, dt, tiles, "relu_dead"), (MI, dt, 8, "ln_const"), (MI, dt, 8, "ln_mode")])
            r = EC.reference_chain(p, 0)
            assert float(r["hid"].abs().max()) == 0.0                                           # y2 = b2 + x1
            assert torch.equal(r["y2"], LR.rnd(r["x1"] + p.b[0, 2].double(), dt))
            p = EC.make_problem((MI, dt, tiles, "relu_open"))
            c = EC.chain(p, 0, no_relu=True)
            assert torch.equal(c["hid"], EC.reference_chain(p, 0)["hid"]) and float(c["hid"].min()) > 0     # nothing is clipped
            p = EC.make_problem((MI, dt, 8, "ln_const"))
            r = EC.reference_chain(p, 1)
            const = r["y1"][p.const_rows]                                                       # one exactly constant row per tile, all odd
            assert len(p.const_rows) == 8 and (p.const_rows % 2 == 1).all() and len(set(p.const_rows % EC.TOKENS[MI])) == 8
            assert bool((const == const[:, :1]).all()) and torch.equal(r["x1"][p.const_rows], LR.rnd(p.be[1, 0].double(), dt).expand_as(const))
            odd = np.setdiff1d(np.arange(1, p.rows, 2), p.const_rows)
            var = r["y1"][odd].var(-1, unbiased=False)
            assert 1e-5 < float(var.min()) and float(var.max()) < 1e-4                         # within a few eps of eps
            p = EC.make_problem((MI, dt, 8, "ln_mode"))
            y2 = EC.reference_chain(p, 0)["y2"]
            assert float(y2.mean(-1).abs().min()) > 25 and float(y2.std(-1).max()) < 0.15       # mean >> spread in front of LayerNorm 2
            p = EC.make_problem((MI, dt, tiles, "ln_spike"))
            assert float(p.x.double().abs().max()) > 100
            p = EC.make_problem((MI, dt, tiles, "perm"))
            assert all(bool(((p.W[h, i] != 0).sum(0) == 1).all() and ((p.W[h, i] != 0).sum(1) == 1).all()) for h in range(2) for i in range(3))
            assert not torch.equal(p.W[0, 0], p.W[0, 1]) and not torch.equal(p.W[0, 1], p.W[0, 2])


@pytest.fixture(scope="module")
def measured():
    return EC.emulation_peaks()


def test_the_emulation_stays_inside_every_bound(measured):
    _, rows = measured
    fails = []
    for case, order, c in rows:
        p = EC.make_problem(case) if case[2] <= 3 else None
        fam_tok = (case[3], EC.TOKENS[case[0]])
        hard, stat, mean = EC.K_ELEM, (None if fam_tok[0] not in EC.INDEPENDENT else (EC.K_16 if fam_tok[1] == 16 else EC.K_80)), EC.K_MEAN
        print(f"{EC.case_id(case):26s} {order:12s} worst {c['worst']:.4f} (hard {hard}, statistical {stat})  signed mean {c['mean']:+.2e} over {c['n']}")
        if p is not None:
            assert EC.limits(p) == (hard, stat, mean)
        if not c["worst"] <= (hard if stat is None else min(hard, stat)) or not abs(c["mean"]) <= mean:
            fails.append((EC.case_id(case), order, c))
    assert not fails, fails


def test_the_constants_are_twice_the_emulations_peaks(measured):
    peaks, _ = measured
    print("emulation peaks:", {k: f"{v:.4g}" for k, v in peaks.items()})
    for name, K in (("elem", EC.K_ELEM), ("k16", EC.K_16), ("k80", EC.K_80), ("mean", EC.K_MEAN)):
        assert 2.0 * peaks[name] <= K <= 2.5 * peaks[name], f"{name}: constant {K} against a re-measured peak of {peaks[name]:.5g}"


# ---- negative controls -------------------------------------------------------------------------------------------------------------------
def _control_cases():
    for dt in (EC.F16, EC.BF16):
        for MI in (1, 5):
            t = 2 if MI == 5 else 3
            for fam in EC.FAMILIES:
                yield next(c for c in EC.CASES if c[:2] == (MI, dt) and c[3] == fam and (fam != "iid" or c[2] == t))
            yield (MI, dt, 10 if MI == 5 else 25, "iid")


def _controls(case):
    """{name: (mutation, the assertion that must be among those that fire)} of the controls that can change this case"""
    MI, dt, tiles, fam = case
    behind = MI - 1                                   # the last token fragment: behind KR at MI = 5
    frag = 0 if fam == "live" else behind             # (tile 0 of `live` holds its one live token in fragment 0)
    gross = {"residual of GEMM 3 missing": (dict(no_res3=True), None),
             "LN1 and LN2 parameters swapped": (dict(swap_ln=True), None),
             "head 1 with head 0's weights": (dict(head_swap=True), None),
             "ReLU missing": (dict(no_relu=True), None)}
    if (fam, dt) == ("ln_mode", EC.BF16):     # ulp(30) = 1/8 in bf16 exceeds the spread of 0.1 that x1 carries: what changes y1 or a few
        return gross                          # channels does not survive x1's rounding; the gross defects behind it are counted
    out = dict(gross)
    out.update({"residual of GEMM 1 missing": (dict(no_res1=True), None),
                "biases b2 of channels 200..207 shifted by 8": (dict(bias_shift=(2, 200)), None),
                "att row t with residual row t + 16": (dict(x_shift=16), None)})
    if fam != "ln_mode":                              # (there x1 = 30 + 0.1 x_hat: a sixteenth of y1 moves it by a fifth of its ulp)
        out["K-step 5 of GEMM 1 dropped for one fragment"] = (dict(drop=(0, frag, 5)), None)
        out["LN2 output truncated"] = (dict(trunc="z"), "mean")       # (ln_mode: z's own rounding is a few per cent of U)
    if fam in ("iid", "perm", "ln_spike", "relu_open", "live"):
        out["K-step 11 of GEMM 2 dropped for one fragment"] = (dict(drop=(1, frag, 11)), None)
        out["K-step 0 of GEMM 3 dropped for one fragment"] = (dict(drop=(2, frag, 0)), None)
        out["biases b1 of channels 8..15 shifted by 8"] = (dict(bias_shift=(1, 8)), None)
    if fam != "ln_const":                             # (b_o is zero there)
        out["biases bo of channels 504..511 shifted by 8 (from 496..)"] = (dict(bias_shift=(0, 488)), None)
    if fam == "relu_open":                            # (nothing is clipped there: the chain without the ReLU is the same chain)
        del out["ReLU missing"]
    if fam == "ln_const":
        out["LN eps 1e-6"] = (dict(eps=1e-6), None)
    return out


UNCOUNTED = {"residual of GEMM 3 unrounded": dict(res3_unrounded=True), "y1 truncated": dict(trunc="y1"), "y2 truncated": dict(trunc="y2"), "x1 truncated": dict(trunc="x1"),
             "hidden layer truncated": dict(trunc="hid"), "LN eps 1e-6 (outside ln_const)": dict(eps=1e-6)}


def _miss(p, c):
    hard, stat, mean = EC.limits(p)
    return c["worst"] / (hard if stat is None else stat), abs(c["mean"]) / mean


def test_every_control_is_rejected_on_every_case_it_can_change():
    weakest, fails = {}, []
    for case in _control_cases():
        p = EC.make_problem(case)
        ref = EC.reference(p)
        base = EC.compare(p, ref, ref["S"])
        assert base["worst"] == 0.0 and EC.verdict(p, base) == []
        for name, (mut, must) in _controls(case).items():
            c = EC.compare(p, ref, EC.mutated_sums(p, **dict(mut)))
            v = EC.verdict(p, c)
            amp, mean = _miss(p, c)
            print(f"{EC.case_id(case):24s} {name:58s} fails {','.join(v) or '-':14s} worst / bound {amp:10.3g}  |mean| / bound {mean:10.3g}")
            weakest[name] = min(weakest.get(name, (float("inf"), None)), (max(amp, mean), EC.case_id(case)))
            if not v or (must and must not in v):
                fails.append(f"{EC.case_id(case)}: '{name}' -> {v} (worst / bound {amp:.3g}, mean / bound {mean:.3g})")
    for name, (m, cid) in sorted(weakest.items(), key=lambda kv: kv[1]):
        print(f"weakest miss of '{name}': {m:.3g} x its bound ({cid})")
    assert not fails, "\n".join(fails)


def test_the_uncounted_controls_are_measured():
    """(no assertion on the verdict: the module docstring says why each may stay inside the bound)"""
    for case in [(5, EC.F16, 81, "live"), (1, EC.F16, 17, "live"), (5, EC.BF16, 2, "iid"), (1, EC.F16, 8, "ln_mode")]:
        p = EC.make_problem(case)
        ref = EC.reference(p)
        for name, mut in UNCOUNTED.items():
            c = EC.compare(p, ref, EC.mutated_sums(p, **dict(mut)))
            amp, mean = _miss(p, c)
            print(f"{EC.case_id(case):24s} {name:36s} fails {','.join(EC.verdict(p, c)) or '-':10s} worst / bound {amp:8.3g}  |mean| / bound {mean:8.3g}")
            assert np.isfinite(amp)


# ---- qkv_tile_kernel and enc_heads_kernel ------------------------------------------------------------------------------------------------
def test_qkv_emulation_passes_and_its_controls_fail():
    for case in EC.QKV_CASES:
        dt, tiles, fam = case
        x, W, b, exact = EC.make_qkv_problem(case)
        ref, acc = EC.qkv_reference(x, W, b)
        got = EC.qkv_emulate(x, W, b)
        if exact:
            assert torch.equal(got, ref.to(EC.TORCH_DT[dt])), case           # one exact product per output: bit for bit, infinities included
            if fam == "top":
                n_inf = int(torch.isinf(got.float()).sum())
                assert 0 < n_inf < got.numel() // 20, (case, n_inf)
                continue
        else:
            worst, bias = LR.stage_error(got.double(), ref, acc, dt)
            assert worst <= 1.0 and abs(bias) <= LR.BIAS_ULP, (case, worst, bias)
        rotated = torch.roll(ref, EC.EMBED, 1)                                 # Q / K / V blocks rotated by one
        w1, _ = LR.stage_error(LR.rnd(rotated, dt), ref, acc, dt)
        assert w1 > 1.0, (case, w1)
        if tiles > 1:                                                          # tile 1 computed from tile 0's rows
            moved = ref.clone()
            moved[EC.QKV_TOKENS:2 * EC.QKV_TOKENS] = ref[:EC.QKV_TOKENS]
            w2, _ = LR.stage_error(LR.rnd(moved, dt), ref, acc, dt)
            assert w2 > 1.0, (case, w2)
            print(f"{EC.qkv_case_id(case):20s} rotated blocks {w1:10.3g} x the bound, neighbouring tile's rows {w2:10.3g} x")


def test_heads_reference_and_its_sequential_emulation():
    for case in EC.HEADS_CASES:
        n, parts, fam, _ = case
        pd, bias = EC.make_heads_problem(case)
        y, bound, y32 = EC.heads_reference(pd, bias, n, parts, fam.startswith("rough"))
        assert y.shape == (2, n, 3) and np.isfinite(y).all() and np.isnan(pd[..., 3]).all()
        r = np.abs(y32 - y) / bound
        print(f"{EC.heads_case_id(case):22s} sequential f32 emulation: {r.max():.3f} of the bound")
        assert r.max() <= 1.0, case
        if parts > 1:                        # controls: the last tile left out; divided by 80 tokens instead of 400
            v = pd.reshape(2, n, parts, 4)[..., :3].astype(np.float64)
            assert (np.abs(v[:, :, :-1].sum(2) / EC.SEQ_TOKENS + bias[:, None] - y) > bound).any()
        assert (np.abs((y - bias[:, None]) * 5 + bias[:, None] - y) > bound).any()
