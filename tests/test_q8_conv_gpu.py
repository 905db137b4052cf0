"""The 8-bit convolutions (FP_PREC_INT8 / FP_PREC_FP8 trunks) on raw bit patterns against a float64 reference, over every class of plan
step an accepted batch size can launch (tests/q8_conv_cases.py: the classes, the inputs, the reference and the comparison;
tests/test_q8_conv_cases_cpu.py holds the case list to plan_conv without a GPU and the comparison to its negative controls).

fpt_conv_q8_raw runs ONE convolution through run_conv with every operand in device form and returns the whole output buffers, canaries
included, the tables the layer uploaded and the plan that ran.  Cases that share (layer, images, operand type, family) share one float64
reference convolution, computed with torch on the GPU like tests/layer_ref.py does.  INT8 accumulates exactly, so its codes are held to
the float64 value up to the f32 roundings of the epilogue; FP8 adds the suite's accumulation constant (q8_conv_cases.C_ACC_FP8)."""
import collections
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import layer_ref as LR
import q8_conv_cases as Q
from foundationpose_cpp_amd import _lib
from test_conv_plan_cpu import Planner

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, FP8, I8 = Q.F16, Q.FP8, Q.I8
P = Planner()
CASES = Q.case_list()
GROUPS = collections.OrderedDict()           # (layer, NB, dt, 8-bit output type, family) -> [(N, odt)]: one reference convolution each
for _name, _N, _NB, _dt, _odt, _fam in CASES:
    GROUPS.setdefault((_name, _NB, _dt, Q.odt_q(_odt) if _dt == F16 else _dt, _fam), []).append((_N, _odt))
TABLE, TIMES = [], []


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(a, dt=None):
    return None if a is None else np.ascontiguousarray(a, dt)


def run_raw(o, tab, N, odt, raw16, raw8):
    """one fpt_conv_q8_raw call for output type odt: fills raw16 / raw8 -> (steps [(kernel, m_begin, M)], fused, tables the library uploaded)"""
    L = P.L
    L.fpt_conv_q8_raw.argtypes = [C.c_void_p] * 19
    L.fpt_conv_q8_raw.restype = C.c_int
    ly, dt, NB = o["layer"], o["dt"], o["NB"]
    g = Q.geometry(o, N, odt)
    OH, Cout = g["OH"], ly.Cout
    rk = 0 if not ly.res else 2 if Q.odt_rq(odt) else 1
    res = None
    if rk == 1:      # the residual's border is never read: quiet NaNs / the largest code
        res = np.full((NB, OH + 2, OH + 2, Cout), 0x7E00, np.uint16)
        res[:, 1:-1, 1:-1] = o["res16"].view(np.uint16)
    elif rk == 2:
        res = np.full((NB, OH + 2, OH + 2, Cout), 0x7F, np.uint8)
        res[:, 1:-1, 1:-1] = o["res8"]
    cfg = np.array([ly.Cin, Cout, ly.stride, NB, ly.HW, dt, odt, 1, g["split"], rk, g["opad"], 1, g["guard"]], np.int32)
    q8 = dt != F16
    wq = np.zeros((Cout, 9, ly.Cin), np.uint8) if q8 else None
    sw, cs, bu = (np.zeros(Cout, np.float32) for _ in range(3)) if q8 else (None, None, None)
    tm = np.zeros((ly.Cin, Cout), np.float32) if dt == I8 else None
    plan = np.zeros(26, np.int32)
    bimg = Q.bias_img_rows(o, tab) if Q.has_img_bias(N, dt, odt) else None
    rc = L.fpt_conv_q8_raw(_p(cfg), _p(o["x"]), _p(_c(o["w"], np.float32)), _p(o["bias"]), _p(o["s_in"]), _p(o["s_out"]) if tab["fold"] else None, _p(res),
                           _p(o["rscale"]) if rk == 2 else None, _p(_c(bimg)), _p(o["oinv"]) if Q.odt_scaled(odt) else None,
                           _p(_c(o["pe"].view(np.uint16))) if Q.offers_table(ly, odt) else None, _p(raw16), _p(raw8), _p(wq), _p(sw), _p(cs), _p(bu), _p(tm), _p(plan))
    assert rc == 0, (L.fp_last_error() or b"").decode()
    steps = [(Q.KERNELS[plan[2 + 6 * i]], int(plan[3 + 6 * i]), int(plan[4 + 6 * i])) for i in range(plan[0])]
    return steps, bool(plan[1]), {"wq": wq, "sw": sw, "cscale": cs, "bias_up": bu, "tmat_t": tm}


def check_tables(o, tab, up):
    """what the library uploaded is what the reference was computed from, bit for bit; INT8: tmat_t is the tap sum of the rounding errors"""
    if o["dt"] == F16:
        return
    assert np.array_equal(up["wq"], tab["wq"]) and np.array_equal(up["sw"].view(np.uint32), tab["sw"].view(np.uint32))
    assert np.array_equal(up["cscale"].view(np.uint32), tab["cscale"].view(np.uint32)), "cscale as uploaded"
    assert np.array_equal(up["bias_up"].view(np.uint32), tab["bias_up"].view(np.uint32)), "bias as uploaded (128-offset fold)"
    if o["dt"] == I8:
        ly = o["layer"]
        vf = (o["w"].reshape(ly.Cout, 9, ly.Cin) * o["s_in"][None, None, :]).astype(np.float32) / tab["sw"][:, None, None]      # the quantiser's f32 quotient
        t = (tab["wq"].view(np.int8).astype(np.float64) - vf.astype(np.float64)).sum(1).T                                          # [Cin][Cout]
        assert np.abs(up["tmat_t"] - t).max() <= 9 * 2.0 ** -22, float(np.abs(up["tmat_t"] - t).max())


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    if not TABLE:
        return
    worst = collections.defaultdict(lambda: [0.0, 0.0])
    share, need = collections.defaultdict(float), collections.defaultdict(float)
    for case, dtn, kern, form, ratio, ulp, sh in TABLE:
        if form == "f16":
            w = worst[(dtn, kern)]
            w[0], w[1] = max(w[0], ratio), max(w[1], abs(ulp))
        elif form == "C needed":
            need[kern] = max(need[kern], ratio)
        elif sh is not None:
            share[(dtn, form)] = max(share[(dtn, form)], sh)
    lines = [f"{'operands':<8} {'kernel':<10} {'worst err/bound':>16} {'worst |mean err| (ulp)':>24}"]
    lines += [f"{d:<8} {k:<10} {w[0]:>16.3f} {w[1]:>24.4f}" for (d, k), w in sorted(worst.items())]
    lines += [f"fp8      {k:<10} accumulation constant needed: {v:.2f} x C_ACC (used: {Q.C_ACC_FP8 / Q.C_ACC:.2f} x)" for k, v in sorted(need.items())]
    lines += [f"{d:<8} largest share of outputs {f}: {v:.2e}" for (d, f), v in sorted(share.items())]
    lines.append(f"{len(TABLE)} rows, {len(TIMES)} groups, {sum(TIMES):.1f} s in the groups (longest {max(TIMES):.1f} s), {time.time() - t0:.1f} s in all")
    print("\n" + "\n".join(lines))
    out = os.environ.get("FP_Q8_TABLE")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(f"{c:<60} {d:<4} {k:<9} {fo:<10} {'' if r is None else f'{r:10.3f}'} {'' if u is None else f'{u:9.4f}'} {'' if s is None else f'{s:9.2e}'}"
                                                         for c, d, k, fo, r, u, s in TABLE) + "\n")


@pytest.mark.parametrize("group", list(GROUPS), ids=lambda k: f"{k[0]}-NB{k[1]}-{Q.DT_NAME[k[2]]}-{Q.DT_NAME[k[3]]}-{k[4]}")
def test_q8_conv_step_classes(group):
    """every output form of one (layer, images, operand type, family) against one float64 reference convolution"""
    name, NB, dt, qo, fam = group
    t0 = time.time()
    o = Q.make_operands(name, NB, dt, fam, qo)
    tabs = {}
    fails, a = [], None
    for N, odt in GROUPS[group]:
        fold = odt in (I8, FP8)
        if fold not in tabs:
            tabs[fold] = Q.quantise(P.L, o, fold)
        tab = tabs[fold]
        if a is None:
            a, aa = Q.conv_sums(o, tab, DEV)
            if fam == "cancel" and o["layer"].res:
                Q.cancelling_residual(o, tab, a)
        ex = Q.expected(o, tab, a, aa, N, odt)
        g = Q.geometry(o, N, odt)
        raw16, raw8 = Q.canaries(g)
        raw16, raw8 = (raw16 if ex["two"] else None), (raw8 if ex["q"] is not None else None)
        steps, fused, up = run_raw(o, tab, N, odt, raw16, raw8)
        check_tables(o, tab, up)
        want, want_fused, _ = P.plan(o["layer"], NB, dt, odt, g["split"], Q.offers_table(o["layer"], odt))
        assert steps == [(Q.KERNELS[s[7]], s[3], s[4]) for s in want] and fused == bool(want_fused), (steps, want)
        f, rows = Q.check_outputs(raw16, raw8, ex, g, steps, fused, LR.stage_error)
        cid = Q.case_id((name, N, NB, dt, odt, fam))
        for kern, form, ratio, ulp, sh in rows:
            TABLE.append((cid, Q.DT_NAME[dt], kern, form, ratio, ulp, sh))
        fails += [f"{cid}: {x}" for x in f]
        del ex, raw16, raw8
    TIMES.append(time.time() - t0)
    print(f"{len(GROUPS[group])} cases in {TIMES[-1]:.1f} s")
    assert not fails, "\n".join(fails)
