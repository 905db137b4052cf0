"""The 288-row tiles of conv_big_pp_kernel (the ragged 256x256 rounds) on single layers, at the smallest shapes
that can go wrong: 20x20 output maps with Cin = 64 (9 K-steps), one or two rounds of the 256 CUs.

Each case runs the layer through fpt_conv_dt (run_conv on device tensors; its output buffer stands between canaries) with the ragged rounds
on and off -- the outputs must be the same bits, every row keeps its summation order -- and against a float64 convolution of the same
rounded operands at the tolerance of the f16 / bf16 layer cases of tests/test_precision_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from foundationpose_cpp_amd import _lib

pytestmark = pytest.mark.gpu

DT_F16, DT_BF16 = 0, 1
BIG_PP = 8               # fp_nn.hip ConvKernel
TOL = {DT_F16: 2e-3, DT_BF16: 8e-3}    # rtol = atol: the output is rounded to the element type (2^-11 / 2^-8 relative) + summation order

# id: NB, Cout, stride, input H = W, residual, tall tiles of the one launch (0 = the rule does not hold: rounds + left-over, as before)
CASES = {
    "overshoot": (83, 512, 1, 20, False, 14),      # M = 33 200, rest 432: 14 tall tiles reach 16 rows past M -> clamped loads, masked stores
    "exact": (84, 512, 1, 20, True, 26),           # rest 832 = 26 x 32: an exact partition; with the residual
    "stride2": (83, 512, 2, 40, False, 14),        # conv_b2's addressing
    "one_ntile": (165, 256, 1, 20, False, 15),     # one channel tile: 256 row tiles per round, M = 66 000
    "two_rounds": (166, 512, 1, 20, False, 27),    # M = 66 400: tall tiles first, then a round of 256-row tiles at shifted offsets
    "rule_off": (93, 512, 1, 20, False, 0),        # rest 4 432 -> 139 tall tiles x 2 > 256: the old plan still launches
}
RUNS = [(c, DT_F16) for c in CASES] + [("overshoot", DT_BF16), ("two_rounds", DT_BF16)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _quant(a, dt):
    t = torch.from_numpy(a)
    return (t.to(torch.bfloat16) if dt == DT_BF16 else t.to(torch.float16)).to(torch.float32)


@pytest.fixture()
def lib():
    L = _lib.test_lib()
    L.fpt_conv_dt.argtypes = [C.c_void_p] * 4 + [C.c_int] * 13 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    L.fpt_plan_conv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.fpt_set_conv_ragged.argtypes = [C.c_int]
    L.fpt_set_conv_ragged.restype = None
    yield L
    L.fpt_set_conv_ragged(1)


def _plan(L, NB, Cout, stride, H, res, dt):
    shape = np.array([64, Cout, 3, 3, stride, 1, NB, H, H, 1], np.int32)
    fields, names, fused = np.zeros((8, 11), np.int32), np.zeros((8, 48), np.uint8), np.zeros(1, np.int32)
    n = L.fpt_plan_conv(_p(shape), dt, dt, (1 if res else 0) | 4, 0, 0, _p(fields), _p(names), 48, 8, _p(fused))
    return [fields[i].tolist() + [L.fpt_plan_conv_tall(i)] for i in range(n)]


@pytest.mark.parametrize("case,dt", RUNS, ids=[f"{c}-{'bf16' if d else 'f16'}" for c, d in RUNS])
def test_ragged_rounds_same_bits_and_float64(lib, case, dt):
    L = lib
    NB, Cout, stride, H, use_res, n_tall = CASES[case]
    Cin, OH = 64, (H + 2 - 3) // stride + 1
    M = NB * OH * OH
    rng = np.random.default_rng(11)
    x = rng.normal(size=(NB, H, H, Cin)).astype(np.float32)
    w = (rng.normal(size=(Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    b = rng.normal(size=Cout).astype(np.float32)
    res = rng.normal(size=(NB, OH, OH, Cout)).astype(np.float32) if use_res else None
    wk = np.ascontiguousarray(w.transpose(0, 2, 3, 1))

    # the plans the two runs take
    L.fpt_set_conv_ragged(1)
    on = _plan(L, NB, Cout, stride, H, use_res, dt)
    L.fpt_set_conv_ragged(0)
    off = _plan(L, NB, Cout, stride, H, use_res, dt)
    assert [s[7] for s in off][0] == BIG_PP and len(off) >= 2 and off[-1][4] == M and all(s[11] == 0 for s in off), off
    if n_tall:
        assert len(on) == 1 and on[0][3:5] == [0, M] and on[0][7] == BIG_PP and on[0][11] == n_tall, on
        assert on[0][9] == off[0][9] and on[0][9] % 256 == 0, (on, off)                  # the same whole rounds
    else:
        assert on == off, (on, off)

    got = {}
    for ragged in (1, 0):
        L.fpt_set_conv_ragged(ragged)
        out = np.zeros((NB, OH, OH, Cout), np.float32)
        rc = L.fpt_conv_dt(_p(x), _p(wk), _p(b), _p(res), NB, H, H, Cin, Cout, 3, 3, stride, 1, OH, OH, 1, 0, _p(out), 1, None, dt, dt, 1.0, 1.0, 1.0)
        assert rc == 0, (ragged, rc, L.fp_last_error())                                  # 2: a canary next to the output buffer changed
        got[ragged] = out
    L.fpt_set_conv_ragged(1)

    # float64 reference of the rounded operands, computed once
    dev = torch.device("cuda")
    y = torch.nn.functional.conv2d(_quant(x, dt).to(dev).permute(0, 3, 1, 2).double(), _quant(w, dt).to(dev).double(),
                                   torch.from_numpy(b).to(dev).double(), stride, 1).permute(0, 2, 3, 1)
    if use_res:
        y = y + _quant(res, dt).to(dev).double()
    ref = torch.relu(y).float().cpu().numpy()
    del y

    same = got[1].view(np.uint32) == got[0].view(np.uint32)
    bad_rows = np.unique(np.nonzero(~same.reshape(M, Cout))[0])
    err = np.abs(got[1] - ref) - TOL[dt] * np.abs(ref)
    print(f"{case} dt={dt}: M={M} tall={n_tall} rows that differ on/off: {bad_rows.size} (first {bad_rows[:8].tolist()}); "
          f"max |got - ref| - rtol |ref| = {err.max():.3e} (atol {TOL[dt]:.0e})")
    assert bad_rows.size == 0, (case, bad_rows[:16].tolist())
    np.testing.assert_allclose(got[1], ref, rtol=TOL[dt], atol=TOL[dt])
    np.testing.assert_allclose(got[0], ref, rtol=TOL[dt], atol=TOL[dt])
