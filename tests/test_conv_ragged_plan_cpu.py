"""The ragged 256x256 rounds of plan_conv (fp_nn.hip) asked on the host, no GPU.

A layer whose rows leave a small rest behind the full rounds of 256x256 tiles gets ONE conv_big_pp_kernel launch in which some row tiles
are 288 rows tall, instead of the rounds + a left-over launch.  The rule, restated here from the layer's shape alone:
  2-byte operands that are also the output type; Cout % 256 == 0 and the 256x256 rounds apply at all (the plan without the switch starts
  with them at row 0); the default schedule switches; no positional table offered; at least one full round; rows_left > 0;
  n_tall = ceil(rows_left / 32) with n_tall * (Cout / 256) <= 256 (every tall tile in the first round) and 256 % (Cout / 256) == 0 (the
  kernel's tile -> row map).
With fpt_set_conv_ragged(1) (the default) the plan is that single step exactly when the rule holds, and otherwise -- every 8-bit pair and
every query that offers the table included -- the plan of fpt_set_conv_ragged(0), field for field."""
import ctypes as C

import numpy as np
import pytest

from foundationpose_cpp_amd import _lib

N_MAX = 2377             # include/foundationpose_amd.h FP_MAX_BATCH
F16, BF16, FP8, I8, DUAL_FP8, DUAL_I8, QS_FP8, QS_I8, QSR_I8, F16RQ_I8 = range(10)      # fp_nn.h DT_*
BIG_PP, DEEP64 = 8, 10   # fp_nn.hip ConvKernel
MAX_STEPS = 8
LDS_TALL = 2 * (288 * 128 + 256 * 128)
PAIRS_2B = [(F16, F16), (BF16, BF16)]
PAIRS_Q8 = [(FP8, FP8), (FP8, F16), (FP8, DUAL_FP8), (FP8, QS_FP8), (I8, I8), (I8, F16), (I8, DUAL_I8), (I8, QS_I8), (I8, QSR_I8), (I8, F16RQ_I8)]

# name, Cin, Cout, stride, input H = W, residual: the five 20x20 layers of a network are one conv_b2, conv_512 (conv1) and conv_512 + residual
SHAPES = [("conv_b2", 256, 512, 2, 40, False), ("conv_512", 512, 512, 1, 20, False), ("conv_512+res", 512, 512, 1, 20, True)]


class Planner:
    def __init__(self):
        self.L = _lib.test_lib()
        self.L.fpt_plan_conv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self.L.fpt_plan_conv.restype = C.c_int
        self.L.fpt_plan_conv_tall.argtypes = [C.c_int]
        self.L.fpt_plan_conv_tall.restype = C.c_int
        self.L.fpt_set_conv_ragged.argtypes = [C.c_int]
        self.L.fpt_set_conv_ragged.restype = None
        self.shape = np.zeros(10, np.int32)
        self.fields = np.zeros((MAX_STEPS, 11), np.int32)
        self.names = np.zeros((MAX_STEPS, 48), np.uint8)
        self.fused = np.zeros(1, np.int32)
        self.ptr = [a.ctypes.data for a in (self.shape, self.fields, self.names, self.fused)]

    def plan(self, shape, N, dt, odt, post=False):
        """-> (steps [[11 fields + the step's tall tiles + its name]], post_fused)"""
        _, Cin, Cout, stride, HW, res = shape
        es = 1 if dt in (FP8, I8) else 2
        wfrag = (9 * Cin * es) % 128 == 0 and Cout % 16 == 0
        self.shape[:] = (Cin, Cout, 3, 3, stride, 1, N, HW, HW, 1)
        flags = (1 if res else 0) | (2 if post else 0) | (4 if wfrag else 0)
        n = self.L.fpt_plan_conv(self.ptr[0], dt, odt, flags, 0, 0, self.ptr[1], self.ptr[2], 48, MAX_STEPS, self.ptr[3])
        assert 1 <= n <= MAX_STEPS, (shape, N, dt, odt, n)
        steps = [self.fields[i].tolist() + [self.L.fpt_plan_conv_tall(i), bytes(self.names[i]).split(b"\0")[0].decode()] for i in range(n)]
        assert self.L.fpt_plan_conv_tall(n) == -1
        return steps, int(self.fused[0])


@pytest.fixture()
def planner():
    P = Planner()
    yield P
    P.L.fpt_set_conv_ragged(1)


def _both(P, *query, **kw):
    P.L.fpt_set_conv_ragged(0)
    off = P.plan(*query, **kw)
    P.L.fpt_set_conv_ragged(1)
    return P.plan(*query, **kw), off


def _rule(Cout, M, off_steps):
    """(holds, row tiles of the full rounds, tall tiles) from the shape; off_steps only says whether the 256x256 rounds apply at all"""
    nt = Cout // 256
    mt_big = (M // 256 * nt // 256) * 256 // nt
    rows_left = M - mt_big * 256
    n_tall = (rows_left + 31) // 32
    rounds = Cout % 256 == 0 and off_steps[0][7] == BIG_PP and off_steps[0][3] == 0
    return rounds and mt_big > 0 and rows_left > 0 and n_tall * nt <= 256 and 256 % nt == 0, mt_big, n_tall


def test_ragged_rounds_exactly_where_the_rule_holds(planner):
    P = planner
    ragged = {}
    for shape in SHAPES:
        Cout = shape[2]
        for dt, odt in PAIRS_2B:
            hits = 0
            for N in range(1, N_MAX + 1):
                M = N * 400
                (on, on_fused), (off, off_fused) = _both(P, shape, N, dt, odt)
                assert all(s[11] == 0 for s in off), (shape, N, dt, off)                 # the switch-off plan never has a tall tile
                holds, mt_big, n_tall = _rule(Cout, M, off)
                if not holds:
                    assert (on, on_fused) == (off, off_fused), (shape, N, dt, on, off)
                    continue
                hits += 1
                assert len(on) == 1 and on_fused == 0, (shape, N, dt, on)
                net, prec, side, m0, m1, ksplit, pe, kern, kt_per, grid, lds, tall, name = on[0]
                assert (net, prec, side, m0, m1, ksplit, pe) == (-1, -1, 0, 0, M, 1, 0), (shape, N, dt, on)
                assert kern == BIG_PP and name == "conv_big_pp_kernel" and lds == LDS_TALL, (shape, N, dt, on)
                assert kt_per == 9 * shape[1] * 2 // 128, (shape, N, dt, on)
                assert grid == mt_big * (Cout // 256) and grid % 256 == 0 and tall == n_tall, (shape, N, dt, on)
                assert 0 <= mt_big * 256 + 32 * tall - M < 32                             # the tiles reach M and overshoot by less than a slice
                assert tall * (Cout // 256) <= 256                                         # every tall tile in the first round of 256 workgroups
                # what it replaces: the same rounds + one left-over step (N = 82..: conv_deep_kernel<64>)
                assert off[0][3:5] == [0, mt_big * 256] and off[0][9] == grid and off[-1][4] == M, (shape, N, dt, off)
            ragged[(shape[0], dt)] = hits
    assert len(set(ragged.values())) == 1 and min(ragged.values()) > 250, ragged           # the rest is at most 4096 of a round's 32768 rows: one batch size in eight


def test_n252_spelled_out(planner):
    P = planner
    for shape in SHAPES:
        (on, _), (off, _) = _both(P, shape, 252, F16, F16)
        assert [s[3:5] + [s[7], s[9], s[11]] for s in on] == [[0, 100800, BIG_PP, 768, 78]], on
        assert [s[3:5] + [s[7], s[9], s[11]] for s in off] == [[0, 98304, BIG_PP, 768, 0], [98304, 100800, DEEP64, 156, 0]], off
        assert 78 * 288 + (384 - 78) * 256 == 100800


def test_a_query_that_offers_the_table_keeps_its_plan(planner):
    P = planner
    shape = SHAPES[2]
    for dt, odt in PAIRS_2B:
        for N in range(1, N_MAX + 1):
            on, off = _both(P, shape, N, dt, odt, post=True)
            assert on == off, (N, dt, on, off)
    (on, fused), _ = _both(P, shape, 252, F16, F16, post=True)                            # the plan tests/test_conv_plan_cpu.py pins
    assert [s[3:5] + [s[6], s[7]] for s in on] == [[0, 98304, 1, BIG_PP], [98304, 100800, 1, DEEP64]] and fused == 1, on


def test_no_8bit_pair_changes_its_plan(planner):
    P = planner
    for shape in SHAPES:
        for dt, odt in PAIRS_Q8:
            if shape[0] == "conv_b2" and odt in (QSR_I8, F16RQ_I8):                       # (the 8-bit residual belongs to layers with one)
                continue
            for N in range(1, N_MAX + 1):
                on, off = _both(P, shape, N, dt, odt)
                assert on == off, (shape, N, dt, odt, on, off)
                assert all(s[11] == 0 for s in on[0]), on


def test_the_other_switches_turn_the_ragged_rounds_off(planner):
    P = planner
    P.L.fpt_set_conv_variant.argtypes = [C.c_int]
    P.L.fpt_set_conv_ablate.argtypes = [C.c_int]
    for setter, value in (("fpt_set_conv_variant", 5), ("fpt_set_conv_variant", 8), ("fpt_set_conv_ablate", 1)):
        getattr(P.L, setter)(value)
        try:
            for shape in SHAPES:
                on, off = _both(P, shape, 252, F16, F16)
                assert on == off and all(s[11] == 0 for s in on[0]), (setter, value, on)
        finally:
            getattr(P.L, setter)(0)
