"""The convolution / Linear schedule of fp_nn.hip (plan_conv) asked on the host, no GPU: fpt_plan_conv returns the steps a layer would
launch.  Over every conv / Linear shape of both networks (tests/layer_ref.py TRUNK), every batch 1..FP_MAX_BATCH with
the image counts the trunks use (2 N, and N + 1 for Register's shared crop) and every element-type pair run_conv dispatches, the plan
must be a sound one:
  * the row-covering steps partition [0, M): ascending, no gap, no overlap;
  * a step with ksplit > 1 is followed by exactly one reduce over the same rows, ksplit * kt_per >= KT and ksplit <= KT / 2 (and no
    reduce stands anywhere else);
  * the positional table is added on all rows or on none, never when it was not offered, and post_fused says which;
  * every grid has at least one workgroup;
  * a conv_deep_kernel<64> step is at most one round of the 256 CUs;
  * an 8-bit operand type never gets a kernel that exists for the 2-byte types only."""
import ctypes as C

import numpy as np
import pytest

from foundationpose_cpp_amd import _lib

N_MAX = 2377             # include/foundationpose_amd.h FP_MAX_BATCH
F16, BF16, FP8, I8, DUAL_FP8, DUAL_I8, QS_FP8, QS_I8, QSR_I8, F16RQ_I8 = range(10)      # fp_nn.h DT_*
KERNELS = ["SMALLX", "SMALLM", "STEM_HALO", "GEMM_K32", "S2_HALO", "HALO", "HALO8", "PP32", "BIG_PP", "PP", "DEEP64", "DEEP128", "IGEMM128",
           "IGEMM64", "SPLITK_REDUCE"]                                                    # fp_nn.hip ConvKernel
K = {n: i for i, n in enumerate(KERNELS)}
TWO_BYTE_ONLY = {K["SMALLM"], K["STEM_HALO"], K["GEMM_K32"], K["S2_HALO"], K["HALO"], K["PP32"]}
MAX_STEPS = 8


def _es(dt):
    return 1 if dt in (FP8, I8) else 2


class Layer:
    """one run_conv call: the layer, its input, and what the caller passes along"""

    def __init__(self, name, Cin, Cout, k, stride, pad, HW, imgs, res=False, concat=False, post=False, grp_rows=0):
        self.name, self.Cin, self.Cout, self.k, self.stride, self.pad, self.HW = name, Cin, Cout, k, stride, pad, HW
        self.imgs, self.res, self.concat, self.post, self.grp_rows = imgs, res, concat, post, grp_rows

    def out_hw(self):
        if self.k == 4:                  # the 7x7 / s2 stem as a 4x4 / s1 conv over the space-to-depth input: 160 -> 80
            return self.HW
        return (self.HW + 2 * self.pad - self.k) // self.stride + 1


# imgs: "ab" = the rendered and the observed crops (2 N, or N + 1 with a shared crop), "n" = N, "rows" = Linear on N * 400 tokens,
# "cross" = Linear on the N hypotheses of the scorer's cross attention, "grp" = the two refiner heads of Track as one grouped launch
TRUNK = [
    Layer("stem", 32, 64, 4, 1, 2, 80, "ab"),
    Layer("encodeA.1", 64, 128, 3, 2, 1, 80, "ab"),
    Layer("encodeA.2.conv1", 128, 128, 3, 1, 1, 40, "ab"),
    Layer("encodeA.2.conv2", 128, 128, 3, 1, 1, 40, "ab", res=True),
    Layer("encodeA.3.conv1", 128, 128, 3, 1, 1, 40, "ab"),
    Layer("encodeA.3.conv2", 128, 128, 3, 1, 1, 40, "ab", res=True, concat=True),
    Layer("encodeAB.0.conv1", 256, 256, 3, 1, 1, 40, "n"),
    Layer("encodeAB.0.conv2", 256, 256, 3, 1, 1, 40, "n", res=True),
    Layer("encodeAB.2", 256, 512, 3, 2, 1, 40, "n"),
    Layer("encodeAB.3.conv1", 512, 512, 3, 1, 1, 20, "n"),
    Layer("encodeAB.3.conv2", 512, 512, 3, 1, 1, 20, "n", res=True),
    Layer("encodeAB.4.conv2", 512, 512, 3, 1, 1, 20, "n", res=True, post=True),
]
LINEAR = [
    Layer("in_proj", 512, 1536, 1, 1, 0, 1, "rows"),
    Layer("out_proj", 512, 512, 1, 1, 0, 1, "rows", res=True),
    Layer("linear1", 512, 512, 1, 1, 0, 1, "rows"),
    Layer("cross.in_proj", 512, 1536, 1, 1, 0, 1, "cross"),
    Layer("cross.out_proj", 512, 512, 1, 1, 0, 1, "cross"),
]
GROUPED = [
    Layer("g.in_proj", 512, 1536, 1, 1, 0, 1, "grp", grp_rows=512),
    Layer("g.out_proj", 512, 512, 1, 1, 0, 1, "grp", res=True, grp_rows=512),
]

# (operand type, output type) pairs of run_conv, and the layers each can meet
PAIRS_2B = [(F16, F16), (BF16, BF16)]
PAIRS_A1_Q8 = [(F16, DUAL_FP8), (F16, DUAL_I8), (F16, QS_I8)]                             # encodeA.1 at the f16 -> 8-bit boundary
PAIRS_Q8 = [(FP8, FP8), (FP8, F16), (FP8, DUAL_FP8), (FP8, QS_FP8), (I8, I8), (I8, F16), (I8, DUAL_I8), (I8, QS_I8), (I8, QSR_I8), (I8, F16RQ_I8)]


class Planner:
    def __init__(self):
        self.L = _lib.test_lib()
        self.L.fpt_plan_conv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self.L.fpt_plan_conv.restype = C.c_int
        self.shape = np.zeros(10, np.int32)
        self.fields = np.zeros((MAX_STEPS, 11), np.int32)
        self.names = np.zeros((MAX_STEPS, 48), np.uint8)
        self.fused = np.zeros(1, np.int32)
        self.ptr = [a.ctypes.data for a in (self.shape, self.fields, self.names, self.fused)]

    def plan(self, ly, NB, dt, odt, split_imgs, offer_post):
        es = _es(dt)
        Kb = ly.k * ly.k * ly.Cin * es
        wfrag = Kb % 128 == 0 and ly.Cout % 16 == 0                                       # ConvLayer::wfrag (upload_layouts)
        wpack = es == 2 and ly.k == 1 and Kb % 64 == 0 and ly.Cout % 256 == 0 and not ly.grp_rows   # ConvLayer::wpack of a Linear layer
        self.shape[:] = (ly.Cin, ly.Cout, ly.k, ly.k, ly.stride, ly.pad, NB, ly.HW, ly.HW, ly.pad)
        flags = (1 if ly.res else 0) | (2 if offer_post else 0) | (4 if wfrag else 0) | (8 if wpack else 0)
        n = self.L.fpt_plan_conv(self.ptr[0], dt, odt, flags, split_imgs, ly.grp_rows, self.ptr[1], self.ptr[2], 48, MAX_STEPS, self.ptr[3])
        assert 1 <= n <= MAX_STEPS, (ly.name, NB, dt, odt, n)
        return self.fields[:n].tolist(), int(self.fused[0]), Kb // 128

    def name(self, i):
        return bytes(self.names[i]).split(b"\0")[0].decode()


def check(P, ly, NB, dt, odt, split_imgs=0):
    offer = ly.post and odt in (F16, BF16, F16RQ_I8)                                      # a positional table goes to 2-byte tokens only
    steps, fused, KT = P.plan(ly, NB, dt, odt, split_imgs, offer)
    M = NB * ly.out_hw() ** 2
    ctx = (ly.name, NB, dt, odt, steps)
    at, pe_rows, i = 0, [], 0
    while i < len(steps):
        net, prec, side, m0, m1, ksplit, pe, kern, kt_per, grid, lds = steps[i]
        assert (net, prec, side) == (-1, -1, 0), ctx
        assert kern != K["SPLITK_REDUCE"], ctx                                            # a reduce only stands behind its split-K launch
        assert m0 == at and m1 > m0 and m1 <= M, ctx                                      # ascending, no gap, no overlap
        assert grid >= 1 and ksplit >= 1 and lds >= 0, ctx
        if kern == K["DEEP64"]:
            assert grid <= 256, ctx
        if _es(dt) == 1:
            assert kern not in TWO_BYTE_ONLY, ctx
        at = m1
        if ksplit > 1:
            assert ksplit * kt_per >= KT and ksplit <= KT // 2 and pe == 0, ctx
            assert i + 1 < len(steps), ctx
            r = steps[i + 1]
            assert r[7] == K["SPLITK_REDUCE"] and r[3:6] == [m0, m1, ksplit] and r[9] >= 1 and r[8] == kt_per, ctx
            assert i + 2 == len(steps) or steps[i + 2][7] != K["SPLITK_REDUCE"], ctx
            pe = r[6]
            i += 1
        else:
            assert kt_per == KT, ctx
        pe_rows.append(pe)
        i += 1
    assert at == M, ctx
    assert len(set(pe_rows)) == 1 and pe_rows[0] == fused, ctx                            # on all rows or on none
    assert not fused or offer, ctx
    return steps


def _image_counts(N):
    return {2 * N, N + 1}                                                                 # own crops / Register's one shared crop


def _check_batch(P, N, pairs_2b=True, pairs_q8=True):
    n = 0
    for ly in TRUNK:
        for NB in (_image_counts(N) if ly.imgs == "ab" else {N}):
            split = N if ly.concat else 0                                                 # the a | b channel concat: images N.. are the observed crops
            pairs = []
            if pairs_2b:
                pairs += PAIRS_2B
            if pairs_q8 and ly.name == "encodeA.1":
                pairs += PAIRS_A1_Q8
            if pairs_q8 and ly.Cin >= 128:
                pairs += PAIRS_Q8
            for dt, odt in pairs:
                check(P, ly, NB, dt, odt, split)
                n += 1
    if pairs_2b:
        for ly in LINEAR:
            for dt, odt in PAIRS_2B:
                check(P, ly, N * 400 if ly.imgs == "rows" else N, dt, odt)
                n += 1
    return n


def test_every_plan_of_both_networks_is_sound():
    P = Planner()
    n = 0
    for N in range(1, N_MAX + 1):
        n += _check_batch(P, N)
    for ly in GROUPED:                                                                    # Track: both heads of the refiner in one launch
        for dt, odt in PAIRS_2B:
            steps = check(P, ly, 2 * ly.grp_rows, dt, odt)
            assert len(steps) == 1, steps
            n += 1
    assert n > 300000, n


PLAN_SIZES = [1, 2, 3, 4, 7, 8, 9, 16, 31, 32, 42, 64, 84, 126, 128, 252, 253, 504, 1008, 1009, 2352, 2377]


@pytest.mark.parametrize("setter,value", [("fpt_set_conv_variant", 3), ("fpt_set_conv_variant", 5), ("fpt_set_conv_variant", 7), ("fpt_set_conv_variant", 8),
                                          ("fpt_set_smallm", 0), ("fpt_set_smallm", 2), ("fpt_set_smallm", 3)])
def test_plans_under_the_alternative_schedules_are_sound(setter, value):
    P = Planner()
    default = {"fpt_set_conv_variant": 0, "fpt_set_smallm": 1}[setter]
    getattr(P.L, setter)(value)
    try:
        for N in PLAN_SIZES:
            _check_batch(P, N)
    finally:
        getattr(P.L, setter)(default)


def test_known_schedules():
    """a few plans spelled out, so that the hook is known to answer for the layer it was asked about"""
    P = Planner()
    conv512_pe = TRUNK[-1]
    # Track: one launch per layer on the small-problem kernel, the positional table in its epilogue
    s = check(P, conv512_pe, 1, F16, F16)
    assert [x[7] for x in s] == [K["SMALLX"]] and s[0][6] == 1 and P.name(0) == "conv_smallm_kernel"
    # Register, 252 hypotheses: 256x256 rounds + a deep-ring left-over, both with the table
    s = check(P, conv512_pe, 252, F16, F16)
    assert [x[7] for x in s] == [K["BIG_PP"], K["DEEP64"]] and [x[6] for x in s] == [1, 1], s
    assert s[0][3:5] == [0, 98304] and s[1][3:5] == [98304, 100800], s
    # the 3x3 / 40x40 layers of a large batch: the resident-halo kernels, by operand type
    assert [x[7] for x in check(P, TRUNK[6], 252, BF16, BF16)] == [K["HALO"]]
    assert [x[7] for x in check(P, TRUNK[6], 252, FP8, DUAL_FP8)] == [K["HALO8"]]
    # the Linear layers of Register
    assert [x[7] for x in check(P, LINEAR[0], 252 * 400, F16, F16)] == [K["GEMM_K32"]]
