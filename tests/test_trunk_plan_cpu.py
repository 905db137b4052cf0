"""The wiring of the shared CNN trunk (fp_nn.hip, plan_trunk) asked on the host, no GPU: fpt_plan_trunk returns, for each of the 15
convolutions, which tensors it reads and writes in which element type, which scale tables its epilogue gets, and what runs around it
(per-image bias, shared-crop broadcast, q8_copy, calibration record).  Every plan is held to the table written out below -- the 2-byte
networks, FP8 and INT8 under all 16 stage masks, the test build's 8-bit residual stream, with and without the per-image compensation,
on both sides of its batch threshold, with own crops and the shared one -- and to invariants that need no table at all."""
import ctypes as C
import itertools

import numpy as np
import pytest

from foundationpose_cpp_amd import _lib

N_MAX = 2377                                   # include/foundationpose_amd.h FP_MAX_BATCH
F16, BF16, FP8, I8 = 0, 1, 2, 3                # fp_nn.h DT_*
NONE = -1
NN_IN, STEM, X128, X256, X512, TOKENS = 0, 1, 2, 5, 8, 11      # fp_nn.hip TrunkSlot (X128 + i, i = 0..2, and so on)
FIELDS = ("op_dt", "in", "in_q", "res", "res_q", "rscale", "out16", "outq", "oinv", "img_bias", "bcast16", "bcastq", "qcopy",
          "rec", "rec_q", "rec_dt", "rec_scale")
DT_FIELDS = ("op_dt", "rec_dt")
STAGE_A, STAGE_B, STAGE_S, STAGE_C = 1, 2, 4, 8                 # encodeA.2-3 / encodeAB.0-1 / encodeAB.2 / encodeAB.3-4
IMG_BIAS_MIN_N = 16
ALL_ROWS = 0x7FFC                              # rows 2..14: every layer an INT8 network quantises carries its tap sums

# the 15 convolutions in order: (input, output, skip operand); a row's index is the trunk activation it writes
ROWS = [(NN_IN, STEM, NONE), (STEM, X128 + 0, NONE),
        (X128 + 0, X128 + 1, NONE), (X128 + 1, X128 + 2, X128 + 0), (X128 + 2, X128 + 1, NONE), (X128 + 1, X256 + 0, X128 + 2),
        (X256 + 0, X256 + 1, NONE), (X256 + 1, X256 + 2, X256 + 0), (X256 + 2, X256 + 1, NONE), (X256 + 1, X256 + 0, X256 + 2),
        (X256 + 0, X512 + 0, NONE),
        (X512 + 0, X512 + 1, NONE), (X512 + 1, X512 + 2, X512 + 0), (X512 + 2, X512 + 1, NONE), (X512 + 1, TOKENS, X512 + 2)]
CONCAT_ROW = 5                                 # encodeA.3.conv2 writes the a|b channel concat


class Planner:
    def __init__(self):
        self.L = _lib.test_lib()
        self.L.fpt_plan_trunk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_void_p]
        self.L.fpt_plan_trunk.restype = C.c_int
        self.f = np.zeros((15, 17), np.int32)

    def rc(self, dt, qdt, mask, i8s, comp, comp_rows, N, n_b):
        return self.L.fpt_plan_trunk(dt, qdt, mask, i8s, comp, comp_rows, N, n_b, self.f.ctypes.data)

    def plan(self, *q):
        self.f[:] = -7
        assert self.rc(*q) == 0, q
        return [dict(zip(FIELDS, row)) for row in self.f.tolist()]


@pytest.fixture(scope="module")
def P():
    return Planner()


def step(dt, r, **kw):
    """a row on 2-byte operands that writes and records its 2-byte output; kw overrides"""
    i, o, res = ROWS[r]
    s = dict(op_dt=dt, **{"in": i}, in_q=0, res=res, res_q=0, rscale=NONE, out16=o, outq=NONE, oinv=NONE, img_bias=0, bcast16=0, bcastq=0,
             qcopy=NONE, rec=o if r >= 1 else NONE, rec_q=0, rec_dt=dt if r >= 1 else NONE, rec_scale=NONE)
    s.update(kw)
    return s


def expected(dt, qdt, mask, i8s, comp, comp_rows, N, n_b):
    """THE TABLE"""
    shared = 1 if (n_b == 1 and N > 1) else 0
    if qdt < 0:                # a 2-byte network: every row alike, the shared crop's half of the concat replicated
        return [step(dt, r, bcast16=shared if r == CONCAT_ROW else 0) for r in range(15)]
    q = qdt
    if qdt == I8 and i8s:      # the 8-bit residual stream (test build): whatever the mask says, no f16 tensor between encodeA.1 and the tokens
        rec_q = dict(rec_q=1, rec_dt=q)
        out_q = lambda r: dict(out16=NONE, outq=ROWS[r][1], rec_scale=r, **rec_q)
        t = [step(F16, 0), step(F16, 1, **out_q(1), oinv=1)]
        for r in range(2, 15):
            first = ROWS[r][2] == NONE and r != 10
            s = step(F16, r, op_dt=q, in_q=1)
            if r < 14:         # a block's first conv: the consumer's scales are folded in; the others scale in the epilogue
                s.update(out_q(r), oinv=NONE if first else r)
            if ROWS[r][2] != NONE:        # the skip operand is the 8-bit copy, de-quantised with the scales of the activation it holds
                s.update(res_q=1, rscale={3: 1, 5: 3, 7: 5, 9: 7, 12: 10, 14: 12}[r])
            if r == CONCAT_ROW:
                s.update(bcastq=shared)
            t.append(s)
        return t
    # FP8 / INT8 with the f16 residual stream
    A, B, S, Cc = (bool(mask & b) for b in (STAGE_A, STAGE_B, STAGE_S, STAGE_C))
    bias = lambda r: 1 if (q == I8 and comp and (comp_rows >> r) & 1 and N >= IMG_BIAS_MIN_N) else 0

    def first(r, on):          # first conv of a residual block: 8-bit -> 8-bit alone with the consumer's scales folded in, or plain f16
        if not on:
            return step(F16, r)
        return step(F16, r, op_dt=q, in_q=1, out16=NONE, outq=ROWS[r][1], img_bias=bias(r), rec_q=1, rec_dt=q, rec_scale=r)

    def second(r, on, want16, wantq):
        """a conv whose output starts or continues the f16 stream (skip operand f16): writes the f16 tensor and / or the 8-bit copy
        an 8-bit consumer wants -- from its own epilogue when it is 8-bit itself, through q8_copy otherwise"""
        s = step(F16, r, op_dt=q if on else F16, in_q=1 if on else 0, img_bias=bias(r) if on else 0)
        if on and wantq:
            s.update(outq=ROWS[r][1], oinv=r)
        elif wantq:
            s.update(qcopy=r)
        if not want16:
            s.update(out16=NONE, rec_q=1, rec_dt=q, rec_scale=r)
        return s

    t = [step(F16, 0),
         # encodeA.1 (f16 operands) starts the 128-channel stream; it is not recorded in these trunks
         step(F16, 1, rec=NONE, rec_dt=NONE, **(dict(outq=X128 + 0, oinv=1) if A else {})),
         first(2, A), second(3, A, True, A), first(4, A), second(5, A, True, B),
         first(6, B), second(7, B, True, B), first(8, B),
         second(9, B, not (B and S), S),      # feeds only encodeAB.2: no f16 copy when that reads 8-bit operands from an 8-bit producer
         second(10, S, True, Cc),
         first(11, Cc), second(12, Cc, True, Cc), first(13, Cc), second(14, Cc, True, False)]
    t[CONCAT_ROW].update(bcast16=shared, bcastq=shared if (A and B) else 0)
    return t


SIZES = (1, 2, 15, 16, 42, N_MAX)
CLASSES = [(F16, -1, 0), (BF16, -1, 0)] + [(F16, q, m) for q in (FP8, I8) for m in range(16)]


def queries():
    for (dt, qdt, mask), i8s, (comp, rows), N in itertools.product(CLASSES, (0, 1), ((0, ALL_ROWS), (1, ALL_ROWS), (1, 0x5550), (1, 0)), SIZES):
        for n_b in sorted({N, 1}):
            yield dt, qdt, mask, i8s, comp, rows, N, n_b


def test_every_plan_is_the_table(P):
    n = 0
    for q in queries():
        got, want = P.plan(*q), expected(*q)
        for r in range(15):
            assert got[r] == want[r], (q, r)
        n += 1
    assert n == 34 * 2 * 4 * (2 * 5 + 1)


def test_the_table_says_what_the_issue_says(P):
    """the table above, spot-checked against plain statements (so that a mistake shared by expected() and plan_trunk still shows)"""
    p = lambda qdt, mask, N=42, n_b=42, i8s=0, comp=1: P.plan(F16, qdt, mask, i8s, comp, ALL_ROWS, N, n_b)
    f = p(I8, 15)
    assert [s["op_dt"] for s in f] == [F16, F16] + [I8] * 13
    assert [r for r in range(15) if f[r]["out16"] != NONE and f[r]["outq"] != NONE] == [1, 3, 5, 7, 10, 12]          # the dual epilogues
    assert [r for r in range(15) if f[r]["out16"] == NONE] == [2, 4, 6, 8, 9, 11, 13]                                # 8-bit only
    assert [f[r]["oinv"] for r in range(15)] == [NONE, 1, NONE, 3, NONE, 5, NONE, 7, NONE, 9, 10, NONE, 12, NONE, NONE]
    assert all(s["qcopy"] == NONE and s["res_q"] == 0 and s["rscale"] == NONE for s in f)
    assert [s["img_bias"] for s in f] == [0, 0] + [1] * 13 and not any(s["img_bias"] for s in p(FP8, 15))
    assert not any(s["img_bias"] for s in p(I8, 15, 15, 15)) and not any(s["img_bias"] for s in p(I8, 15, comp=0))
    assert [s["img_bias"] for s in p(I8, 15, 16, 1)] == [0, 0] + [1] * 13      # per CALL: 17 images in encodeA, 16 behind it
    assert f[14]["out16"] == TOKENS and f[14]["rec"] == TOKENS and f[14]["rec_dt"] == F16 and f[14]["res"] == X512 + 2
    # q8_copy behind a 2-byte producer, in its three places
    assert [r for m in (2, 4, 8) for r, s in enumerate(p(I8, m)) if s["qcopy"] != NONE] == [5, 9, 10]
    assert p(FP8, 2)[5]["qcopy"] == 5 and p(FP8, 4)[9]["qcopy"] == 9 and p(FP8, 8)[10]["qcopy"] == 10
    # masks 4 / 6 / 9: 8-bit -> f16 only, 8-bit alone with epilogue scales, both boundaries of a single stage
    assert (p(I8, 4)[10]["op_dt"], p(I8, 4)[10]["out16"], p(I8, 4)[10]["outq"]) == (I8, X512 + 0, NONE)
    assert (p(I8, 6)[9]["out16"], p(I8, 6)[9]["outq"], p(I8, 6)[9]["oinv"]) == (NONE, X256 + 0, 9)
    assert p(I8, 9)[5]["outq"] == NONE and p(I8, 9)[10]["qcopy"] == 10 and p(I8, 9)[1]["outq"] == X128 + 0
    # the shared crop: both copies of the concat are replicated, the 8-bit one only when an epilogue wrote it
    assert (p(I8, 15, 42, 1)[5]["bcast16"], p(I8, 15, 42, 1)[5]["bcastq"]) == (1, 1) and (p(I8, 2, 42, 1)[5]["bcast16"], p(I8, 2, 42, 1)[5]["bcastq"]) == (1, 0)
    assert p(I8, 15, 1, 1)[5]["bcast16"] == 0 and p(I8, 15, 42, 42)[5]["bcast16"] == 0
    # the 8-bit residual stream: 8-bit skip operands with the scales of the activation they hold, no f16 tensor but stem and tokens
    s = p(I8, 15, i8s=1)
    assert [r for r in range(15) if s[r]["out16"] != NONE] == [0, 14] and [s[r]["rscale"] for r in (3, 5, 7, 9, 12, 14)] == [1, 3, 5, 7, 10, 12]
    assert not any(x["img_bias"] or x["bcast16"] for x in p(I8, 15, 42, 1, i8s=1)) and p(I8, 15, 42, 1, i8s=1)[5]["bcastq"] == 1
    assert p(I8, 0, i8s=1) == s and p(FP8, 15, i8s=1) == p(FP8, 15)


def test_invariants_of_every_plan(P):
    for q in queries():
        plan = P.plan(*q)
        dt, qdt = q[0], q[1]
        w16, wq = {NN_IN: -1}, {}                # buffer -> the row that wrote it last (the network input: before the trunk)
        for r, s in enumerate(plan):
            i, o, res = ROWS[r]
            holder = lambda slot: max([-1] + [k for k in range(r) if ROWS[k][1] == slot])     # the row whose output the slot holds now
            assert (s["in"], s["res"]) == (i, res) and {s["out16"], s["outq"]} <= {o, NONE} and (s["out16"], s["outq"]) != (NONE, NONE), (q, r)
            # every operand was written earlier in this plan, in the copy that is read, and is not a stale tensor of the slot
            assert (wq if s["in_q"] else w16).get(i) == holder(i), (q, r)
            assert s["op_dt"] == (qdt if s["in_q"] else dt), (q, r)
            if res != NONE:
                assert (wq if s["res_q"] else w16).get(res) == holder(res), (q, r)     # (also: nobody overwrote a skip operand still to be read)
                assert s["rscale"] == (holder(res) if s["res_q"] else NONE), (q, r)
            else:
                assert s["res_q"] == 0 and s["rscale"] == NONE, (q, r)
            # an 8-bit tensor carries its OWN activation's scales: from the epilogue table, folded into a residual-free 8-bit layer, or from q8_copy
            assert s["oinv"] in ((r, NONE) if (res == NONE and s["in_q"] and s["out16"] == NONE) else (r,)) or s["outq"] == NONE, (q, r)
            assert s["oinv"] == NONE or s["outq"] != NONE, (q, r)
            assert s["qcopy"] in (NONE, r) and not (s["qcopy"] != NONE and (s["outq"] != NONE or s["out16"] == NONE)), (q, r)
            assert not s["img_bias"] or (s["in_q"] and qdt == I8), (q, r)
            assert (not s["bcast16"] or s["out16"] != NONE) and (not s["bcastq"] or s["outq"] != NONE), (q, r)
            if s["out16"] != NONE:
                w16[o] = r
            if s["outq"] != NONE or s["qcopy"] != NONE:
                wq[o] = r
            # a record reads a tensor this row wrote, with its element type and, if 8-bit, its own scales
            if s["rec"] != NONE:
                assert s["rec"] == o and (wq if s["rec_q"] else w16).get(o) == r, (q, r)
                assert (s["rec_dt"], s["rec_scale"]) == ((qdt, r) if s["rec_q"] else (dt, NONE)), (q, r)
            else:
                assert (s["rec_q"], s["rec_dt"], s["rec_scale"]) == (0, NONE, NONE), (q, r)
        assert w16.get(TOKENS) == 14, q


def test_mask_zero_is_the_f16_plan(P):
    """an 8-bit network with no stage in the mask runs the f16 trunk: field for field apart from the element types.  STATED EXCEPTION: the
    8-bit trunks with an f16 stream have never recorded encodeA.1's output (activation 1) during a calibration, the 2-byte trunk does;
    this plan keeps both as they were, so that calibration launches and records stay what they are."""
    for qdt in (FP8, I8):
        for comp, N in itertools.product((0, 1), SIZES):
            for n_b in sorted({N, 1}):
                want = P.plan(F16, -1, 0, 0, comp, ALL_ROWS, N, n_b)
                got = P.plan(F16, qdt, 0, 0, comp, ALL_ROWS, N, n_b)
                for r in range(15):
                    skip = DT_FIELDS + (("rec", "rec_dt") if r == 1 else ())
                    assert {k: v for k, v in got[r].items() if k not in skip} == {k: v for k, v in want[r].items() if k not in skip}, (qdt, N, n_b, r)
                    assert got[r]["op_dt"] == F16
                assert got[1]["rec"] == NONE and want[1]["rec"] == X128 + 0


def test_queries_outside_the_domain_are_refused(P):
    ok = (F16, I8, 15, 0, 1, ALL_ROWS, 42, 42)
    assert P.rc(*ok) == 0
    assert P.rc(F16, I8, 15, 0, 1, ALL_ROWS, 0, 0) == 1                     # no hypothesis
    assert P.rc(F16, I8, 15, 0, 1, ALL_ROWS, 42, 2) == 1                    # the observed crops are the hypotheses' own, or one
    assert P.rc(FP8, -1, 0, 0, 0, 0, 42, 42) == 1                           # the stem and the token path have no 8-bit form
    assert P.rc(F16, F16, 15, 0, 0, 0, 42, 42) == 1 and P.rc(F16, 4, 15, 0, 0, 0, 42, 42) == 1      # qdt is DT_FP8 or DT_I8
    assert P.rc(BF16, I8, 15, 0, 0, 0, 42, 42) == 1                         # the 8-bit layers sit in an f16 network
    assert P.rc(F16, I8, 15, 0, 1, ALL_ROWS, N_MAX, 1) == 0
