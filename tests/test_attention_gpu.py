"""Both attention kernels against the float64 reference of tests/layer_ref.py (LR.sdpa) over every class of shapes they serve.

The cases, the class definition and the input families are tests/attention_cases.py (tests/test_attention_cases_cpu.py holds them to the
library's plan and shows that the bound below can fail).  Every draw of a case is ONE launch through the test build's fpt_attention_raw -- raw
element patterns in and out, guard rows around both device buffers, the kernel planned (the product's path) or forced.

Bound: the stage suite's own (layer_ref.stage_error), per element |got - ref| <= 0.5 ulp(|ref| + acc) + acc against the UNROUNDED float64
value, and a mean signed error within 0.05 ulp where the output has at least 16384 elements (below that the mean of half-ulp rounding
errors is itself noisy at the 0.01 ulp level; an output of fewer than 262144 elements pools the mean over several draws of its
family, attention_cases.n_draws, every draw held to everything else).  Further: `onehot` returns v[perm] bit for bit; no NaN in a
row < T although every input row >= T inside a pitch holds quiet NaNs; the output rows >= T inside a pitch keep their canary; the hook
finds its guard rows intact; the kernel that ran is the one the case expects.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cases as AC
import layer_ref as LR
from foundationpose_cpp_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0x7FFF            # a NaN in f16 and bf16 alike: an output row < T the kernel skipped fails the NaN check, too
TABLE = []


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_attention_raw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.fpt_attention_raw.restype = C.c_int
    yield L
    worst = {}
    for kernel, dt, ratio, bias, cid in TABLE:
        key = (("attention32_kernel", "attention32_skv_kernel")[kernel], "bf16" if dt else "f16")
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, cid)
    for (k, d), (ratio, cid) in sorted(worst.items()):
        print(f"\n{k} {d}: worst err / bound {ratio:.3f} ({cid})", end="")
    biased = [t for t in TABLE if t[3] is not None]
    if biased:
        t = max(biased, key=lambda t: abs(t[3]))
        print(f"\nlargest |mean error| {abs(t[3]):.4f} ulp ({t[4]})")


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _launch(tl, case, draw):
    """one launch of the case on one draw of its family, every assertion but the pooled one -> (err / bound, mean error in ulps)"""
    B, T, pitch, dt, kernel, fam = case
    cid = AC.case_id(case) + f" draw {draw}"
    x, perm = AC.make_inputs(B, T, dt, fam, draw)
    qkv = np.full((B, pitch, 1536), AC.QNAN[dt], np.uint16)
    qkv[:, :T] = _bits(x)
    out = np.full((B, pitch, AC.EMBED), CANARY, np.uint16)
    info = np.full(3, -1, np.int32)
    rc = tl.fpt_attention_raw(qkv.ctypes.data, B, T, pitch, dt, kernel, out.ctypes.data, info.ctypes.data)
    assert rc == 0, (cid, rc, tl.fp_last_error())        # (2 / 3: a guard row of the output / input buffer changed)
    want = AC.expected_kernel(case)
    assert tuple(info) == (want,) + AC.launch_shape(want, B, T), (cid, info)
    assert (out[:, T:] == CANARY).all(), f"{cid}: an output row >= T inside the pitch was written"
    got_e = torch.from_numpy(out[:, :T].view(np.int16).copy()).view(AC.TORCH_DT[dt])
    assert not bool(torch.isnan(got_e.float()).any()), f"{cid}: NaN in an output row < T"
    ref, acc = LR.sdpa(x.to(DEV), dt, round_out=False, q_per=1024)
    worst, bias = LR.stage_error(got_e.to(DEV).double(), ref, acc, dt)
    assert worst <= 1.0, f"{cid}: err / bound = {worst:.3f}"
    if fam == "onehot":
        assert torch.equal(got_e, torch.take_along_dim(x[..., 2 * AC.EMBED:], perm[:, :, None], 1)), f"{cid}: not v[perm] bit for bit"
    return worst, bias


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_attention_matches_float64(tl, case):
    B, T, _, dt, _, _ = case
    cid = AC.case_id(case)
    runs = [_launch(tl, case, d) for d in range(AC.n_draws(B, T))]    # (several draws below BIAS_POOL_ELEMS elements: attention_cases.py)
    worst, bias = max(r[0] for r in runs), sum(r[1] for r in runs) / len(runs)
    check_bias = B * T * AC.EMBED >= AC.BIAS_MIN_ELEMS
    TABLE.append((AC.expected_kernel(case), dt, worst, bias if check_bias else None, cid))
    print(f"{cid}: err / bound {worst:.3f}, mean error {bias:+.4f} ulp over {len(runs)} draw(s){'' if check_bias else ' (not asserted)'}")
    if check_bias:
        assert abs(bias) <= LR.BIAS_ULP, f"{cid}: mean error {bias:.4f} ulp"
