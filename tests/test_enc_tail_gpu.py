"""The tile kernels of the heads -- enc_tail_kernel, qkv_tile_kernel, enc_heads_kernel -- on caller-chosen operands against float64.

Cases, families, reference, comparators and bounds are tests/enc_tail_cases.py (tests/test_enc_tail_cases_cpu.py holds them to the library's
plan, re-measures the constants and shows that every comparator can fail).  Every case is ONE call of a raw hook of the test build
(fpt_enc_tail_raw, fpt_qkv_tile_raw, fpt_enc_heads_raw): raw element patterns in, the whole output buffer back, guard rows around every
device buffer, the product's launch code.

enc_tail_kernel leaves three floats per tile, so the hook launches it once per probe set: 171 sets of one-hot read-out rows return the 512
column sums of the rounded LayerNorm-2 output of every tile of both heads exactly; two further sets are dense read-out rows, held to the
dot product of those very sums within the f32 accumulation error (C_ACC sum |S w|).  The column
sums (family `live`: the single live row recovered from them) are held to the float64 chain of layer_ref.encoder_chain in units of
U = u (|g| rstd (|y2| + mean |y2|) + |z|): the hard bound K_ELEM, the statistical bound K_16 / K_80 on every family but `live`, the
signed mean K_MEAN on every case.  qkv_tile_kernel: the stage suite's bound (half an ulp + C_ACC sum |x w|, mean error within 0.05 ulp),
bit for bit where every sum is one exact product, infinities where the reference rounds to infinity.  enc_heads_kernel: one f32 ulp of
sum |parts| / tokens + |bias| against the float64 sum on shares that add up exactly, `parts` ulps on shares that do not; the fused pose equals the product's own pose update on the returned y bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import enc_tail_cases as EC
import layer_ref as LR
from foundationpose_cpp_amd import _lib

pytestmark = pytest.mark.gpu

CANARY32 = 0x7FC5A5C3          # a quiet NaN: slot 3 of every pdot tile must come back with these bits
CANARY16 = 0x7FFF              # a NaN in f16 and bf16 alike
TABLE = []                     # (kernel, instantiation, family, err / bound, what)


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    vp, ci = C.c_void_p, C.c_int
    L.fpt_enc_tail_raw.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    L.fpt_qkv_tile_raw.argtypes = [ci, ci, vp, vp, vp, vp, vp]
    L.fpt_enc_heads_raw.argtypes = [vp, vp, ci, ci, C.c_float, ci, C.c_float, vp, vp, vp, vp]
    for f in (L.fpt_enc_tail_raw, L.fpt_qkv_tile_raw, L.fpt_enc_heads_raw):
        f.restype = ci
    yield L
    worst = {}
    for kernel, inst, fam, ratio, what in TABLE:
        key = (kernel, inst, fam, what)
        worst[key] = max(worst.get(key, 0.0), ratio)
    print("\nkernel, instantiation, family: worst err / bound")
    for (kernel, inst, fam, what), ratio in sorted(worst.items()):
        print(f"  {kernel:16s} {inst:10s} {fam:10s} {what:16s} {ratio:.3f}")


def _f32(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_enc_tail_matches_the_float64_chain(tl, case):
    MI, dt, tiles, fam = case
    cid = EC.case_id(case)
    p = EC.make_problem(case)
    hw = EC.probes(case)
    P = hw.shape[0]
    att, x = EC.bits(p.att), EC.bits(p.x)
    W, b, g, be = _f32(p.W), _f32(p.b), _f32(p.g), _f32(p.be)
    pdot = np.full((P, 2, tiles, 4), CANARY32, np.uint32)
    info = np.full(4, -1, np.int32)
    rc = tl.fpt_enc_tail_raw(dt, MI, tiles, att.ctypes.data, x.ctypes.data, W.ctypes.data, b.ctypes.data, g.ctypes.data, be.ctypes.data,
                             hw.ctypes.data, P, pdot.ctypes.data, info.ctypes.data)
    assert rc == 0, (cid, rc, tl.fp_last_error())               # (2 / 3: a guard of pdot / an input buffer changed)
    assert tuple(info) == (MI, tiles, 2 * tiles, EC.LDS_TAIL[MI]), (cid, info)
    assert (pdot[..., 3] == CANARY32).all(), f"{cid}: slot 3 of a pdot tile was written"
    got = pdot[..., :3].copy().view(np.float32)
    assert np.isfinite(got).all(), f"{cid}: a tile's share is not finite (or was not written)"
    assert (got[EC.N_ONEHOT - 1, :, :, 2] == 0).all(), f"{cid}: the all-zero probe row of the last one-hot set"
    ref = EC.reference(p)
    S = EC.sums_from_pdot(got)
    c = EC.compare(p, ref, S)
    hard, stat, mean = EC.limits(p)
    inst = f"<{EC.DT_NAME[dt]}, {MI}>"
    TABLE.append(("enc_tail_kernel", inst, fam, c["worst"] / hard, "hard"))
    if stat is not None:
        TABLE.append(("enc_tail_kernel", inst, fam, c["worst"] / stat, "statistical"))
    TABLE.append(("enc_tail_kernel", inst, fam, abs(c["mean"]) / mean, "signed mean"))
    want, bound = EC.dense_reference(S, hw[EC.N_ONEHOT:])        # (the read-out path against the one-hot sums of this very call)
    dense = float((torch.from_numpy(got[EC.N_ONEHOT:].astype(np.float64)) - want).abs().div(bound).max())
    TABLE.append(("enc_tail_kernel", inst, fam, dense, "dense probes"))
    codes = float((S != ref["S"]).double().mean())
    print(f"{cid}: worst |dS| / sum U {c['worst']:.4f} (hard {hard}, statistical {stat}), signed mean {c['mean']:+.2e} over {c['n']} "
          f"(bound {mean}), dense probes {dense:.4f} of their bound, {100 * codes:.1f} % of the sums differ")
    assert EC.verdict(p, c) == [], f"{cid}: {EC.verdict(p, c)} -- worst {c['worst']:.4f}, signed mean {c['mean']:+.3e}"
    assert dense <= 1.0, f"{cid}: dense probes at {dense:.3f} of their bound"


@pytest.mark.parametrize("case", EC.QKV_CASES, ids=EC.qkv_case_id)
def test_qkv_tile_matches_float64(tl, case):
    dt, tiles, fam = case
    cid = EC.qkv_case_id(case)
    x, W, b, exact = EC.make_qkv_problem(case)
    rows = tiles * EC.QKV_TOKENS
    xb, Wf, bf = EC.bits(x), _f32(W), _f32(b)
    out = np.full((rows, 3 * EC.EMBED), CANARY16, np.uint16)
    info = np.full(3, -1, np.int32)
    rc = tl.fpt_qkv_tile_raw(dt, tiles, xb.ctypes.data, Wf.ctypes.data, bf.ctypes.data, out.ctypes.data, info.ctypes.data)
    assert rc == 0, (cid, rc, tl.fp_last_error())
    assert tuple(info) == (tiles, tiles, EC.LDS_QKV), (cid, info)
    got = EC.from_bits(out, dt)
    assert not bool(torch.isnan(got.float()).any()), f"{cid}: an output element was not written"
    ref, acc = EC.qkv_reference(x, W, b)
    inst = f"<{EC.DT_NAME[dt]}>"
    if exact:
        want = ref.to(EC.TORCH_DT[dt])
        same = torch.equal(got.view(torch.int16), want.view(torch.int16))
        TABLE.append(("qkv_tile_kernel", inst, fam, 0.0 if same else float("inf"), "bit for bit"))
        if fam == "top":
            assert bool(torch.isinf(want.float()).any())
        assert same, f"{cid}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ from the rounded reference"
        return
    worst, bias = LR.stage_error(got.double(), ref, acc, dt)
    TABLE.append(("qkv_tile_kernel", inst, fam, worst, "stage bound"))
    TABLE.append(("qkv_tile_kernel", inst, fam, abs(bias) / LR.BIAS_ULP, "mean error"))
    print(f"{cid}: err / bound {worst:.3f}, mean error {bias:+.4f} ulp")
    assert worst <= 1.0, f"{cid}: err / bound = {worst:.3f}"
    assert abs(bias) <= LR.BIAS_ULP, f"{cid}: mean error {bias:.4f} ulp"


@pytest.mark.parametrize("case", EC.HEADS_CASES, ids=EC.heads_case_id)
def test_enc_heads_adds_the_tiles_up(tl, case):
    n, parts, fam, fused = case
    cid = EC.heads_case_id(case)
    pd, bias = EC.make_heads_problem(case)
    pd, bias = np.ascontiguousarray(pd), np.ascontiguousarray(bias)
    rng = np.random.default_rng(n * 100 + parts)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3], pose[:3, 3] = q, (0.1, -0.2, 0.8)
    pose_in = np.ascontiguousarray(pose.T).reshape(16)                 # column-major, as the library keeps poses
    pose_io, pose_ref = pose_in.copy(), np.zeros(16, np.float32)
    flag = np.array([0xABCD0000], np.uint32)
    y = np.full((2, n, 3), np.nan, np.float32)
    rc = tl.fpt_enc_heads_raw(pd.ctypes.data, bias.ctypes.data, n, parts, EC.SEQ_TOKENS, fused, 0.3, pose_io.ctypes.data, flag.ctypes.data,
                              pose_ref.ctypes.data, y.ctypes.data)
    assert rc == 0, (cid, rc, tl.fp_last_error())
    want, bound, y32 = EC.heads_reference(pd, bias, n, parts, fam.startswith("rough"))
    ratio = float((np.abs(y.astype(np.float64) - want) / bound).max())
    seq = bool((y.view(np.uint32) == y32.view(np.uint32)).all())
    TABLE.append(("enc_heads_kernel", f"parts {parts}", fam, ratio, "`parts` f32 ulps" if fam.startswith("rough") else "one f32 ulp"))
    print(f"{cid}: err / bound {ratio:.3f}; the sequential float32 emulation is {'matched bit for bit' if seq else 'NOT matched bit for bit'}")
    assert ratio <= 1.0, f"{cid}: err / bound = {ratio:.3f}"
    if fused:
        assert flag[0] == 1, f"{cid}: the completion flag was not raised"
        assert not np.array_equal(pose_io, pose_in)
        assert np.array_equal(pose_io.view(np.uint32), pose_ref.view(np.uint32)), f"{cid}: the fused pose is not the pose update of the returned y"
    else:
        assert flag[0] == 0xABCD0000 and np.array_equal(pose_io.view(np.uint32), pose_in.view(np.uint32)), f"{cid}: the unfused call touched pose or flag"
