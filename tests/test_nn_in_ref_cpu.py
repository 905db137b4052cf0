"""The host reference of nn_in (tests/nn_in_ref.py): its layout IS the address formula of fp_geometry.hip, unpack inverts pack, and the
two comparators of tests/test_nn_input_gpu.py reject every way the device's store is likely to go wrong."""
import numpy as np
import pytest
import torch

import nn_in_ref as R


@pytest.fixture(scope="module")
def blobs():
    """three images of full-mantissa content in the range of the real tensors (colours in [0, 1], coordinates in [-2, 2], 20 % exact zeros
    like the background); no two rows or columns alike"""
    rng = np.random.default_rng(17)
    x = np.concatenate([rng.uniform(0, 1, (3, 160, 160, 3)), rng.uniform(-2, 2, (3, 160, 160, 3))], -1).astype(np.float32)
    x[rng.uniform(size=x.shape[:3]) < 0.2] = 0.0
    return x


def test_layout_is_the_address_formula_of_the_kernels(blobs):
    """in 16-byte units (8 elements) pixel (n, y, x) sits at ((n*84 + y/2 + 2)*84 + x/2 + 2)*4 + (y&1)*2 + (x&1): plain integer arithmetic
    over every pixel of two images; everything the formula does not address (pad channels, border) is zero"""
    a, b = blobs[:1], blobs[1:2]
    flat = R.nn_in_from_blobs(a, b).numpy().reshape(-1)
    assert flat.size == 2 * 84 * 84 * 32
    n, y, x = np.meshgrid(np.arange(2), np.arange(160), np.arange(160), indexing="ij")
    unit = ((n * 84 + y // 2 + 2) * 84 + x // 2 + 2) * 4 + (y & 1) * 2 + (x & 1)
    assert len(np.unique(unit)) == unit.size
    src = np.concatenate([a, b])
    seen = np.zeros(flat.size, bool)
    for c in range(6):
        assert np.array_equal(flat[unit * 8 + c], src[..., c].astype(np.float64)), c
        seen[(unit * 8 + c).reshape(-1)] = True
    assert not flat[~seen].any()
    for dt in (R.F16, R.BF16):      # the typed packer stores the same elements, rounded
        p = R.pack(src, dt).reshape(-1)
        for c in range(6):
            assert torch.equal(p[torch.from_numpy(unit * 8 + c)], R.rne(torch.from_numpy(src[..., c]), dt)), (dt, c)
        assert not p[torch.from_numpy(~seen)].to(torch.float64).abs().sum()


@pytest.mark.parametrize("dt", [R.F16, R.BF16])
def test_pack_unpack_round_trip(blobs, dt):
    t = R.pack(blobs, dt)
    assert t.shape == (3, 84, 84, 32) and t.dtype == R.TORCH_DT[dt]
    x, pad, ring = R.blobs_from_nn_in(t)
    assert torch.equal(x, R.rne(torch.from_numpy(blobs), dt))
    assert x.shape == (3, 160, 160, 6) and pad.shape == (3, 160, 160, 2) and ring.numel() == 3 * (84 * 84 - 80 * 80) * 32
    assert not pad.to(torch.float64).abs().sum() and not ring.to(torch.float64).abs().sum()
    # unpack -> pack of the float64 form too
    x64, _, _ = R.blobs_from_nn_in(R.nn_in_from_blobs(blobs[:2], blobs[2:]))
    assert np.array_equal(x64.numpy(), blobs.astype(np.float64))


def test_window_ends():
    """the window is the rounded image of the f32 values within TOL of the oracle, ends included"""
    ref = np.array([0.0, 1.0, 0.5 + 2.0 ** -12, -0.25, 3e-6], np.float32)      # 0.5 + 2^-12: a tie between two f16 values, TOL to either side decides
    lo, hi = R.window(ref, R.F16)
    sub = 2.0 ** -24                                                           # spacing of the f16 subnormals
    assert lo.tolist() == [-34 * sub, 1.0, 0.5, -0.25, 17 * sub]               # 2e-6 = 33.55 sub, 1e-6 = 16.78 sub
    assert hi.tolist() == [34 * sub, 1.0, 0.5 + 2.0 ** -11, -0.25, 84 * sub]   # 5e-6 = 83.89 sub
    # an f32 just outside the real interval is not part of it
    r = np.array([1.0], np.float32)
    lo, hi = R.window(r, R.BF16, tol=2.0 ** -24)      # 1 - 2^-24 is an f32 (inside); 1 + 2^-24 is not, and 1 + 2^-23 lies outside
    assert lo.tolist() == [1.0] and hi.tolist() == [1.0]


def _truncate(x, dt):
    """f32 -> element type by dropping the low bits (round toward zero)"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    r = R.rne(x, dt)
    over = r.to(torch.float32).abs() > x.abs()
    return (r.view(torch.int16) - over.to(torch.int16)).view(R.TORCH_DT[dt])     # sign-magnitude: one step towards zero


def _swap_x(t):
    return t.reshape(t.shape[:3] + (4, 8))[..., [1, 0, 3, 2], :].reshape(t.shape).contiguous()


def _mutations(blobs, dt):
    """name -> a tensor that is wrong in one way the device's store could be"""
    good = R.pack(blobs, dt)
    x8 = torch.zeros(blobs.shape[:3] + (8,), dtype=R.TORCH_DT[dt])
    x8[..., :6] = _truncate(blobs, dt)
    trunc = torch.zeros_like(good)
    trunc[:, 2:-2, 2:-2] = x8.reshape(-1, 80, 2, 80, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(-1, 80, 80, 32)
    shifted = blobs.copy()
    shifted[1, 80] = np.roll(blobs[1, 80], 1, axis=0)
    pad, border = good.clone(), good.clone()
    pad[2, 40, 41, 8 + 7] = 2.0 ** -14
    border[0, 83, 5, 3] = -2.0 ** -14
    return {"truncation instead of round-to-nearest-even": trunc, "row 80 of one image shifted by one pixel": R.pack(shifted, dt),
            "the two x&1 sub-positions swapped": _swap_x(good), "vertical flip omitted": R.pack(blobs[:, ::-1], dt),
            "non-zero pad channel": pad, "non-zero border element": border}


@pytest.mark.parametrize("dt", [R.F16, R.BF16])
@pytest.mark.parametrize("check", [R.check_oracle, R.check_bits])
def test_comparators_have_teeth(blobs, dt, check):
    good = R.pack(blobs, dt)
    assert check("good", good, blobs, dt) == []
    muts = _mutations(blobs, dt)
    assert len(muts) == 6
    for name, t in muts.items():
        assert not torch.equal(t.view(torch.int16), good.view(torch.int16)), name
        msgs = check(name, t, blobs, dt)
        assert msgs and all(m.startswith(name) for m in msgs), (name, msgs)
    # one element one step of the element type off, and nothing else, is enough
    one = good.clone().view(torch.int16)
    one[1, 30, 31, 17] += 1
    assert check("one step", one.view(good.dtype), blobs, dt)


@pytest.mark.parametrize("dt", [R.F16, R.BF16])
def test_oracle_window_admits_what_the_f32_bar_admits_and_signed_zeros(blobs, dt):
    """a tensor whose f32 source is within TOL of the oracle passes; -0 for 0 passes; a NaN does not"""
    rng = np.random.default_rng(1)
    near = (blobs.astype(np.float64) + rng.uniform(-1.9e-6, 1.9e-6, blobs.shape)).astype(np.float32)
    assert np.abs(near.astype(np.float64) - blobs).max() <= R.TOL
    assert R.check_oracle("near", R.pack(near, dt), blobs, dt) == []
    neg = R.pack(blobs, dt)
    neg[neg == 0] = -0.0
    assert bool((neg.view(torch.int16) == -32768).any())
    assert R.check_oracle("-0", neg, blobs, dt) == []
    nan = R.pack(blobs, dt)
    nan[0, 10, 10, 0] = float("nan")
    assert R.check_oracle("nan", nan, blobs, dt)
