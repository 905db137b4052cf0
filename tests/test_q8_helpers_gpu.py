"""The helper kernels of the 8-bit trunks on raw buffers, through the launch code the product uses (fpt_q8_copy_raw, fpt_q8_img_bias_raw,
fpt_chan_stats_raw): q8_copy_kernel bit for bit against numpy float32, q8_img_bias_fused_kernel (lattice and every-pixel form, and the
test build's three-launch form) and chan_stats_kernel against float64 within the f32 accumulation they make.  Every output buffer is
pre-filled with a canary; what a kernel does not own must come back as it went."""
import ctypes as C

import numpy as np
import pytest
import torch

import q8_conv_cases as Q
from foundationpose_cpp_amd import _lib

pytestmark = pytest.mark.gpu
F16, BF16, FP8, I8 = 0, 1, 2, 3
U24 = 2.0 ** -24


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _lib_err(L):
    return (L.fp_last_error() or b"").decode()


# ---- q8_copy_kernel ----
@pytest.mark.parametrize("qdt", [FP8, I8], ids=["fp8", "int8"])
@pytest.mark.parametrize("imgs,HW,Cc", [(3, 40, 128), (2, 40, 256), (5, 20, 512)])
def test_q8_copy_is_bit_exact(imgs, HW, Cc, qdt):
    """f16 -> f32 is exact, then one f32 multiply and one rounding (RNE, saturating): numpy float32 reproduces it.  The inputs land on .5
    codes, go above 255 / 448 and below 0; the border and the guard image keep their canary."""
    rng = np.random.default_rng(imgs * 1000 + Cc + qdt)
    x = (rng.standard_normal((imgs, HW + 2, HW + 2, Cc)) * 40).astype(np.float16)
    oinv = rng.uniform(0.5, 8.0, Cc).astype(np.float32)
    oinv[::4] = 4.0                                               # value * 4 with values on the f16 grid: .5 codes by the thousand
    x[..., ::4] = (np.rint(x[..., ::4].astype(np.float32) * 8) / 8).astype(np.float16)
    x[:, 3, 3, :] = 300.0                                         # above both ranges after scaling (and in channels scaled by < 1 still in range)
    x[:, 4, 4, :] = 60000.0
    x[x == 0] = np.float16(0.25)                                  # (no signed zeros: the two e4m3 zeros are not told apart here)
    x[:, 0, :, :] = np.nan                                        # the f16 border is never read
    x[:, -1, :, :] = np.nan
    x[:, :, 0, :] = np.nan
    x[:, :, -1, :] = np.nan
    q = Q.canary8((imgs + 1) * (HW + 2) * (HW + 2) * Cc).reshape(imgs + 1, HW + 2, HW + 2, Cc).copy()
    pat = q.copy()
    info = np.zeros(2, np.int32)
    L = _lib.test_lib()
    L.fpt_q8_copy_raw.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]
    assert L.fpt_q8_copy_raw(_p(np.ascontiguousarray(x.view(np.uint16))), _p(oinv), imgs, HW, Cc, qdt, 1, _p(q), _p(info)) == 0, _lib_err(L)
    assert info[0] * info[1] >= imgs * HW * HW * Cc // 8 > (info[0] - 1) * info[1]                  # one thread per 8 channels of a pixel
    t = x[:, 1:-1, 1:-1, :].astype(np.float32) * oinv                                                # one f32 rounding
    if qdt == I8:
        want = np.clip(np.rint(t), 0, 255).astype(np.uint8) ^ np.uint8(0x80)
        assert (np.abs(t - np.floor(t) - 0.5) == 0).sum() > 1000 and (t > 255).sum() > 100 and (t < 0).sum() > 1000
    else:
        want = Q.e4m3_bits(Q.q_e4m3(torch.from_numpy(t.astype(np.float64))).numpy())
        assert (t > 448).sum() > 100 and (t < -448).sum() > 0 and (t < 0).sum() > 1000
    got = q[:imgs, 1:-1, 1:-1, :]
    bad = got != want
    assert not bad.any(), (int(bad.sum()), t[bad][:5], got[bad][:5], want[bad][:5])
    q[:imgs, 1:-1, 1:-1, :] = pat[:imgs, 1:-1, 1:-1, :]
    assert np.array_equal(q, pat), "the kernel wrote outside the interiors"


# ---- q8_img_bias_fused_kernel ----
def _img_bias(L, xq, tm, cs, bias, n_img, HW, Cin, Cout, form):
    out = np.full((n_img + 2, Cout), 0xFFC0A5A5, np.uint32)
    info = np.zeros(2, np.int32)
    L.fpt_q8_img_bias_raw.argtypes = [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    assert L.fpt_q8_img_bias_raw(_p(xq), _p(tm), _p(cs), _p(bias), n_img, HW, Cin, Cout, form, 2, _p(out), _p(info)) == 0, _lib_err(L)
    assert np.all(out[n_img:] == 0xFFC0A5A5), "rows of images >= n_img were written"
    return out[:n_img].view(np.float32), info


@pytest.mark.parametrize("Cin,Cout,HW", [(128, 128, 40), (256, 256, 40), (256, 512, 40), (512, 512, 20)])
def test_q8_img_bias_fused(Cin, Cout, HW):
    """bias - cscale * inv_px * sum_c Tt[c][co] * sum[c] in float64 from the same bytes; the integer channel sums are exact, so what is left
    is the f32 accumulation of the dot product, Cin * 2^-24 * cscale * inv_px * sum |t m|, and one rounding of the result.  1, 4, 5 and 19
    images: one short group, one full one, a last group of one, several groups with a last one of three."""
    L = _lib.test_lib()
    rng = np.random.default_rng(Cin + Cout + HW)
    tm = (0.4 * rng.standard_normal((Cin, Cout))).astype(np.float32)
    cs = rng.uniform(2e-5, 2e-4, Cout).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    for n_img in (1, 4, 5, 19):
        u = np.zeros((n_img, HW + 2, HW + 2, Cin), np.uint8)
        u[:, 1:-1, 1:-1, :] = np.clip(np.maximum(rng.standard_normal((n_img, HW, HW, Cin), dtype=np.float32), 0) * rng.uniform(10, 90, Cin).astype(np.float32), 0, 255)
        u[n_img // 2, 1:-1, 1:-1, 5] = 255                                     # a channel at the top of its range: the largest integer sum
        xq = u ^ np.uint8(0x80)
        t64, c64, b64 = tm.astype(np.float64), cs.astype(np.float64), bias.astype(np.float64)
        results = {}
        for form, name in ((0, "lattice"), (1, "every pixel"), (2, "three launches")):
            got, info = _img_bias(L, xq, tm, cs, bias, n_img, HW, Cin, Cout, form)
            pts = u[:, ::2, ::2, :] if form == 0 else u                         # even rows x even columns of the padded image: exactly the lattice
            inv_px = np.float64(np.float32(1.0) / np.float32((HW // 2) ** 2 if form == 0 else HW * HW))
            m = pts.reshape(n_img, -1, Cin).sum(1, dtype=np.int64).astype(np.float64)                # exact
            ref = b64 - c64 * inv_px * (m @ t64)
            bound = Cin * U24 * c64 * inv_px * (np.abs(m) @ np.abs(t64)) + U24 * np.abs(ref) + 2 * U24 * np.abs(c64 * inv_px * (m @ t64))
            err = np.abs(got.astype(np.float64) - ref)
            print(f"Cin {Cin} Cout {Cout} HW {HW} images {n_img:>2} {name:<14}: worst err / bound {float((err / bound).max()):.3f}, grid {info[0]}")
            assert np.all(err <= bound), (name, n_img, float((err / bound).max()))
            if form < 2:
                assert info[0] == -(-n_img // 4) and info[1] == 1024
            results[form] = got
        # the every-pixel form and the three-launch form compute the same quantity in another summation order
        assert np.abs(results[1].astype(np.float64) - results[2]).max() <= 2 * bound.max()


# ---- chan_stats_kernel ----
def _decode(raw, dt, scale):
    """the f32 values the kernel sees"""
    if dt == F16:
        return raw.view(np.float16).astype(np.float32)
    if dt == BF16:
        return (raw.astype(np.uint32) << 16).view(np.float32)
    v = (raw ^ np.uint8(0x80)).astype(np.float32) if dt == I8 else Q.E4M3[raw].astype(np.float32)
    return v * scale if scale is not None else v


@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("dt", [F16, BF16, FP8, I8], ids=["f16", "bf16", "fp8", "int8"])
def test_chan_stats(dt, with_scale):
    """per-channel |max| exactly, the sum within each thread's f32 accumulation plus 2^-21 per thread for the 2^-20 fixed-point conversion;
    the trunk's tensors: [3, 42, 42, 128], [2, 22, 22, 512] with their zero borders and a [5 * 400, 512] token tensor"""
    L = _lib.test_lib()
    L.fpt_chan_stats_raw.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 4
    rng = np.random.default_rng(dt * 2 + with_scale)
    for imgs, HP, Cc, border in ((3, 42, 128, 1), (2, 22, 512, 1), (5, 20, 512, 0)):
        x = rng.standard_normal((imgs, HP, HP, Cc)).astype(np.float32) * rng.uniform(0.5, 4, Cc).astype(np.float32)
        if dt in (FP8, I8):
            x = np.maximum(x, 0) if dt == I8 else x
        mask = np.zeros((imgs, HP, HP, 1), bool)
        mask[:, border:HP - border, border:HP - border] = True
        x = np.where(mask, x, 0)
        scale = rng.uniform(0.01, 0.1, Cc).astype(np.float32) if with_scale else None
        if dt == F16:
            raw = x.astype(np.float16).view(np.uint16)
        elif dt == BF16:
            raw = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        elif dt == I8:
            raw = np.clip(np.rint(x * 20), 0, 255).astype(np.uint8) ^ np.uint8(0x80)
        else:
            raw = Q.e4m3_bits(Q.q_e4m3(torch.from_numpy((x * 20).astype(np.float64))).numpy())
        raw = np.ascontiguousarray(raw.reshape(-1, Cc))
        f = _decode(raw, dt, scale if dt in (FP8, I8) else None)               # [pixels, C] f32, as the kernel computes them
        amax = np.zeros(Cc, np.float32)
        s0 = 12345
        ssum = np.full(Cc, s0, np.int64)
        info = np.zeros(2, np.int32)
        assert L.fpt_chan_stats_raw(_p(raw), raw.shape[0], Cc, dt, _p(scale), _p(amax), _p(ssum), _p(info)) == 0, _lib_err(L)
        threads = info[0] * info[1] // (Cc // 8)                                # threads that walk every channel
        assert threads == 1024
        want_max = np.abs(f.astype(np.float64)).max(0)
        assert np.array_equal(amax.astype(np.float64), want_max), (dt, Cc)
        per_thread = -(-raw.shape[0] // threads)                                # pixels a thread adds up
        ref = f.astype(np.float64).sum(0)
        bound = per_thread * U24 * np.abs(f.astype(np.float64)).sum(0) + threads * 2.0 ** -21
        err = np.abs((ssum - s0) / 2.0 ** 20 - ref)
        print(f"dt {dt} scale {with_scale} [{raw.shape[0]}, {Cc}]: sum worst err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), float((err / bound).max())
