"""Host reference of the networks' input tensor nn_in and the two comparators tests/test_nn_input_gpu.py holds it to.

Layout (fp_geometry.hip, s2d_index / pack6): [NB, 84, 84, 32] in a 2-byte type = space-to-depth 2x2 of NHWC [NB, 160, 160, 8] (six
channels r, g, b, x, y, z + two zero pad channels) with a zero border of 2 space-to-depth pixels.  In 16-byte units (8 elements) pixel
(n, y, x) sits at ((n*84 + y/2 + 2)*84 + x/2 + 2)*4 + (y&1)*2 + (x&1).  The first N images are the renders, the rest the observed crops.

Comparators (each returns a list of messages, empty = pass; NO element is exempted):
  check_oracle   every stored value lies in [rne(ref - TOL), rne(ref + TOL)], TOL = 2e-6 = the bar of the f32 tensors (F32_TOL of
                 tests/test_geometry_gpu.py); rne = torch's float32 -> float16 / bfloat16 conversion on the CPU.  Rounding is monotone, so a
                 device f32 value within TOL of the oracle rounds into that window.  The window's ends are taken from the f32 values inside
                 [ref - TOL, ref + TOL] (the device value is an f32), so it is never wider than the real interval's.  Values are compared,
                 so -0 == +0; a NaN is outside every window.  Pad channels 6-7 and the whole border are exactly zero.
  check_bits     the f32 blobs of the device's own f32 path, packed with rne, equal the tensor bit for bit (pad and border included)."""
import numpy as np
import torch

F16, BF16 = 0, 1                       # (layer_ref.F16 / BF16)
TORCH_DT = {F16: torch.float16, BF16: torch.bfloat16}
CROP, BORDER = 160, 2
P = CROP // 2 + 2 * BORDER             # 84
TOL = 2e-6


def nn_in_from_blobs(a, b):
    """the device's network input: [2N, 84, 84, 32] = space-to-depth 2x2 of [2N, 160, 160, 8] (6 channels + 2 zero) with a border of 2"""
    x = np.concatenate([a, b], 0)
    x8 = np.zeros(x.shape[:3] + (8,), np.float64)
    x8[..., :6] = x
    s2d = x8.reshape(-1, 80, 2, 80, 2, 8).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 80, 80, 32)
    return torch.from_numpy(np.pad(s2d, ((0, 0), (2, 2), (2, 2), (0, 0))))


def blobs_from_nn_in(t):
    """the inverse: [NB, 84, 84, 32] (torch tensor of any float type, or an array) -> (blobs [NB, 160, 160, 6], the two pad channels
    [NB, 160, 160, 2], every border element as one flat tensor); values unchanged, element type kept"""
    t = torch.as_tensor(t)
    assert t.shape[1:] == (P, P, 32), t.shape
    inner = t[:, BORDER:-BORDER, BORDER:-BORDER]
    x8 = inner.reshape(-1, 80, 80, 2, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(-1, CROP, CROP, 8)
    ring = torch.cat([t[:, :BORDER].flatten(), t[:, -BORDER:].flatten(), t[:, BORDER:-BORDER, :BORDER].flatten(),
                      t[:, BORDER:-BORDER, -BORDER:].flatten()])
    return x8[..., :6], x8[..., 6:], ring


def rne(x, dt):
    """float32 -> element type, round to nearest even (torch's CPU conversion)"""
    x = torch.as_tensor(x)
    assert x.dtype == torch.float32 and x.device.type == "cpu"
    return x.to(TORCH_DT[dt])


def pack(blobs, dt):
    """f32 blobs [NB, 160, 160, 6] -> nn_in [NB, 84, 84, 32] in the element type, as pack6 + s2d_index store it"""
    x = rne(torch.as_tensor(np.ascontiguousarray(blobs, np.float32)), dt)
    out = torch.zeros((x.shape[0], P, P, 32), dtype=x.dtype)
    x8 = torch.zeros(x.shape[:3] + (8,), dtype=x.dtype)
    x8[..., :6] = x
    out[:, BORDER:-BORDER, BORDER:-BORDER] = x8.reshape(-1, 80, 2, 80, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(-1, 80, 80, 32)
    return out


def window(ref, dt, tol=TOL):
    """(lo, hi) in float64: the element-type values of the smallest / largest f32 inside [ref - tol, ref + tol]"""
    r = torch.as_tensor(np.ascontiguousarray(ref, np.float32)).to(torch.float64)
    inf = torch.tensor(float("inf"), dtype=torch.float32)
    lo = (r - tol).to(torch.float32)
    lo = torch.where(lo.to(torch.float64) < r - tol, torch.nextafter(lo, inf), lo)
    hi = (r + tol).to(torch.float32)
    hi = torch.where(hi.to(torch.float64) > r + tol, torch.nextafter(hi, -inf), hi)
    return rne(lo, dt).to(torch.float64), rne(hi, dt).to(torch.float64)


def _where(idx, shape):
    return tuple(int(v) for v in np.unravel_index(int(idx), shape))


def _zero_parts(case, pad, ring):
    msgs = []
    bad = pad.to(torch.float64) != 0          # (-0 == +0; NaN != 0)
    if bool(bad.any()):
        n, y, x, c = _where(torch.nonzero(bad.flatten())[0], bad.shape)
        msgs.append(f"{case}: {int(bad.sum())} non-zero pad elements, first at image {n} row {y} column {x} channel {6 + c}")
    bad = ring.to(torch.float64) != 0
    if bool(bad.any()):
        msgs.append(f"{case}: {int(bad.sum())} non-zero border elements")
    return msgs


def check_oracle(case, got, ref_blobs, dt, chunk=32):
    """got: nn_in [NB, 84, 84, 32] in the element type (CPU); ref_blobs: the oracle's f32 [NB, 160, 160, 6]"""
    got = torch.as_tensor(got)
    assert got.dtype == TORCH_DT[dt] and got.shape[0] == len(ref_blobs), (got.dtype, got.shape, len(ref_blobs))
    blobs, pad, ring = blobs_from_nn_in(got)
    msgs = _zero_parts(case, pad, ring)
    nbad, first = 0, None
    for i in range(0, len(ref_blobs), chunk):
        g = blobs[i:i + chunk].to(torch.float64)
        lo, hi = window(ref_blobs[i:i + chunk], dt)
        bad = ~((g >= lo) & (g <= hi))
        k = int(bad.sum())
        if k and first is None:
            n, y, x, c = _where(torch.nonzero(bad.flatten())[0], bad.shape)
            first = (f"first at image {i + n} row {y} column {x} channel {c}: stored {float(g[n, y, x, c])!r}, oracle "
                     f"{float(ref_blobs[i + n][y, x, c])!r}, window [{float(lo[n, y, x, c])!r}, {float(hi[n, y, x, c])!r}]")
        nbad += k
    if nbad:
        msgs.append(f"{case}: {nbad} of {blobs.numel()} elements outside the oracle window; {first}")
    return msgs


def check_bits(case, got, dev_blobs, dt):
    """got as above; dev_blobs: the f32 blobs of the device's f32 path on the same poses"""
    got = torch.as_tensor(got)
    exp = pack(dev_blobs, dt)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, got.shape, exp.shape)
    bad = got.view(torch.int16) != exp.view(torch.int16)
    if not bool(bad.any()):
        return []
    n, sy, sx, e = _where(torch.nonzero(bad.flatten())[0], bad.shape)
    y, x, c = 2 * (sy - BORDER) + e // 16, 2 * (sx - BORDER) + (e // 8) % 2, e % 8
    per = bad.flatten(1).sum(1)
    imgs = [int(i) for i in torch.nonzero(per).flatten()[:8]]
    return [f"{case}: {int(bad.sum())} elements differ in bits from the packed f32 path (images {imgs}{' ...' if int((per > 0).sum()) > 8 else ''}); "
            f"first at image {n} row {y} column {x} channel {c}: stored {float(got[n, sy, sx, e])!r}, f32 path {float(exp[n, sy, sx, e])!r}"]
