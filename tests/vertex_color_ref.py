"""Host reference of the vertex-colour shading rule (raster_shade_kernel<VCOL = true>) in numpy float32.

For a foreground pixel of triangle (i0, i1, i2) with the rasteriser's barycentrics (b0, b1), b2 = 1.f - b0 - b1:

    c_k[ch] = (float)u8 * (1.f / 255.f)
    rgb[ch] = dot3(b0, c_0[ch], b1, c_1[ch], b2, c_2[ch])       the attribute interpolation rule, in the model's float model
    o[ch]   = clamp(rgb[ch] * shade * fg, 0, 1)                 shade = mad(dif, 0.5, 0.8), the per-pixel Lambert factor

Inputs are what the library's own stage operators hand out: fp_debug_rasterize's rast_out [N, 160, 160, 4] = (b0, b1, z/w, triangle id + 1),
which is stored y-UP (row py) while render_out is flipped (row 159 - py); the face list; the colours.  The Lambert factor is taken from
the rgb of the SAME poses rendered with a constant texture of value g: a constant texture samples to exactly g / 255, so that rendering
is fl(fl(g/255 * shade) * fg) and shade = grey / (g / 255) up to two f32 roundings of values <= 1.3 (no clamp: 1.3 * g / 255 < 1)."""
import numpy as np

CROP = 160
F32 = np.float32


def _mad(a, b, c, fmad):
    """FMAD: one rounding (exact product and sum in float64, rounded to f32); else the product is rounded first"""
    if fmad:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    return (a * b).astype(F32) + c


def interpolate(b0, b1, tri, faces, colors, fmad=True):
    """rgb [..., 3] f32 of pixels with barycentrics b0, b1 (f32) on triangles tri (index into faces), before shading"""
    b0, b1 = np.asarray(b0, F32), np.asarray(b1, F32)
    b2 = (F32(1.0) - b0) - b1
    c = np.asarray(colors, np.uint8)[np.asarray(faces)[tri]].astype(F32) * F32(1.0 / 255.0)     # [..., corner, channel]
    out = np.empty(b0.shape + (3,), F32)
    for ch in range(3):
        acc = (b0 * c[..., 0, ch]).astype(F32)
        acc = _mad(b1, c[..., 1, ch], acc, fmad)
        out[..., ch] = _mad(b2, c[..., 2, ch], acc, fmad)
    return out


def lambert_from_grey(grey_rgb, g):
    """per-pixel shade * fg [N, 160, 160] from channel 0 of the rendering with a constant texture of value g (render_out orientation)"""
    assert 1.3 * g / 255.0 < 1.0
    return np.asarray(grey_rgb, F32)[..., 0] / (F32(g) * F32(1.0 / 255.0))


def render_rgb(rast, faces, colors, shade, fmad=True):
    """channels 0..2 of render_out [N, 160, 160, 3] f32: rast = fp_debug_rasterize's rast_out (y-up), shade = lambert_from_grey(...)
    (already in render_out's orientation)"""
    rast = np.asarray(rast, F32)[:, ::-1]          # y-up -> the flipped order render_out is stored in
    tid = rast[..., 3].astype(np.int64) - 1
    fg = tid >= 0
    rgb = interpolate(rast[..., 0], rast[..., 1], np.where(fg, tid, 0), faces, colors, fmad)
    o = np.clip((rgb * np.asarray(shade, F32)[..., None]).astype(F32), F32(0), F32(1))
    return np.where(fg[..., None], o, F32(0)).astype(F32)
