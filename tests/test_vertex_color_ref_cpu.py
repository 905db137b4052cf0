"""tests/vertex_color_ref.py pinned on a hand-made triangle: corners red / green / blue."""
import numpy as np
import pytest

import vertex_color_ref as VR

FACES = np.array([[0, 1, 2]], np.int32)
COLORS = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
# (row py in rast_out's y-up order, column, b0, b1) -> expected rgb before shading
PIXELS = [(10, 20, 1 / 3, 1 / 3, (1 / 3, 1 / 3, 1 / 3)),      # centroid
          (0, 0, 1.0, 0.0, (1, 0, 0)), (159, 7, 0.0, 1.0, (0, 1, 0)), (80, 159, 0.0, 0.0, (0, 0, 1))]     # the three corners


@pytest.mark.parametrize("fmad", [True, False])
def test_interpolation_at_centroid_and_corners(fmad):
    for _, _, b0, b1, exp in PIXELS:
        got = VR.interpolate(np.float32(b0), np.float32(b1), 0, FACES, COLORS, fmad)
        np.testing.assert_allclose(got, exp, rtol=0, atol=1e-7)
    # corners are exact: 255 * fl(1/255) rounds to 1 and the other two products are zero
    assert (VR.interpolate(np.float32(1), np.float32(0), 0, FACES, COLORS, fmad) == [1, 0, 0]).all()


def test_render_flips_rows_shades_clamps_and_leaves_background_black():
    rast = np.zeros((1, VR.CROP, VR.CROP, 4), np.float32)
    shade = np.full((1, VR.CROP, VR.CROP), 0.9, np.float32)
    for py, px, b0, b1, _ in PIXELS:
        rast[0, py, px] = (b0, b1, 0.5, 1.0)           # triangle id + 1
    shade[0, VR.CROP - 1 - 159, 7] = 1.3                 # the green corner: 1 * 1.3 clamps to 1
    out = VR.render_rgb(rast, FACES, COLORS, shade)
    assert out.shape == (1, VR.CROP, VR.CROP, 3) and out.dtype == np.float32
    for py, px, _, _, exp in PIXELS:
        s = 1.3 if (py, px) == (159, 7) else 0.9
        np.testing.assert_allclose(out[0, VR.CROP - 1 - py, px], np.clip(np.array(exp) * s, 0, 1), rtol=0, atol=2e-7)
    mask = np.zeros((VR.CROP, VR.CROP), bool)
    for py, px, *_ in PIXELS:
        mask[VR.CROP - 1 - py, px] = True
    assert (out[0][~mask] == 0).all() and (out[0][mask].max(-1) > 0).all()


def test_lambert_factor_from_a_constant_grey_rendering():
    g = 128
    shade = np.float32([0.8, 1.0, 1.3])
    grey = (np.float32(g) * np.float32(1 / 255.0) * shade).astype(np.float32)
    got = VR.lambert_from_grey(np.repeat(grey[:, None], 3, 1), g)
    np.testing.assert_allclose(got, shade, rtol=3e-7)     # two f32 roundings
    with pytest.raises(AssertionError):
        VR.lambert_from_grey(grey, 200)                   # 1.3 * 200 / 255 >= 1: the grey rendering could have clamped
