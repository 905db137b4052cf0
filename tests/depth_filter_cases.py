"""Inputs and host-side references shared by tests/test_depth_filter_cpu.py and tests/test_depth_filter_gpu.py (fp_set_depth_filter,
DESIGN.md section 4.7).

filter_frame    the generated frame family: the project's noise frames (uniform(0.2, 2.0)) erode to all zeros, so a filter test on them
                compares zeros with zeros.  These frames are eight tilted planes quantised to 1 mm (most of a plane survives the erosion),
                one of them straddling 0.1 m and one straddling 100 m (erode's validity limits), one made of 3-pixel stripes whose offset
                walks across 16..24 mm (neighbourhoods on both sides of the bilateral's |d - mean| < 0.01), 2 % holes and isolated spikes
window_before   the window estimate of Track as it stood before plan_track_window existed, transcribed: the expectation of reach 0"""
import math

import numpy as np

WHOLE, OUTSIDE, ROWS, RECT = range(4)           # fp_internal.h TrackWindowKind


def filter_frame(H, W, seed, z_lo=0.4, z_hi=1.5):
    """-> (rgb [H,W,3] u8 noise, depth [H,W] f32); the planes' base depths are drawn from [z_lo, z_hi]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    region = (xx * 4 // W).astype(int) + 4 * (yy * 2 // H).astype(int)
    d = np.zeros((H, W), np.float64)
    for r in range(8):
        base = rng.uniform(z_lo, z_hi)
        gx, gy = rng.uniform(-4e-4, 4e-4, 2)
        plane = base + gx * (xx - W / 2) + gy * (yy - H / 2)
        if r == 5:      # straddles erode's near limit: 0.095 .. 0.105
            plane = 0.1 + 0.005 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
        if r == 6:      # straddles zfar
            plane = 100.0 + 0.01 * np.sin(xx / 9.0 + yy / 11.0)
        if r == 2:      # stripes three pixels wide, 16 .. 24 mm apart: |d - mean| on both sides of 0.01
            plane = base + ((xx // 3) % 2) * (0.016 + 0.008 * yy / H)
        d = np.where(region == r, plane, d)
    d = np.round(d * 1000.0) / 1000.0
    spikes = rng.random((H, W)) < 0.005
    d = np.where(spikes, d + rng.uniform(0.05, 0.5, (H, W)), d)
    d = np.where(rng.random((H, W)) < 0.02, 0.0, d)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return rgb, d.astype(np.float32)


def window_before(K, diameter, pose, H, W):
    """track_submit_impl's estimate (host frame, refine_itr 1) before it became plan_track_window, followed by upload_frame_async's
    clamps -> (kind, row0, row1, col0, col1) and the unclamped (row0, row1, col0, col1) the estimate itself produced (None: no such)"""
    K = [float(np.float32(v)) for v in np.asarray(K).reshape(9)]
    r = float(np.float32(diameter)) * 1.2 / 2
    tx, ty, tz = (float(np.float32(pose[i][3])) for i in range(3))

    def div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)

    def proj_v(x, y, z):
        return div(K[3] * x + K[4] * y + K[5] * z, K[6] * x + K[7] * y + K[8] * z)

    def proj_u(x, y, z):
        return div(K[0] * x + K[1] * y + K[2] * z, K[6] * x + K[7] * y + K[8] * z)

    row0, row1, col0, col1 = 0, -1, 0, -1
    kind, raw = WHOLE, None
    if tz > 1e-6:
        v0 = proj_v(tx, ty, tz)
        rad = 0.0
        for ox, oy in ((r, 0), (-r, 0), (0, r), (0, -r)):
            rad = max(rad, abs(proj_v(tx + ox, ty + oy, tz) - v0))       # (std::max(rad, NaN) keeps rad, and so does Python's max)
        if math.isfinite(v0) and math.isfinite(rad) and rad < 4.0 * H:
            if v0 + rad + 5 <= 0 or v0 - rad - 4 >= H:
                row0, row1, kind = 0, 0, OUTSIDE
            elif -float(H) < v0 < 2.0 * H:
                row0 = math.floor(v0 - rad) - 4
                row1 = math.ceil(v0 + rad) + 5
                kind = ROWS
                u0 = proj_u(tx, ty, tz)
                if math.isfinite(u0) and -float(W) < u0 < 2.0 * W:
                    col0 = math.floor(u0 - rad) - 4
                    col1 = math.ceil(u0 + rad) + 5
                    if col1 <= 0 or col0 >= W:
                        col0, col1 = 0, -1
                    else:
                        kind = RECT
                raw = (row0, row1, col0, col1)
    return (kind,) + clamp(row0, row1, col0, col1, H, W), raw


def clamp(row0, row1, col0, col1, H, W):
    """upload_frame_async's clamps of a row / column range"""
    if row1 < 0 or row1 > H:
        row1 = H
    row0 = max(0, min(row0, row1))
    if col1 < 0 or col1 > W:
        col1 = W
    col0 = max(0, min(col0, col1))
    return row0, row1, col0, col1
