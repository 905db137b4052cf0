"""numpy float64 references of the stages in front of and behind the render + crop stage, written from the RULES (the header comments of
fp_geometry.hip / fp_internal.h, DESIGN.md section 2.2, the reference project's lines those cite), with no expression of the oracle or
of the kernels and no f32 intermediate.  f32 enters only as data: frames, K, poses, the mesh diameter, and the constants the rules name
as f32 (0.001f, 0.1f, 0.8f, 0.01f), widened with float64(float32(c)).  Poses are [N, 4, 4] row-major; K is a row-major 3 x 3.

    xyz_ref                back-projection of a depth frame
    erode_ref              erode_depth (radius 2)
    bilateral_ref          bilateral_filter_depth (radius 2) + the tie margin of every pixel
    guess_translation_ref  GuessTranslation: bounding box, exact median, K^-1 (uc, vc, 1) zc
    crop_window_ref        ComputeCropWindowTF + ConstructBBox2D + the warp's inverse coefficients
    pose_update_ref        RefinePostProcess
    argmax_ref             first maximum; any NaN is an error
"""
import numpy as np


def f32c(c):
    """a constant the rules name as f32, as the double it is"""
    return np.float64(np.float32(c))


MIN_DEPTH = f32c(0.001)        # depth -> xyz cut, GuessTranslation's min_depth
DEPTH_LO, ZFAR = f32c(0.1), 100.0   # the filters' valid range [0.1, zfar)
ERODE_DIFF, ERODE_RATIO = f32c(0.001), f32c(0.8)
BILATERAL_BAND = f32c(0.01)
SIGMA_D, SIGMA_R = 2.0, 100000.0
RADIUS = 2
ROT_NORM = 0.349065850398865   # RefinePostProcess: tanh(rot) * rot_normalizer (20 degrees)
CROP = 160

ST_OK, ST_EMPTY_MASK, ST_NO_DEPTH = 0, 1, 2


def xyz_ref(depth, K, min_depth=MIN_DEPTH):
    """(u - cx) d / fx, (v - cy) d / fy, d; a depth below min_depth gives (0, 0, 0)"""
    d = np.asarray(depth, np.float64)
    K = np.asarray(K, np.float64)
    H, W = d.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.stack([(u - K[0, 2]) * d / K[0, 0], (v - K[1, 2]) * d / K[1, 1], d], -1)
    out[d < min_depth] = 0.0
    return out


ROW_BLOCK = 128   # the filters walk the frame in blocks of rows (25 taps of a 1920 x 1080 frame in float64 at once would take 400 MB each)


def _taps(a, radius, y0, y1, fill=0.0):
    """[(2 radius + 1)^2, y1 - y0, W]: tap (dy, dx) of every pixel of rows [y0, y1), `fill` where the tap lies outside the frame; and
    the squared distances"""
    H, W = a.shape
    p = np.full((H + 2 * radius, W + 2 * radius), fill, np.float64)
    p[radius:radius + H, radius:radius + W] = a
    taps, d2 = [], []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            taps.append(p[radius + dy + y0:radius + dy + y1, radius + dx:radius + dx + W])
            d2.append(float(dx * dx + dy * dy))
    return np.stack(taps), np.array(d2)


def _inside(hw, radius, y0, y1):
    """[(2 radius + 1)^2, y1 - y0, W] bool: the tap lies inside the frame"""
    return _taps(np.ones(hw), radius, y0, y1)[0] > 0


def _row_blocks(H):
    return [(y, min(y + ROW_BLOCK, H)) for y in range(0, H, ROW_BLOCK)]


def erode_ref(depth, radius=RADIUS, count_outside=False, strict=True):
    """A pixel outside [0.1, zfar) becomes 0.  Otherwise its (2 radius + 1)^2 window is walked: taps outside the frame are skipped and do
    not count in the total; a tap is bad when it is outside [0.1, zfar) or more than 0.001 away from the centre; the pixel becomes 0
    when bad / total > 0.8.  (count_outside / strict=False: the wrong rules of the negative controls.)"""
    d = np.asarray(depth, np.float64)
    out = np.zeros_like(d)
    for y0, y1 in _row_blocks(d.shape[0]):
        c = d[y0:y1]
        t, _ = _taps(d, radius, y0, y1)
        inside = _inside(d.shape, radius, y0, y1)
        bad = inside & ((t < DEPTH_LO) | (t >= ZFAR) | (np.abs(t - c[None]) > ERODE_DIFF))
        nbad = bad.sum(0).astype(np.float64)
        total = np.full(c.shape, float((2 * radius + 1) ** 2)) if count_outside else inside.sum(0).astype(np.float64)
        # bad / total > 0.8f, the f32 constant (0.800000011920929), decided in exact arithmetic
        kill = (nbad > ERODE_RATIO * total) if strict else (nbad >= np.float64(0.8) * total)
        o = np.where(kill, 0.0, c)
        o[(c < DEPTH_LO) | (c >= ZFAR)] = 0.0
        out[y0:y1] = o
    return out


def bilateral_ref(depth, radius=RADIUS, sigma_d=SIGMA_D, mean_over_all=False):
    """mean = average of the window's valid taps (inside the frame, in [0.1, zfar)); no valid tap: 0.  The output is the weighted average
    of the valid taps with |tap - mean| < 0.01, weight exp(-(dx^2 + dy^2) / (2 sigmaD^2) - (centre - tap)^2 / (2 sigmaR^2)) -- the centre
    as it is, valid or not, so an invalid centre is filled from its neighbours; no tap in the band: 0.
    -> (out, margin, tapmax): margin = the smallest | |tap - mean| - 0.01 | over the pixel's valid taps (inf without one), the distance
    of the nearest tap from changing sides; tapmax = the largest valid tap.  (mean_over_all: the wrong rule "a mean that includes
    invalid taps".)"""
    d = np.asarray(depth, np.float64)
    out, margin, tapmax = np.zeros_like(d), np.zeros_like(d), np.zeros_like(d)
    for y0, y1 in _row_blocks(d.shape[0]):
        t, d2 = _taps(d, radius, y0, y1)
        inside = _inside(d.shape, radius, y0, y1)
        valid = inside & (t >= DEPTH_LO) & (t < ZFAR)
        tv = np.where(valid, t, 0.0)
        n = valid.sum(0)
        if mean_over_all:
            mean = np.where(inside, t, 0.0).sum(0) / np.maximum(inside.sum(0), 1)
        else:
            mean = tv.sum(0) / np.maximum(n, 1)
        dist = np.abs(tv - mean[None])
        band = valid & (dist < BILATERAL_BAND)
        w = np.exp(-d2[:, None, None] / (2.0 * sigma_d * sigma_d) - (d[None, y0:y1] - tv) ** 2 / (2.0 * SIGMA_R * SIGMA_R)) * band
        sw = w.sum(0)
        out[y0:y1] = np.where((sw > 0) & (n > 0), (w * tv).sum(0) / np.where(sw > 0, sw, 1.0), 0.0)
        margin[y0:y1] = np.where(valid, np.abs(dist - BILATERAL_BAND), np.inf).min(0)
        tapmax[y0:y1] = tv.max(0)
    return out, margin, tapmax


def median_ref(values):
    """exact median of f32 values -> f32: an even count takes the mean of the two middle values in double, cast to f32"""
    s = np.sort(np.asarray(values, np.float32))
    n = len(s)
    if n % 2:
        return np.float32(s[n // 2])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32((np.float64(s[n // 2 - 1]) + np.float64(s[n // 2])) / 2.0)


def guess_translation_ref(filtered, mask, K, min_depth=MIN_DEPTH, lower_median=False, int_centre=False, mask_rule=None, strict_min=False):
    """-> (status, centre float64 [3] or None, zc f32 or None, (uc, vc) or None).  Bounding box of mask > 0 with centre (min + max) / 2;
    the values with mask > 0 and d >= min_depth (a NaN is not >= anything); their exact median zc; K^-1 (uc, vc, 1) zc.
    (lower_median / int_centre / mask_rule / strict_min: the wrong rules of the negative controls.)"""
    m = (np.asarray(mask) > 0) if mask_rule is None else mask_rule(np.asarray(mask))
    if not m.any():
        return ST_EMPTY_MASK, None, None, None
    vs, us = np.nonzero(m)
    su, sv = int(us.min()) + int(us.max()), int(vs.min()) + int(vs.max())
    uc, vc = (float(su // 2), float(sv // 2)) if int_centre else (su / 2.0, sv / 2.0)
    d = np.asarray(filtered, np.float32)[m]
    with np.errstate(invalid="ignore"):
        d64 = d.astype(np.float64)
        d = d[(d64 > np.float64(min_depth)) if strict_min else (d64 >= np.float64(min_depth))]
    if len(d) == 0:
        return ST_NO_DEPTH, None, None, (uc, vc)
    zc = np.sort(d)[(len(d) - 1) // 2] if lower_median else median_ref(d)
    with np.errstate(invalid="ignore", over="ignore"):
        centre = np.linalg.solve(np.asarray(K, np.float64), np.array([uc, vc, 1.0])) * np.float64(zc)
    return ST_OK, centre, np.float32(zc), (uc, vc)


def round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def crop_window_ref(poses, K, ratio, diameter, rounder=round_half_away, radius_column=1, size_plus_one=False):
    """Per pose: the translation t and t +- (r, 0, 0), t +- (0, r, 0) with r = diameter * ratio / 2 are projected with K; the centre is the
    first projection, the radius |max over the five of (v_k - v_0)| -- the v column only; the edges centre -+ radius are rounded half AWAY
    from zero; tf = [[sx, 0, -sx left], [0, sy, -sy top], [0, 0, 1]] with sx = 160 / (right - left), sy = 160 / (bottom - top);
    bbox = tf^-1 {(0, 0), (159, 159)}; the warp's inverse coefficients (m0, m2, m4, m5) = float32 of the double inverse of the F32 tf.
    -> dict of float64 arrays: raw [N, 4] unrounded (left, right, top, bottom), edges [N, 4], tf [N, 9], bbox [N, 4], centre [N, 2],
    radius [N].  `diameter` and `ratio` are f32 data; their product is not (r is formed in double).
    (rounder / radius_column / size_plus_one: the wrong rules of the negative controls.)"""
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    K = np.asarray(K, np.float64)
    r = np.float64(np.float32(diameter)) * np.float64(np.float32(ratio)) / 2.0
    off = np.array([[0, 0, 0], [r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0]], np.float64)
    pts = P[:, None, :3, 3] + off[None]                       # [N, 5, 3]
    q = pts @ K.T
    uv = q[..., :2] / q[..., 2:3]
    centre = uv[:, 0]
    radius = np.abs((uv[:, :, radius_column] - centre[:, None, radius_column]).max(1))
    raw = np.stack([centre[:, 0] - radius, centre[:, 0] + radius, centre[:, 1] - radius, centre[:, 1] + radius], 1)
    e = rounder(raw)
    return dict(raw=raw, centre=centre, radius=radius, size_plus_one=size_plus_one, **window_from_edges(e, size_plus_one))


def window_from_edges(e, size_plus_one=False):
    """tf and bbox of integer edges [N, 4] = (left, right, top, bottom), in float64"""
    e = np.asarray(e, np.float64)
    left, right, top, bottom = e.T
    one = 1.0 if size_plus_one else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        sx, sy = CROP / (right - left + one), CROP / (bottom - top + one)
        z, o = np.zeros_like(sx), np.ones_like(sx)
        tf = np.stack([sx, z, -sx * left, z, sy, -sy * top, z, z, o], 1)
        bbox = np.stack([left, top, left + (CROP - 1) / sx, top + (CROP - 1) / sy], 1)
    return dict(edges=e, tf=tf, bbox=bbox)


def warp_inverse_ref(tf_f32):
    """(m0, m2, m4, m5) [N, 4] f32 of an f32 tf [N, 9]: src = (m0 x + m2, m4 y + m5), the inverse taken in double and cast"""
    t = np.asarray(tf_f32, np.float32).astype(np.float64).reshape(-1, 9)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([1.0 / t[:, 0], -t[:, 2] / t[:, 0], 1.0 / t[:, 4], -t[:, 5] / t[:, 4]], 1).astype(np.float32)


def rodrigues(v):
    """rotation by |v| about v / |v| [N, 3] -> [N, 3, 3]; the zero vector gives the identity"""
    v = np.asarray(v, np.float64)
    ang = np.linalg.norm(v, axis=1)
    a = v / np.where(ang > 0, ang, 1.0)[:, None]
    Kx = np.zeros((len(v), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
    s, c = np.sin(ang)[:, None, None], np.cos(ang)[:, None, None]
    return np.eye(3)[None] + s * Kx + (1.0 - c) * (Kx @ Kx)


def pose_update_ref(poses, trans, rot, diameter, transpose=True, left=True, trans_scale=0.5, use_tanh=True):
    """t += trans * diameter / 2;  v = tanh(rot) * 0.349065850398865, Rd = Rodrigues(v);  R <- Rd^T R.  [N, 4, 4] float64.
    (transpose / left / trans_scale / use_tanh: the wrong rules of the negative controls.)"""
    P = np.array(np.asarray(poses, np.float32), np.float64).reshape(-1, 4, 4)
    tr, ro = np.asarray(trans, np.float32).astype(np.float64), np.asarray(rot, np.float32).astype(np.float64)
    Rd = rodrigues((np.tanh(ro) if use_tanh else ro) * ROT_NORM)
    if transpose:
        Rd = Rd.transpose(0, 2, 1)
    out = P.copy()
    out[:, :3, 3] = P[:, :3, 3] + tr * (np.float64(np.float32(diameter)) * trans_scale)
    out[:, :3, :3] = (Rd @ P[:, :3, :3]) if left else (P[:, :3, :3] @ Rd)
    return out


def argmax_ref(scores):
    """index of the first maximum; any NaN is an error"""
    s = np.asarray(scores, np.float32).ravel()
    if len(s) == 0 or np.isnan(s).any():
        raise ValueError("arg-max over NaN scores")
    return int(np.flatnonzero(s == s.max())[0])
