"""Float64 pins of depth -> xyz, erode, bilateral, GuessTranslation, the crop window, RefinePostProcess and arg-max.

Four parts, none needs a GPU:
  (a) the references of tests/pose_rules_ref.py against hand-derived answers, written as fractions;
  (b) the oracle against the references over the inputs of tests/pose_rules_cases.py;
  (c) the bounds, derived from rounding counts (u = 2^-24), the exemptions and their caps -- and a re-measurement of every peak on the
      oracle: a peak above HALF of its bound fails (the derivation would be wrong; the constant is not to be raised);
  (d) negative controls: every wrong rule fails its assertion on every case it can differ on.
tests/test_pose_rules_gpu.py imports the cases, checks, bounds, exemptions and caps from here and applies them to the device's outputs.
"""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

import pose_rules_cases as PC
import pose_rules_ref as R
from foundationpose_cpp_amd import synthetic as syn
from oracle import fp_oracle as fo

U = 2.0 ** -24                 # unit roundoff of f32: one correctly rounded operation errs by at most u relative
HALF = 0.5                     # a peak above half of a derived bound means the derivation is wrong

# ---- bounds: counted roundings (DESIGN.md section 2.2 spells the counts out) -----------------------------------------------------------
XYZ_C = 6.0                    # (c - cx), * d, / fx: 3 roundings, times the factor 2 of the half rule (3 independent roundings reach 2 u)
BILATERAL_C = 64.0             # per sum: expf (2 ulp = 4 u) + its argument (2 u) + the product (1) + 24 additions = 31; two sums + the division
BILATERAL_TIE_C = 32.0         # f32 error of the mean: 24 additions + the division, rounded up: a tap this close to the band may take either side
BILATERAL_TIE_CAP = 0.002      # share of a frame
TRANS_XY_C = 14.0              # K^-1 by cofactors (fy * id: 3, cx fy * id: 4), * uc (1), two additions (2), * zc (1): 7 at most per term, times 2
TRANS_Z_C = 6.0                # det * id (2 + 1), * zc (1): 3, times 2
EDGE_CENTRE_C = 5.0            # a projected centre coordinate: 2 products, 2 sums, 1 division, relative to |u0 - cx| + |cx|
EDGE_RADIUS_C = 11.0           # the radius: two such projections of the v column (one with the + r: 6) and their difference, relative to |v0 - cy| + |cy| + radius
EDGE_SUM_C = 1.0               # centre -+ radius, relative to |centre| + radius
EDGE_CAP = 0.02                # share of the windows of a sweep with an edge one off
TF_C = 4.0                     # sx: one division (exact integer operands); sx * (-left): one more; times 2
BBOX_C = 8.0                   # 1 / sx (2), -tf2 / tf0 (4), * 159 and the sum (2)
ROT_C = 24.0                   # tanhf, sinf, cosf (2 ulp each), norm and axis (6), 9 entries of Rd (<= 12 u each) through a 3-term product
POSE_T_C = 4.0                 # trans * (d / 2) and the sum: 2 roundings, times 2


def _frac(err, bound, what):
    """largest err / bound over the elements with a positive bound; elements with a zero bound have to be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    z = bound <= 0
    assert not (err[z] > 0).any(), f"{what} off: a value that has to be exact is not"
    return float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0


# ---- checks: each returns its peaks as fractions of the bounds and asserts the bounds ----------------------------------------------------
def check_xyz(got, depth, K, ref_fn=R.xyz_ref):
    ref = ref_fn(depth, K)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    f = _frac(np.abs(got - ref), XYZ_C * U * np.abs(ref), "xyz")
    assert f <= 1.0, f"xyz off: {f:.3g} of the bound"
    return dict(xyz=f)


def check_erode(got, depth, ref_fn=R.erode_ref):
    ref = ref_fn(depth).astype(np.float32)
    bad = np.asarray(got, np.float32) != ref
    assert not bad.any(), f"erode differs at {int(bad.sum())} pixels, first {tuple(np.argwhere(bad)[0])}"
    return dict(erode=0.0)


def check_bilateral(got, eroded, ref_fn=R.bilateral_ref):
    ref, margin, tapmax = ref_fn(eroded)
    got = np.asarray(got, np.float64)
    exempt = margin < BILATERAL_TIE_C * U * tapmax
    share = float(exempt.mean())
    assert share <= BILATERAL_TIE_CAP, f"bilateral: {share:.3%} of the frame within the tie margin (cap {BILATERAL_TIE_CAP:.1%})"
    # an exempted pixel still holds an average of its taps, or nothing
    assert ((got[exempt] >= 0) & (got[exempt] <= tapmax[exempt] * (1 + BILATERAL_C * U))).all(), "bilateral: an exempted pixel holds no average of its taps"
    f = _frac(np.abs(got - ref)[~exempt], (BILATERAL_C * U * np.abs(ref))[~exempt], "bilateral")
    assert f <= 1.0, f"bilateral off: {f:.3g} of the bound"
    return dict(bilateral=f, tie_share=share)


def check_translation(got, filtered, mask, K, min_depth=R.MIN_DEPTH, ref_fn=R.guess_translation_ref):
    """got: the translation [3] (None: the call failed) for `filtered` = the output of the filter UNDER TEST, so that the median is exact"""
    st, centre, zc, uvc = ref_fn(filtered, mask, K, min_depth)
    assert (got is None) == (st != R.ST_OK), f"translation: failure {got is None} against the reference's status {st}"
    if got is None:
        return dict(tx=0.0, ty=0.0, tz=0.0)
    K = np.asarray(K, np.float64)
    z = abs(float(zc))
    bx = TRANS_XY_C * U * (abs(uvc[0]) + abs(K[0, 2])) / K[0, 0] * z
    by = TRANS_XY_C * U * (abs(uvc[1]) + abs(K[1, 2])) / K[1, 1] * z
    bz = TRANS_Z_C * U * z
    e = np.abs(np.asarray(got, np.float64) - centre)
    s = dict(tx=_frac(e[0], bx, "translation"), ty=_frac(e[1], by, "translation"), tz=_frac(e[2], bz, "translation"))
    assert max(s.values()) <= 1.0, f"translation off: {s} (got {got}, reference {centre})"
    return s


def check_translation_bits(got, vals, mask, min_depth, ref_fn=R.guess_translation_ref):
    """K = identity: the centre is (uc zc, vc zc, zc), each a single rounding of an exact product (uc has 12 bits, zc 24): the median bit for
    bit.  got: the translation [3] f32, or None when the call failed"""
    st, c, zc, _ = ref_fn(vals, mask, np.eye(3), np.float32(min_depth))
    assert (got is None) == (st != R.ST_OK), f"translation: failure {got is None} against the reference's status {st}"
    if got is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            want = c.astype(np.float32)
        assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), want.view(np.uint32)), f"translation bits off: {got} against {want}"
    return st


def edges_of_tf(tf):
    """the integer edges (left, right, top, bottom) [N, 4] a tf [N, 9] f32 was built from, recovered in double: left = -tf2 / sx, right = left +
    160 / sx; they have to be integers"""
    t = np.asarray(tf, np.float32).astype(np.float64).reshape(-1, 9)
    assert np.isfinite(t).all() and (t[:, 0] > 0).all() and (t[:, 4] > 0).all(), "a window without a size"
    raw = np.stack([-t[:, 2] / t[:, 0], -t[:, 2] / t[:, 0] + R.CROP / t[:, 0], -t[:, 5] / t[:, 4], -t[:, 5] / t[:, 4] + R.CROP / t[:, 4]], 1)
    e = np.rint(raw)
    assert (np.abs(raw - e) <= 1e-4 * np.maximum(1.0, np.abs(e))).all(), "window edges off: not integers"
    assert not t[:, [1, 3, 6, 7]].any() and (t[:, 8] == 1).all(), "tf is not [[sx, 0, .], [0, sy, .], [0, 0, 1]]"
    return e


def check_window(tf, bbox, poses, K, ratio, diameter, exempt_ties=True, ref_fn=R.crop_window_ref, coeffs=None):
    """tf [N, 9], bbox [N, 4] f32 (and coeffs [N, 4] = m0, m2, m4, m5 where the side under test returns them) against crop_window_ref"""
    ref = ref_fn(poses, K, ratio, diameter)
    e = edges_of_tf(tf)
    diff = e - ref["edges"]
    K64 = np.asarray(K, np.float64)
    c, rad = ref["centre"], ref["radius"]
    su, sv = np.abs(c[:, 0] - K64[0, 2]) + abs(K64[0, 2]), np.abs(c[:, 1] - K64[1, 2]) + abs(K64[1, 2])
    r_err = EDGE_RADIUS_C * (sv + rad)                   # the radius comes from the v column, for the x edges too
    tol_x = U * (EDGE_CENTRE_C * su + r_err + EDGE_SUM_C * (np.abs(c[:, 0]) + rad))
    tol_y = U * (EDGE_CENTRE_C * sv + r_err + EDGE_SUM_C * (np.abs(c[:, 1]) + rad))
    near_tie = np.abs(np.abs(ref["raw"] - np.floor(ref["raw"])) - 0.5) <= np.stack([tol_x, tol_x, tol_y, tol_y], 1)
    allowed = (diff == 0) | ((np.abs(diff) == 1) & near_tie & exempt_ties)
    assert allowed.all(), f"window edges off: pose {int(np.argwhere(~allowed)[0][0])} has {e[np.argwhere(~allowed)[0][0]]} against {ref['edges'][np.argwhere(~allowed)[0][0]]}"
    share = float((diff != 0).any(1).mean())
    assert share <= EDGE_CAP, f"{share:.2%} of the windows have an edge one off (cap {EDGE_CAP:.0%})"
    own = R.window_from_edges(e, ref["size_plus_one"])           # tf and bbox of the edges the side under test chose
    t = np.asarray(tf, np.float64).reshape(-1, 9)
    # sx, sy: the one correctly rounded division of the rule
    assert np.array_equal(np.float32(own["tf"][:, [0, 4]]), np.float32(t[:, [0, 4]])), "tf / bbox off: sx, sy are not float32(160 / size)"
    f_tf = _frac(np.abs(t - own["tf"]), TF_C * U * np.abs(own["tf"]), "tf / bbox")
    ext = np.stack([np.abs(e[:, 0]) + np.abs(e[:, 1]), np.abs(e[:, 2]) + np.abs(e[:, 3])] * 2, 1)
    f_bb = _frac(np.abs(np.asarray(bbox, np.float64) - own["bbox"]), BBOX_C * U * ext, "tf / bbox")
    assert f_tf <= 1.0 and f_bb <= 1.0, f"tf / bbox off: {f_tf:.3g} / {f_bb:.3g} of the bounds"
    if coeffs is not None:
        want = R.warp_inverse_ref(tf)
        assert np.array_equal(np.asarray(coeffs, np.float32).view(np.uint32), want.view(np.uint32)), "m0, m2, m4, m5 are not float32 of the double inverse of tf"
    return dict(tf=f_tf, bbox=f_bb, edge_share=share)


def check_pose_update(got, poses, trans, rot, diameter, ref_fn=R.pose_update_ref):
    ref = ref_fn(poses, trans, rot, diameter)
    got = np.asarray(got, np.float64).reshape(-1, 4, 4)
    f_r = float(np.abs(got[:, :3, :3] - ref[:, :3, :3]).max() / (ROT_C * U))
    td = np.abs(np.asarray(trans, np.float64)) * (float(np.float32(diameter)) / 2)
    f_t = _frac(np.abs(got[:, :3, 3] - ref[:, :3, 3]), POSE_T_C * U * (np.abs(np.asarray(poses, np.float64)[:, :3, 3]) + td), "pose update")
    assert np.array_equal(got[:, 3], np.asarray(poses, np.float64)[:, 3]), "pose update: the bottom row changed"
    assert f_r <= 1.0 and f_t <= 1.0, f"pose update off: rotation {f_r:.3g}, translation {f_t:.3g} of the bounds"
    return dict(rot=f_r, trans=f_t)


ARGMAX_ERROR = "error"        # the outcome of an arg-max over scores with a NaN


def argmax_outcome(fn, scores, error=ValueError):
    """fn(scores) -> its index, or ARGMAX_ERROR when it refuses with `error`"""
    try:
        return int(fn(scores))
    except error:
        return ARGMAX_ERROR


def check_argmax(got, scores, ref_fn=R.argmax_ref):
    """got: the outcome of the side under test, an index or ARGMAX_ERROR"""
    want = argmax_outcome(ref_fn, scores)
    assert got == want, f"arg-max {got}, the rule gives {want}"


def print_row(kind, name, s, extra=""):
    cols = " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in s.items())
    print(f"  {kind:11s} {name:10s} {extra}: {cols}")


# ---- (a) references against hand-derived answers ----------------------------------------------------------------------------------------
def test_window_ties_by_hand():
    poses = PC.hand_poses()
    ref = R.crop_window_ref(poses, PC.HAND_K, PC.HAND_RATIO, PC.HAND_DIAMETER)
    for i, ((a, b), edges) in enumerate(PC.HAND_WINDOWS):
        assert ref["radius"][i] == PC.HAND_RADIUS and tuple(ref["centre"][i]) == (float(a), float(b))
        assert tuple(ref["raw"][i]) == (float(a - 48), float(a + 48), float(b - 48), float(b + 48))
        assert tuple(ref["edges"][i]) == edges, (i, ref["edges"][i])
        left, right, top, bottom = edges
        sx, sy = Fr(160, right - left), Fr(160, bottom - top)
        np.testing.assert_allclose(ref["tf"][i], [float(sx), 0, float(-sx * left), 0, float(sy), float(-sy * top), 0, 0, 1], rtol=1e-15)
        np.testing.assert_allclose(ref["bbox"][i], [left, top, float(left + 159 / sx), float(top + 159 / sy)], rtol=1e-15, atol=1e-13)
    assert PC.hand_poses()[0, 0, 3] == np.float32(-299 / 256) and ref["raw"][0, 0] == -46.5 and ref["edges"][0, 0] == -47
    # the inverse coefficients: tf = [[2, 0, -6], [0, 4, 8]] -> src = (x / 2 + 3, y / 4 - 2)
    m = R.warp_inverse_ref(np.array([[2, 0, -6, 0, 4, 8, 0, 0, 1]], np.float32))
    assert m.tolist() == [[0.5, 3.0, 0.25, -2.0]]
    # the radius takes the v column: fy = 2 fx doubles it, fx does not enter
    K2 = np.array([[100, 0, 50], [0, 200, 50], [0, 0, 1]], np.float32)
    r2 = R.crop_window_ref(syn.pose_matrix(np.eye(3), (0, 0, 1))[None], K2, 1.0, 0.5)
    assert r2["radius"][0] == 50.0 and tuple(r2["edges"][0]) == (0, 100, 0, 100)


def _frame_of(rows):
    return np.array(rows, np.float32)


def test_erode_and_bilateral_by_hand():
    # bad / total against 0.8: 20/25, 12/15 (a frame edge), 4/5 (a frame one row high) are not above it; 7/9 and 8/9 at the corners
    for nbad, total, hw, centre in ((20, 25, (9, 9), (4, 4)), (21, 25, (9, 9), (4, 4)), (12, 15, (9, 9), (4, 0)), (13, 15, (9, 9), (4, 0)),
                                    (12, 15, (9, 9), (8, 4)), (7, 9, (9, 9), (0, 0)), (8, 9, (9, 9), (8, 8)), (4, 5, (1, 7), (0, 3))):
        f = np.full(hw, 0.5, np.float32)
        cy, cx = centre
        taps = [(y, x) for y in range(cy - 2, cy + 3) for x in range(cx - 2, cx + 3) if 0 <= y < hw[0] and 0 <= x < hw[1] and (y, x) != centre]
        assert len(taps) + 1 == total, (len(taps), total)
        for k, (y, x) in enumerate(taps[:nbad]):
            f[y, x] = (0.5 + 0.0011, 0.05, 100.0, 0.5 - 0.002)[k % 4]      # too far above, under 0.1, at zfar, too far below
        want = 0.0 if Fr(nbad, total) > Fr(4, 5) else 0.5
        assert R.erode_ref(f)[centre] == np.float32(want), (nbad, total, centre)
    # the difference rule is "more than 0.001f": the largest f32 not more than 0.001f above the centre stays good, the next one is bad
    lo = np.float32(0.125 + R.ERODE_DIFF)
    lo = lo if np.float64(lo) - 0.125 <= R.ERODE_DIFF else np.nextafter(lo, np.float32(0))
    hi = np.nextafter(lo, np.float32(1))
    assert np.float64(lo) - 0.125 <= R.ERODE_DIFF < np.float64(hi) - 0.125
    for tap, want in ((lo, 0.125), (hi, 0.0)):
        e = np.full((5, 5), tap, np.float32)
        e[2, 2] = 0.125
        assert R.erode_ref(e)[2, 2] == want
    # out of range centres
    assert R.erode_ref(_frame_of([[0.05, 100.0, 99.0]]))[0].tolist() == [0.0, 0.0, 99.0]

    # bilateral: an invalid centre between two valid neighbours at distance 1 (equal weights) is filled with their average
    b = np.zeros((5, 5), np.float32)
    b[2, 1], b[2, 3] = 0.5, 0.504
    out, margin, tapmax = R.bilateral_ref(b)
    np.testing.assert_allclose(out[2, 2], 0.502, rtol=1e-7)          # (f32 data: 0.504f is not 0.504)
    assert tapmax[2, 2] == np.float64(np.float32(0.504))
    np.testing.assert_allclose(margin[2, 2], 0.01 - 0.002, rtol=1e-5)
    # weights: centre 1.0 (weight 1), one tap at distance 1 (e^-1/8), one at distance sqrt(8) (e^-1), all within the band
    b = np.zeros((5, 5), np.float32)
    b[2, 2], b[2, 3], b[0, 0] = 1.0, 1.00390625, 0.99609375
    w1, w8 = np.exp(-1 / 8), np.exp(-1.0)
    out, _, _ = R.bilateral_ref(b)
    np.testing.assert_allclose(out[2, 2], (1.0 + w1 * 1.00390625 + w8 * 0.99609375) / (1 + w1 + w8), rtol=1e-9)   # (the range term is 1e-15)
    # a tap 0.02 from the mean of three is left out; without a tap in the band: 0; no valid tap: 0
    b = np.zeros((5, 5), np.float32)
    b[2, 2], b[2, 3], b[2, 1] = 0.5, 0.5, 0.53
    out, margin, _ = R.bilateral_ref(b)       # mean 0.51 - 1e-8 (0.53f is below 0.53): the 0.5s are 0.0099999905 away, inside 0.01f = 0.0099999998
    assert out[2, 2] == 0.5 and 0 < margin[2, 2] < 1e-8
    b[2, 1] = 0.56                                                     # mean 0.52: every tap >= 0.02 away -> nothing
    assert R.bilateral_ref(b)[0][2, 2] == 0.0
    assert R.bilateral_ref(np.zeros((3, 3), np.float32))[0].tolist() == [[0.0] * 3] * 3
    # frame corner: the window of (0, 0) of a constant frame holds 9 taps, the result is the constant
    np.testing.assert_allclose(R.bilateral_ref(np.full((4, 4), 0.75, np.float32))[0][0, 0], 0.75, rtol=1e-15)


def test_median_box_and_translation_by_hand():
    f = np.float32
    assert R.median_ref([f(0.5)]) == f(0.5)
    assert R.median_ref([f(0.75), f(0.25)]) == f(0.5)
    assert R.median_ref([f(0.9), f(0.1), f(0.9)]) == f(0.9)                       # duplicates
    assert R.median_ref([f(4), f(1), f(2), f(2)]) == f(2)
    assert R.median_ref([f(4), f(1), f(3), f(2)]) == f(2.5)
    a, b = f(0.49999997), f(0.5)                                                   # neighbours: the mean is a tie, rounded to even
    assert R.median_ref([a, b]) == f((float(a) + float(b)) / 2) and R.median_ref([a, b]) in (a, b)
    assert R.median_ref([f(1), f(np.inf)]) == f(np.inf)
    K = np.array([[100, 0, 10], [0, 50, 20], [0, 0, 1]], np.float32)
    d = np.full((6, 8), 2.0, np.float32)
    for pix, centre in (([(3, 5)], (5.0, 3.0)), ([(0, 0), (5, 7)], (3.5, 2.5)), ([(0, 0)], (0.0, 0.0)), ([(5, 7)], (7.0, 5.0)), ([(1, 2), (1, 5), (4, 3)], (3.5, 2.5))):
        m = np.zeros((6, 8), np.uint8)
        for y, x in pix:
            m[y, x] = 1
        st, c, zc, uvc = R.guess_translation_ref(d, m, K)
        assert st == R.ST_OK and uvc == centre and zc == 2.0
        np.testing.assert_allclose(c, [float(Fr(2) * (Fr(centre[0]) - 10) / 100), float(Fr(2) * (Fr(centre[1]) - 20) / 50), 2.0], rtol=1e-15)
    assert R.guess_translation_ref(d, np.zeros((6, 8), np.uint8), K)[0] == R.ST_EMPTY_MASK
    m = np.ones((6, 8), np.uint8)
    assert R.guess_translation_ref(np.full((6, 8), 0.0005, np.float32), m, K)[0] == R.ST_NO_DEPTH
    at = np.full((6, 8), np.float32(0.001))
    assert R.guess_translation_ref(at, m, K)[0] == R.ST_OK                            # d >= min_depth: equality counts
    assert R.guess_translation_ref(np.full((6, 8), np.nan, np.float32), m, K)[0] == R.ST_NO_DEPTH


def test_xyz_pose_update_and_argmax_by_hand():
    K = np.array([[100, 0, 2], [0, 50, 1], [0, 0, 1]], np.float32)
    d = _frame_of([[1.0, 0.0005, 2.0], [0.5, np.float32(0.001), 4.0]])
    x = R.xyz_ref(d, K)
    assert x[0, 0].tolist() == [-0.02, -0.02, 1.0] and x[0, 1].tolist() == [0, 0, 0] and x[0, 2].tolist() == [0.0, -0.04, 2.0]
    assert x[1, 0].tolist() == [-0.01, 0.0, 0.5] and x[1, 1, 2] == np.float64(np.float32(0.001)) and x[1, 2].tolist() == [0.0, 0.0, 4.0]
    pose = syn.pose_matrix(syn.random_rotation(9), (0.1, -0.2, 0.7))[None]
    z = np.zeros((1, 3), np.float32)
    assert np.array_equal(R.pose_update_ref(pose, z, z, 0.2)[0], pose[0].astype(np.float64))                  # zero update
    out = R.pose_update_ref(pose, np.array([[1, 2, 3]], np.float32), z, 0.25)[0]
    assert np.array_equal(out[:3, :3], pose[0, :3, :3]) and np.array_equal(out[:3, 3], pose[0, :3, 3].astype(np.float64) + 0.125 * np.array([1, 2, 3]))
    ang = 0.5 * 0.349065850398865                                               # rot = atanh(1/2) about x: Rd = Rx(ang), R <- Rx(ang)^T R
    rot = np.array([[np.arctanh(0.5), 0, 0]], np.float32)
    Rx = np.array([[1, 0, 0], [0, np.cos(ang), -np.sin(ang)], [0, np.sin(ang), np.cos(ang)]])
    np.testing.assert_allclose(R.pose_update_ref(pose, z, rot, 0.2)[0, :3, :3], Rx.T @ pose[0, :3, :3].astype(np.float64), atol=2e-8)   # (atanh(1/2) as f32)
    assert R.argmax_ref([0.1, 0.9, 0.9, 0.3]) == 1 and R.argmax_ref([-5.0]) == 0 and R.argmax_ref([-np.inf, -np.inf]) == 0
    assert R.argmax_ref([-0.0, 0.0]) == 0 and R.argmax_ref([0.0, -0.0, 1.0]) == 2
    with pytest.raises(ValueError):
        R.argmax_ref([0.5, np.nan])


# ---- (b) + (c) the oracle against the references ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_filters(name):
    f = PC.frame(name)
    e = fo.erode_depth(f.depth)
    return e, fo.bilateral_filter_depth(e)


def oracle_frame_peaks(name):
    f = PC.frame(name)
    e, b = oracle_filters(name)
    s = {}
    s.update(check_xyz(fo.depth_to_xyz(f.depth, f.K), f.depth, f.K))
    s.update(check_erode(e, f.depth))
    s.update(check_bilateral(b, e))
    s.update(check_translation(fo.guess_translation(b, f.mask, f.K), b, f.mask, f.K))
    return s


def oracle_window_peaks(seed, ratio):
    mesh, K, poses, _ = PC.sweep_poses(seed)
    tf = fo.crop_window_tf(syn.to_colmajor(poses), K, ratio, mesh.diameter)
    return check_window(tf, fo.bbox2d(tf), poses, K, ratio, mesh.diameter)


def oracle_pose_update_peaks():
    poses, trans, rot = PC.pose_updates()
    out = syn.from_colmajor(fo.refine_post_process(syn.to_colmajor(poses), trans, rot, 0.1937))
    return check_pose_update(out, poses, trans, rot, 0.1937)


@functools.lru_cache(maxsize=None)
def measure_peaks():
    """every peak of the oracle over the case list, as fractions of the bounds"""
    peaks = {}

    def fold(s):
        for k, v in s.items():
            peaks[k] = max(peaks.get(k, 0.0), v)

    for name in PC.CPU_FRAMES:
        fold(oracle_frame_peaks(name))
    for seed in range(12):
        for ratio in PC.RATIOS:
            fold(oracle_window_peaks(seed, ratio))
    fold(oracle_pose_update_peaks())
    return peaks


PEAK_KEYS = ("xyz", "bilateral", "tx", "ty", "tz", "tf", "bbox", "rot", "trans")


@pytest.mark.parametrize("name", PC.CPU_FRAMES)
def test_oracle_filters_and_translation(name):
    s = oracle_frame_peaks(name)
    print_row("frame", name, s)
    assert PC.frame(name).mask.any()


def test_oracle_windows():
    n = 0
    for seed in range(12):
        for ratio in PC.RATIOS:
            s = oracle_window_peaks(seed, ratio)
            print_row("window", f"rnd{seed}", s, f"ratio {ratio}")
            n += 200
    assert n == 4800
    # the hand-made ties: no exemption
    tf = fo.crop_window_tf(syn.to_colmajor(PC.hand_poses()), PC.HAND_K, PC.HAND_RATIO, PC.HAND_DIAMETER)
    check_window(tf, fo.bbox2d(tf), PC.hand_poses(), PC.HAND_K, PC.HAND_RATIO, PC.HAND_DIAMETER, exempt_ties=False)
    assert edges_of_tf(tf).tolist() == [list(map(float, e)) for _, e in PC.HAND_WINDOWS]


def test_oracle_pose_update_and_argmax():
    print_row("pose update", "2000", oracle_pose_update_peaks())
    poses, trans, rot = PC.pose_updates()
    out = syn.from_colmajor(fo.refine_post_process(syn.to_colmajor(poses), trans, rot, 0.1937))
    assert np.array_equal(out[0], poses[0])                                     # the zero update returns its input
    for name, s in PC.argmax_cases():
        check_argmax(fo.argmax(s), s)
    # (the C oracle has no error path: it answers an index for scores with a NaN, so the rule "any NaN is an error" is held on the
    # device alone, tests/test_pose_rules_gpu.py::test_argmax)


def test_oracle_sampler_patterns_bit_for_bit():
    """K = identity: the centre is (uc zc, vc zc, zc), each a single rounding of an exact product -- the oracle's median bit for bit"""
    for p in PC.sampler_patterns() + PC.sampler_sequence():
        try:
            check_translation_bits(fo.guess_translation(p.vals, p.mask, np.eye(3, dtype=np.float32), p.min_depth), p.vals, p.mask, p.min_depth)
        except AssertionError as e:
            raise AssertionError(f"{p.name}: {e}") from None


def test_measured_peaks_stay_under_half_of_their_bounds():
    """re-measured on the oracle: a peak above half of its bound means the derivation is wrong; the caps hold on the oracle alone (the checks
    assert them).  DESIGN.md section 2.2 records these numbers."""
    peaks = measure_peaks()
    print("  oracle peaks as fractions of their bounds: " + " ".join(f"{k}={peaks[k]:.3g}" for k in peaks))
    for k in PEAK_KEYS:
        assert 0 < peaks[k] <= HALF, (k, peaks[k])
    assert peaks["tie_share"] <= BILATERAL_TIE_CAP and peaks["edge_share"] <= EDGE_CAP


# ---- (d) negative controls -------------------------------------------------------------------------------------------------------------------
def _small(name, rows=480, cols=641):
    """the frame, or its top-left corner: a control re-runs the float64 filters per wrong rule"""
    f = PC.frame(name)
    return f.depth[:rows, :cols], f.mask[:rows, :cols], f.K


def _half_even(x):
    return np.rint(x)


def _floor_half(x):
    return np.floor(np.asarray(x) + 0.5)


WRONG_WINDOWS = {
    "half-even rounding": functools.partial(R.crop_window_ref, rounder=_half_even),
    "floor(x + 1/2)": functools.partial(R.crop_window_ref, rounder=_floor_half),
    "radius from the u column": functools.partial(R.crop_window_ref, radius_column=0),
    "160 / (right - left + 1)": functools.partial(R.crop_window_ref, size_plus_one=True),
}
WRONG_ERODE = {
    "out-of-frame taps counted": functools.partial(R.erode_ref, count_outside=True),
    ">= for the ratio": functools.partial(R.erode_ref, strict=False),
    "radius 1": functools.partial(R.erode_ref, radius=1),
}
WRONG_BILATERAL = {
    "mean over invalid taps too": functools.partial(R.bilateral_ref, mean_over_all=True),
    "sigma_D = 1": functools.partial(R.bilateral_ref, sigma_d=1.0),
}
WRONG_SAMPLER = {
    "lower median": functools.partial(R.guess_translation_ref, lower_median=True),
    "integer box centre": functools.partial(R.guess_translation_ref, int_centre=True),
    "mask == 255": functools.partial(R.guess_translation_ref, mask_rule=lambda m: m == 255),
    "> at min_depth": functools.partial(R.guess_translation_ref, strict_min=True),
}
WRONG_POSE_UPDATE = {
    "Rd instead of Rd^T": functools.partial(R.pose_update_ref, transpose=False),
    "right-multiplication": functools.partial(R.pose_update_ref, left=False),
    "translation scaled by the diameter": functools.partial(R.pose_update_ref, trans_scale=1.0),
    "no tanh": functools.partial(R.pose_update_ref, use_tanh=False),
}


def _last_max(s):
    s = np.asarray(s, np.float32).ravel()
    if np.isnan(s).any():
        raise ValueError
    return int(np.flatnonzero(s == s.max())[-1])


def _nan_ignored(s):
    s = np.asarray(s, np.float32).ravel()
    if np.isnan(s).all():
        return 0
    return int(np.flatnonzero(s == np.nanmax(s))[0])


def window_control_differs(rule, poses, K, ratio, diameter):
    a, b = R.crop_window_ref(poses, K, ratio, diameter), WRONG_WINDOWS[rule](poses, K, ratio, diameter)
    return not (np.array_equal(a["edges"], b["edges"]) and np.allclose(a["tf"], b["tf"], rtol=1e-9, atol=0))


def test_wrong_window_rules_fail():
    hit = {r: 0 for r in WRONG_WINDOWS}
    sets = [(PC.hand_poses(), PC.HAND_K, PC.HAND_RATIO, PC.HAND_DIAMETER, False)]
    for seed in range(12):
        mesh, K, poses, _ = PC.sweep_poses(seed)
        sets += [(poses, K, ratio, mesh.diameter, True) for ratio in PC.RATIOS]
    for poses, K, ratio, diam, exempt in sets:
        tf = fo.crop_window_tf(syn.to_colmajor(poses), K, ratio, diam)
        bb = fo.bbox2d(tf)
        for rule, fn in WRONG_WINDOWS.items():
            if window_control_differs(rule, poses, K, ratio, diam):
                hit[rule] += 1
                with pytest.raises(AssertionError, match="window edges off|tf / bbox off"):
                    check_window(tf, bb, poses, K, ratio, diam, exempt_ties=exempt, ref_fn=fn)
    assert hit["half-even rounding"] >= 1 and hit["floor(x + 1/2)"] >= 1, hit          # (exact ties exist in the hand-made windows only)
    assert hit["radius from the u column"] == 24 and hit["160 / (right - left + 1)"] == 25, hit


@pytest.mark.parametrize("name", PC.CPU_FRAMES)
def test_wrong_filter_rules_fail(name):
    depth, mask, K = _small(name)
    e = fo.erode_depth(depth)
    b = fo.bilateral_filter_depth(e)
    check_erode(e, depth)
    check_bilateral(b, e)
    right = R.erode_ref(depth)
    for rule, fn in WRONG_ERODE.items():
        if not np.array_equal(fn(depth), right):
            with pytest.raises(AssertionError, match="erode differs"):
                check_erode(e, depth, ref_fn=fn)
        else:
            assert rule == ">= for the ratio", (rule, name)      # the two others differ on every frame; an exact 0.8 needs the hand frames below
    for rule, fn in WRONG_BILATERAL.items():
        with pytest.raises(AssertionError, match="bilateral"):
            check_bilateral(b, e, ref_fn=fn)


def test_median_of_the_unfiltered_depth_fails():
    """the sampler's values are the FILTERED depth: a reference fed the unfiltered frame fails wherever its median differs"""
    hit = 0
    for name in PC.CPU_FRAMES:
        f = PC.frame(name)
        _, b = oracle_filters(name)
        got = fo.guess_translation(b, f.mask, f.K)
        st, _, zc, _ = R.guess_translation_ref(f.depth, f.mask, f.K)
        if got is not None and (st != R.ST_OK or zc != R.guess_translation_ref(b, f.mask, f.K)[2]):
            hit += 1
            with pytest.raises(AssertionError, match="translation"):
                check_translation(got, f.depth, f.mask, f.K)
    assert hit >= 12, hit


def test_wrong_erode_ratio_rule_fails_on_exact_ratios():
    for hw, centre, nbad in (((9, 9), (4, 4), 20), ((9, 9), (4, 0), 12), ((1, 7), (0, 3), 4)):
        f = np.full(hw, 0.5, np.float32)
        cy, cx = centre
        taps = [(y, x) for y in range(cy - 2, cy + 3) for x in range(cx - 2, cx + 3) if 0 <= y < hw[0] and 0 <= x < hw[1] and (y, x) != centre]
        for y, x in taps[:nbad]:
            f[y, x] = 0.05
        e = fo.erode_depth(f)
        check_erode(e, f)
        assert e[centre] == np.float32(0.5)
        for rule in (">= for the ratio", "out-of-frame taps counted"):
            if not np.array_equal(WRONG_ERODE[rule](f), R.erode_ref(f)):
                with pytest.raises(AssertionError, match="erode differs"):
                    check_erode(e, f, ref_fn=WRONG_ERODE[rule])
        assert not np.array_equal(WRONG_ERODE[">= for the ratio"](f), R.erode_ref(f))


def test_wrong_sampler_rules_fail():
    hit = {r: 0 for r in WRONG_SAMPLER}
    Kid = np.eye(3, dtype=np.float32)
    for p in PC.sampler_patterns():
        got = fo.guess_translation(p.vals, p.mask, Kid, p.min_depth)
        right = R.guess_translation_ref(p.vals, p.mask, Kid, np.float32(p.min_depth))
        for rule, fn in WRONG_SAMPLER.items():
            wrong = fn(p.vals, p.mask, Kid, np.float32(p.min_depth))
            with np.errstate(invalid="ignore", over="ignore"):
                same = wrong[0] == right[0] and (wrong[0] != R.ST_OK or np.array_equal(wrong[1].astype(np.float32), right[1].astype(np.float32), equal_nan=True))
            if not same:
                hit[rule] += 1
                with pytest.raises(AssertionError, match="translation"):
                    check_translation_bits(got, p.vals, p.mask, p.min_depth, ref_fn=fn)
    assert all(n >= 3 for n in hit.values()), hit


def test_wrong_pose_update_and_argmax_rules_fail():
    poses, trans, rot = PC.pose_updates()
    out = syn.from_colmajor(fo.refine_post_process(syn.to_colmajor(poses), trans, rot, 0.1937))
    for rule, fn in WRONG_POSE_UPDATE.items():
        with pytest.raises(AssertionError, match="pose update off"):
            check_pose_update(out, poses, trans, rot, 0.1937, ref_fn=fn)
        # ... and row by row wherever the wrong rule moves an entry by more than the bound
        right, wrong = R.pose_update_ref(poses, trans, rot, 0.1937), fn(poses, trans, rot, 0.1937)
        rows = np.flatnonzero(np.abs(right - wrong).reshape(len(poses), -1).max(1) > 1e-4)
        assert len(rows) > 1500, (rule, len(rows))
        for i in rows[:50]:
            with pytest.raises(AssertionError, match="pose update off"):
                check_pose_update(out[i:i + 1], poses[i:i + 1], trans[i:i + 1], rot[i:i + 1], 0.1937, ref_fn=fn)
    hit = 0
    for name, s in PC.argmax_cases():
        if _last_max(s) != R.argmax_ref(s):
            hit += 1
            with pytest.raises(AssertionError, match="arg-max"):
                check_argmax(fo.argmax(s), s, ref_fn=_last_max)
    assert hit >= 30, hit
    # NaN ignored: the rule's outcome is an error, the wrong rule's an index -- an outcome that follows the rule fails against the wrong
    # rule on every NaN case, and the oracle's index (it has no error path) fails against the rule
    for name, s in PC.argmax_nan_cases():
        assert argmax_outcome(R.argmax_ref, s) == ARGMAX_ERROR and argmax_outcome(_nan_ignored, s) != ARGMAX_ERROR
        check_argmax(ARGMAX_ERROR, s)
        with pytest.raises(AssertionError, match="arg-max"):
            check_argmax(ARGMAX_ERROR, s, ref_fn=_nan_ignored)
        with pytest.raises(AssertionError, match="arg-max"):
            check_argmax(fo.argmax(s), s)
