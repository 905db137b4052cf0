"""The float64 references of tests/shade_warp_ref.py held to hand-derived answers, and the CPU oracle (oracle/fp_oracle.c) held to them.

The oracle and the kernels restate the reference's float expressions by one hand, so a mistake in a shared rule is made twice and their
2e-6 agreement cannot see it.  Here the render + crop stage is compared with references that share no expression with either; the
bounds are derived from the f32 arithmetic the stage is allowed, not from what the code gives, and every
comparison has a deliberately wrong twin that must fail it.  tests/test_shade_warp_gpu.py imports the cases, bounds, exemptions and
caps of this module and applies them to the device's outputs unchanged."""
import dataclasses
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

import shade_warp_ref as ref
from foundationpose_cpp_amd import synthetic as syn
from geometry_cases import random_case
from oracle import fp_oracle as fo

U = 2.0 ** -24                 # unit roundoff of f32

# measured on the oracle over CPU_CASES in both float models (test_measured_constants_have_their_margin re-measures them), margin 2:
ETA = 6.0e-4                   # px: equivalent sample-position error of the rasteriser's barycentrics and z/w
ETA_W = 1.4e-4                 # px: equivalent source-position error of the warp's bilinear value
assert ETA < 0.1               # (at 0.1 px the half-pixel control would fail by less than a factor of 2.5 after the margin)

HALF = 0.5                     # a peak above half of a derived bound means the derivation is wrong
CUT_CAP = 1e-3                 # share of foreground within the xyz bound of the 4.0 cut, per image
BARY_CAP = 0.05                # share of foreground whose float64 barycentrics leave [0, 1] (the rasteriser clamps there), per image
RGB_STEP_CAP = 0.01            # share of warped rgb values one u8 step off, per case
RGB_STEP_CAP_SMOOTH = 5e-4     # ... on a smooth frame
TIE_WINDOW = 2.0 ** -10        # nearest tap: source coordinate + 0.5 this close to an integer may take either tap
WARP_XYZ_CAP = 0.02            # share of warped pixels exempted (tap ties + the 4.0 cut), per image


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    mesh: syn.Mesh
    K: np.ndarray
    rgb: np.ndarray
    depth: np.ndarray
    poses: np.ndarray             # [N, 4, 4] f32
    hw: tuple
    ratios: tuple = (1.2, 1.1)
    smooth: bool = False


def _rot(ax_deg, ay_deg, az_deg):
    a, b, c = np.deg2rad([ax_deg, ay_deg, az_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def wrapped_quad(tex, half=0.06, uv_scale=(3.7, 2.3), uv_offset=(-1.6, -1.2)):
    """a square whose texture coordinates span several wraps of a non-square texture; normals differ per corner so that the Lambert term
    is really interpolated"""
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float32)
    n = np.array([[0.2, 0.1, -1], [-0.3, 0.1, -1], [0.1, -0.4, -1], [0, 0, -1]], np.float32)
    uv = (np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64) * uv_scale + uv_offset).astype(np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return syn.Mesh("wquad", v, n, uv, f, tex, diameter=0.2, center=np.zeros(3, np.float32))


def _smooth_frame(h, w, seed):
    """a low-passed image: noise at 1/16 resolution, bilinearly enlarged"""
    rng = np.random.default_rng(seed)
    small = rng.uniform(0, 255, (h // 16 + 2, w // 16 + 2, 3))
    y, x = np.arange(h) / 16.0, np.arange(w) / 16.0
    y0, x0 = y.astype(int), x.astype(int)
    ay, ax = (y - y0)[:, None, None], (x - x0)[None, :, None]
    img = ((small[y0][:, x0] * (1 - ax) + small[y0][:, x0 + 1] * ax) * (1 - ay)
           + (small[y0 + 1][:, x0] * (1 - ax) + small[y0 + 1][:, x0 + 1] * ax) * ay)
    return np.rint(img).astype(np.uint8)


CPU_CASES = [f"rnd{i}" for i in range(12)] + ["ellipsoid", "wquad"]      # the list the constants are measured on and every control must fail on
EXTRA_CASES = ["tex1xN", "texNx1", "tex1024x3", "edge", "smooth"]      # textures no other test renders, the edge poses, a smooth frame
ALL_CASES = CPU_CASES + EXTRA_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("rnd"):
        mesh, K, rgb, depth, poses, hw = random_case(int(name[3:]))
        return Case(name, mesh, K, rgb, depth, poses, hw)
    if name.startswith("tex"):                               # the mesh, frame and poses of rnd1 under another texture
        mesh, K, rgb, depth, poses, hw = random_case(1)
        shape = {"tex1xN": (1, 53), "texNx1": (47, 1), "tex1024x3": (3, 1024)}[name]
        tex = np.random.default_rng(77).integers(0, 256, shape + (3,), dtype=np.uint8)
        return Case(name, dataclasses.replace(mesh, name=name, texture=tex), K, rgb, depth, poses, hw)
    scene_mesh = syn.make_mesh()
    scene = syn.make_scene(scene_mesh)
    if name == "ellipsoid":                                  # the 512 x 512 texture at four rotations
        poses = np.stack([syn.pose_matrix(syn.random_rotation(i), (0.02, -0.01, 0.7)) for i in range(4)])
        return Case(name, scene_mesh, scene.K, scene.rgb, scene.depth, poses, (480, 640))
    if name == "wquad":
        tex = np.random.default_rng(5).integers(0, 256, (37, 23, 3), dtype=np.uint8)
        poses = np.stack([syn.pose_matrix(_rot(*a), (0.03, -0.02, 0.6)) for a in [(35, -40, 20), (-50, 25, 70), (10, 48, -130)]])
        return Case(name, wrapped_quad(tex), scene.K, scene.rgb, scene.depth, poses, (480, 640))
    if name == "edge":                                       # partly outside the frame, crossing the near plane, 5 m away
        R = syn.random_rotation(11)
        poses = np.stack([syn.pose_matrix(R, t) for t in [(0.45, 0.3, 0.7), (0.0, 0.0, 0.12), (0.0, 0.0, 0.05), (0.3, -0.2, 5.0), (-0.6, 0.0, 0.7)]])
        return Case(name, scene_mesh, scene.K, scene.rgb, scene.depth, poses, (480, 640), ratios=(1.2,))
    if name == "smooth":
        poses = np.stack([syn.pose_matrix(syn.random_rotation(i), t) for i, t in enumerate([(0.02, -0.01, 0.7), (-0.2, 0.1, 0.45), (0.3, 0.2, 1.3)])])
        return Case(name, scene_mesh, scene.K, _smooth_frame(480, 640, 9), scene.depth, poses, (480, 640), smooth=True)
    raise KeyError(name)


def window_tf(c, ratio, poses=None):
    """[N, 9] f32 crop windows (ComputeCropWindowTF; the oracle's, pinned to the float64 rule crop_window_ref of tests/pose_rules_ref.py by
    tests/test_pose_rules_ref_cpu.py and, for the device's PoseRec, tests/test_pose_rules_gpu.py: DESIGN.md section 2.2)"""
    return fo.crop_window_tf(syn.to_colmajor(c.poses if poses is None else poses), c.K, ratio, c.mesh.diameter)


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, ratio, fmad=True):
    c = case(name)
    p16 = syn.to_colmajor(c.poses)
    fo.set_fmad(fmad)
    try:
        out, tri, rast = fo.render(fo.OracleMesh(c.mesh), p16, c.K, c.hw, ratio, debug=True)
    finally:
        fo.set_fmad(True)
    return dict(render=out, tri=tri, rast=rast)


def _tie_lines(tf):
    """number of crop columns + rows whose nearest tap is a tie (source coordinate + 0.5 within TIE_WINDOW of an integer)"""
    return sum(int((np.abs(s + 0.5 - np.rint(s + 0.5)) <= TIE_WINDOW).sum()) for s in ref.warp_source(tf))


@functools.lru_cache(maxsize=None)
def warp_poses(name, ratio):
    """the poses of a case for the warp comparison.  A window of integer size w reads column x at left + x w / 160, which is an exact
    k + 1/2 for gcd(w, 160) columns unless gcd(w, 160) is 32 or 160: most even sizes make ties systematic (2 columns + 2 rows are already
    2.5 % of the crop).  Such a pose is swapped for the same pose 0.2 %, 0.4 %, ... further away, the first whose window has at most three
    tie lines (1.9 %), so that the cap on exempted pixels stays what it is.  The smooth frame takes windows with NO tie line (sizes 32, 96,
    160, 224, ...): on a tie row the bilinear value of a smooth image is itself an exact k + 1/2 wherever the two rows differ by an odd
    step, which is a property of the window size and not of the warp's arithmetic."""
    c = case(name)
    out = []
    for pose in c.poses:
        for k in range(2000):
            q = pose.copy()
            q[:3, 3] = pose[:3, 3] * np.float32(1.0 + 0.002 * k)
            if _tie_lines(fo.crop_window_tf(syn.to_colmajor(q[None]), c.K, ratio, c.mesh.diameter)[0]) <= (0 if c.smooth else 3):
                break
        else:
            raise AssertionError(f"{name}: no pose without systematic ties")
        out.append(q)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def oracle_crop(name, ratio):
    c = case(name)
    return fo.crop(c.rgb, c.depth, c.K, syn.to_colmajor(warp_poses(name, ratio)), ratio, c.mesh.diameter)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def colour_bound(mesh):
    """|got - ref| of a shaded colour: the uv interpolation costs ~3 roundings at magnitude |uv|max, the scale by the
    texture size and the - 0.5 about one more -> 4 (|uv|max + 1) u of a texture size in texels; one texel of error moves the colour by at
    most one texel difference (<= 1) per axis; the lerps and the shade add a constant; the shade factor is <= 1.3"""
    th, tw = mesh.texture.shape[:2]
    uvmax = np.abs(ref.vertex_uv(mesh)).max()
    return (4.0 * (uvmax + 1.0) * (tw + th) + 16.0) * 1.3 * U


def xyz_bound(pmax, tmax, radius):
    """|got - ref| of a normalised coordinate: ~8 roundings (f32 vertex transform or back-projection, interpolation, - t, / radius) of values
    <= |p|max + |t|max"""
    return 8.0 * U * (pmax + tmax) / radius


# ---- comparison 1: a render tensor against shade_ref fed the rasteriser's own output ---------------------------------------------------
def check_shade(got, mesh, pose, rast, sample=ref.texture_ref):
    """one image.  Every foreground pixel is checked, none exempted (xyz: a component whose float64 value lies within the bound of the 4.0
    cut may be zero on either side).  -> dict(nfg, colour, xyz, cut): peaks as fractions of their bounds, cut = exempted share"""
    want, d = ref.shade_ref(mesh, pose, rast, sample, details=True)
    fg = d["fg"]
    got = np.asarray(got, np.float64)
    assert (got[~fg] == 0).all(), "background must be zero"
    if not fg.any():
        return dict(nfg=0, colour=0.0, xyz=0.0, cut=0.0)
    cb = colour_bound(mesh)
    ce = np.abs(got[..., :3] - want[..., :3])[fg].max()
    assert ce <= cb, f"colour off by {ce:.3e}, bound {cb:.3e}"
    t = np.abs(np.asarray(pose, np.float64)[:3, 3]).max()
    xb = xyz_bound(np.abs(d["p"][fg]).max(), t, ref.radius_of(mesh))
    near = fg[..., None] & (np.abs(np.abs(d["q"]) - ref.MAX_XYZ) <= xb)
    g, w = got[..., 3:], want[..., 3:]
    err = np.abs(g - w)
    ok = (err <= xb) | (near & ((g == 0) | (np.abs(g - d["q"]) <= xb)))
    assert ok[fg].all(), f"xyz off by {err[fg & ~ok.all(-1)].max():.3e}, bound {xb:.3e}"
    cut = near.any(-1).sum() / fg.sum()
    assert cut <= CUT_CAP, f"{cut:.2%} of the foreground within the bound of the 4.0 cut"
    strict = fg[..., None] & ~near
    return dict(nfg=int(fg.sum()), colour=ce / cb, xyz=(err[strict].max() / xb if strict.any() else 0.0), cut=cut)


def _merge(rows, sums=("nfg", "n", "steps", "lit", "valid")):
    """counts add up, peaks and shares take their maximum over the images of a case"""
    return {k: (sum if k in sums else max)(r[k] for r in rows) for k in rows[0]}


def check_case_shade(c, render, rast, sample=ref.texture_ref):
    s = _merge([check_shade(render[n], c.mesh, c.poses[n], rast[n], sample) for n in range(len(c.poses))])
    assert s["nfg"] > 0, "nothing compared"
    return s


# ---- comparison 2: the rasteriser's output against bary_ref ---------------------------------------------------------------------------
def bary_residual(mesh, pose, K, tf, rast):
    """-> (err, grad, inside): |rast - bary_ref| and |d/dx| + |d/dy| of bary_ref over one pixel, [160, 160, 3] for (b0, b1, z/w), and the mask
    of foreground pixels whose float64 barycentrics b0, b1 lie in [0, 1] (elsewhere the rasteriser clamps by rule)"""
    tid = np.asarray(rast[..., 3]).astype(np.int64)
    b = ref.bary_ref(mesh, pose, K, tf, tid)
    gx = ref.bary_ref(mesh, pose, K, tf, tid, (1.0, 0.5)) - ref.bary_ref(mesh, pose, K, tf, tid, (0.0, 0.5))
    gy = ref.bary_ref(mesh, pose, K, tf, tid, (0.5, 1.0)) - ref.bary_ref(mesh, pose, K, tf, tid, (0.5, 0.0))
    with np.errstate(invalid="ignore"):
        inside = (tid > 0) & (b[..., :2] >= 0).all(-1) & (b[..., :2] <= 1).all(-1) & np.isfinite(gx).all(-1) & np.isfinite(gy).all(-1)
    return np.abs(np.asarray(rast[..., :3], np.float64) - b), np.abs(gx) + np.abs(gy), inside


def check_bary(mesh, pose, K, tf, rast, tri=None, eta=ETA, offset=(0.5, 0.5)):
    """one image: |b - b_ref| <= eta (|db/dx| + |db/dy|) + 1e-6 for b0, b1 and z/w at every pixel where bary_ref lies in [0, 1]; the others are
    at most BARY_CAP of the foreground.  `offset` moves the reference's sample point (the half-pixel control).
    -> dict(nfg, eta = the measured equivalent position error as a fraction of `eta`, clamped = exempted share)"""
    if tri is not None:
        assert (np.asarray(rast[..., 3]).astype(np.int64) == tri).all(), "rast id != triangle-id buffer"
    nfg = int((rast[..., 3] > 0).sum())
    if nfg == 0:
        return dict(nfg=0, eta=0.0, clamped=0.0)
    if tuple(offset) != (0.5, 0.5):
        tid = np.asarray(rast[..., 3]).astype(np.int64)
        _, grad, inside = bary_residual(mesh, pose, K, tf, rast)
        with np.errstate(invalid="ignore"):
            err = np.abs(np.asarray(rast[..., :3], np.float64) - ref.bary_ref(mesh, pose, K, tf, tid, offset))
    else:
        err, grad, inside = bary_residual(mesh, pose, K, tf, rast)
    clamped = 1.0 - inside.sum() / nfg
    assert clamped <= BARY_CAP, f"{clamped:.2%} of the foreground has float64 barycentrics outside [0, 1]"
    assert inside.any(), "nothing compared"
    e, g = err[inside], grad[inside]
    bad = e > eta * g + 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(e > 1e-6, (e - 1e-6) / g, 0.0).max()
    assert not bad.any(), f"{bad.sum()} values off; equivalent sample-position error {need:.4f} px, allowed {eta} px"
    return dict(nfg=nfg, eta=need / eta, clamped=clamped)


def check_case_bary(c, ratio, rast, tri=None, eta=ETA, offset=(0.5, 0.5)):
    tf = window_tf(c, ratio)
    s = _merge([check_bary(c.mesh, c.poses[n], c.K, tf[n], rast[n], None if tri is None else tri[n], eta, offset) for n in range(len(c.poses))])
    assert s["nfg"] > 0, "nothing compared"
    return s


# ---- comparison 3: an observed crop against warp_ref ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warp_reference(name, ratio):
    """per pose: the reference tensor and what the exemptions need (computed once, shared by every test and both float models)"""
    c = case(name)
    out = []
    for pose, tf in zip(warp_poses(name, ratio), window_tf(c, ratio, warp_poses(name, ratio))):
        sx, sy = ref.warp_source(tf)
        taps, ax, ay = ref.bilinear_taps(c.rgb, sx, sy)
        val = ref.bilinear_value(taps, ax, ay)
        xyz, d = ref.nearest_xyz(c.depth, c.K, pose, c.mesh.diameter, np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64),
                                 details=True)
        fx, fy = sx + 0.5 - np.floor(sx + 0.5), sy + 0.5 - np.floor(sy + 0.5)
        tie = (np.minimum(fy, 1 - fy) <= TIE_WINDOW)[:, None] | (np.minimum(fx, 1 - fx) <= TIE_WINDOW)[None, :]
        # what a tie pixel may hold instead: the tap on either side of the tie, per axis
        sides = [ref.nearest_xyz(c.depth, c.K, pose, c.mesh.diameter, np.floor(sx + 0.5 + dx).astype(np.int64), np.floor(sy + 0.5 + dy).astype(np.int64))
                 for dx in (-TIE_WINDOW, TIE_WINDOW) for dy in (-TIE_WINDOW, TIE_WINDOW)]
        out.append(dict(val=val, spread=ref.tap_spread(taps), xyz=xyz, tie=tie, sides=sides, **d))
    return out


def check_warp(got, w, pose, radius, eta_w=ETA_W):
    """one image against its _warp_reference record.  rgb: a value differs by exactly one u8 step or not at all, and only where the float64
    pre-rounding value lies within eta_w * spread + 1e-3 of the tie between the two.  xyz: within the bound, except nearest-tap ties (which must
    hold the tap of one side or the other) and components within the bound of the 4.0 cut (at most WARP_XYZ_CAP of the image).
    -> dict(n = rgb values compared, steps = values one step off, eta_w = the measured equivalent position error as a fraction of eta_w,
            xyz = peak / bound, exempt = exempted share)"""
    got = np.asarray(got, np.float64)
    k = got[..., :3] * 255.0
    assert np.abs(k - np.rint(k)).max() < 1e-4, "rgb is not k / 255"
    k = np.rint(k)
    kref = np.clip(np.rint(w["val"]), 0, 255)
    step = k - kref
    assert np.abs(step).max() <= 1, f"rgb off by {np.abs(step).max():.0f} u8 steps"
    off = step != 0
    dist = np.abs(w["val"] - (np.minimum(k, kref) + 0.5))[off]
    need = np.maximum(dist - 1e-3, 0.0) / np.maximum(w["spread"][off], 1e-300)
    bad = dist > eta_w * w["spread"][off] + 1e-3
    assert not bad.any(), f"{bad.sum()} rgb values a step off although {dist[bad].max():.4f} from the tie (equivalent position error {need.max():.2e} px, allowed {eta_w:.1e})"
    t = np.abs(np.asarray(pose, np.float64)[:3, 3]).max()
    xb = xyz_bound(np.abs(w["p"]).max(-1, keepdims=True), t, radius)
    near = w["valid"][..., None] & (np.abs(np.abs(w["q"]) - ref.MAX_XYZ) <= xb)
    exempt = w["tie"] | near.any(-1)
    err = np.abs(got[..., 3:] - w["xyz"])
    strict = ~exempt
    frac = (err / xb)[strict].max() if strict.any() else 0.0
    assert frac <= 1.0, f"warped xyz off by {frac:.2f} of its bound"
    either = np.min([np.abs(got[..., 3:] - side).max(-1) for side in w["sides"]], 0)       # exempt from the bound above, not from this
    loose = w["tie"] & ~near.any(-1)
    assert (either[loose] <= xb[..., 0][loose]).all(), "a nearest-tap tie holds neither of its two taps"
    share = exempt.mean()
    assert share <= WARP_XYZ_CAP, f"{share:.2%} of the crop exempted (ties {w['tie'].mean():.2%})"
    return dict(n=int(k.size), steps=int(off.sum()), eta_w=(need.max() / eta_w if off.any() else 0.0), xyz=frac, exempt=share,
                lit=int((kref > 0).sum()), valid=int(w["valid"].sum()))


def check_case_warp(c, ratio, crop, eta_w=ETA_W):
    """crop [N, 160, 160, 6]: the observed crops at warp_poses(c.name, ratio)"""
    recs, poses = _warp_reference(c.name, ratio), warp_poses(c.name, ratio)
    rows = [check_warp(crop[n], recs[n], poses[n], ref.radius_of(c.mesh), eta_w) for n in range(len(poses))]
    s = _merge(rows)
    assert s["lit"] > 0 and s["valid"] > 0, "nothing compared"
    cap = RGB_STEP_CAP_SMOOTH if c.smooth else RGB_STEP_CAP
    s["share"] = s["steps"] / s["n"]
    assert s["share"] <= cap, f"{s['share']:.3%} of the rgb values one step off (cap {cap:.2%})"
    return s


def print_row(kind, name, ratio, s, extra=""):
    cols = " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in s.items())
    print(f"  {kind:5s} {name:10s} ratio {ratio} {extra}: {cols}")


# ---- hand cases: texture_ref ------------------------------------------------------------------------------------------------------------
def _texels(th, tw):
    """distinct texels: texel (row r, column c) = (10 + 40 r + 7 c, 200 - 30 r - 11 c, 3 + 90 c + r)"""
    r, c = np.mgrid[0:th, 0:tw]
    return np.stack([10 + 40 * r + 7 * c, 200 - 30 * r - 11 * c, 3 + 90 * c + r], -1).astype(np.uint8)


def _fr(tex, *terms):
    """sum of weight * texel over (weight, row, column) terms, as exact fractions of 255 per channel"""
    return [float(sum(Fr(w) * int(tex[r, c, ch]) for w, r, c in terms) / 255) for ch in range(3)]


def test_texture_ref_hand_cases_2x2():
    tex = _texels(2, 2)
    T = lambda u, v: ref.texture_ref(tex, u, v)
    q, h = Fr(1, 4), Fr(1, 2)
    # texel centres: column c at u = (c + 1/2) / 2, row r at v = (r + 1/2) / 2
    for r in range(2):
        for c in range(2):
            np.testing.assert_allclose(T((c + 0.5) / 2, (r + 0.5) / 2), _fr(tex, (1, r, c)), rtol=0, atol=1e-15)
    # edge midpoints: between the two columns of row 0 (u = 1/2, v = 1/4), between the two rows of column 1 (u = 3/4, v = 1/2)
    np.testing.assert_allclose(T(0.5, 0.25), _fr(tex, (h, 0, 0), (h, 0, 1)), atol=1e-15)
    np.testing.assert_allclose(T(0.75, 0.5), _fr(tex, (h, 0, 1), (h, 1, 1)), atol=1e-15)
    # the corner where all four texels meet
    np.testing.assert_allclose(T(0.5, 0.5), _fr(tex, (q, 0, 0), (q, 0, 1), (q, 1, 0), (q, 1, 1)), atol=1e-15)
    # the wrap seam: u = 0 lies half way between the LAST column and the first (x = -1/2); so does every integer u, and u just below 1
    seam = _fr(tex, (h, 0, 1), (h, 0, 0))
    for u in (0.0, 1.0, -3.0, 1 - 2.0 ** -40):
        np.testing.assert_allclose(T(u, 0.25), seam, atol=1e-10)
    # negative u: frac(-0.25) = 0.75 (column 1's centre); u = 2.25 = column 0's centre; v wraps the same way
    np.testing.assert_allclose(T(-0.25, 0.25), _fr(tex, (1, 0, 1)), atol=1e-15)
    np.testing.assert_allclose(T(2.25, 0.25), _fr(tex, (1, 0, 0)), atol=1e-15)
    np.testing.assert_allclose(T(0.25, -1.25), _fr(tex, (1, 1, 0)), atol=1e-15)
    # x = u * 2 - 1/2 = -1/4 at u = 1/8: 1/4 of the last column + 3/4 of the first; v = 7/8: y = 5/4 -> 3/4 row 1 + 1/4 row 0 (wrapped)
    np.testing.assert_allclose(T(0.125, 0.875), _fr(tex, (Fr(3, 16), 1, 1), (Fr(9, 16), 1, 0), (Fr(1, 16), 0, 1), (Fr(3, 16), 0, 0)), atol=1e-15)


def test_texture_ref_hand_cases_3x2():
    """TH = 2 rows, TW = 3 columns: u scales by 3, v by 2 (the other order reads other texels)"""
    tex = _texels(2, 3)
    T = lambda u, v: ref.texture_ref(tex, u, v)
    q, h = Fr(1, 4), Fr(1, 2)
    for r in range(2):
        for c in range(3):
            np.testing.assert_allclose(T((c + 0.5) / 3, (r + 0.5) / 2), _fr(tex, (1, r, c)), rtol=0, atol=1e-15)
    np.testing.assert_allclose(T(2 / 3, 0.25), _fr(tex, (h, 0, 1), (h, 0, 2)), atol=1e-15)                 # edge between columns 1 and 2
    np.testing.assert_allclose(T(0.5, 0.5), _fr(tex, (h, 0, 1), (h, 1, 1)), atol=1e-15)                    # edge between the rows of column 1
    np.testing.assert_allclose(T(1 / 3, 0.5), _fr(tex, (q, 0, 0), (q, 0, 1), (q, 1, 0), (q, 1, 1)), atol=1e-15)   # a four-texel corner
    for u in (0.0, -2.0, 1 - 2.0 ** -40):                                                                  # the seam joins columns 2 and 0
        np.testing.assert_allclose(T(u, 0.75), _fr(tex, (h, 1, 2), (h, 1, 0)), atol=1e-10)
    np.testing.assert_allclose(T(-1 / 6, 0.25), _fr(tex, (1, 0, 2)), atol=1e-15)                           # frac(-1/6) = 5/6: column 2
    np.testing.assert_allclose(T(2.25, 0.25), _fr(tex, (Fr(3, 4), 0, 0), (q, 0, 1)), atol=1e-15)           # x = 3/4 - 1/2 = 1/4
    np.testing.assert_allclose(T(0.5, 1.0), _fr(tex, (h, 1, 1), (h, 0, 1)), atol=1e-15)                    # the v seam joins rows 1 and 0
    # vectorised calls broadcast
    assert ref.texture_ref(tex, np.zeros((4, 5)), 0.25).shape == (4, 5, 3)


# ---- hand cases: warp_ref ---------------------------------------------------------------------------------------------------------------
def _hand_warp(rgb, depth, t=(0.0, 0.0, 1.0), diameter=0.25, tf=(1, 0, -10.25, 0, 1, -20.5, 0, 0, 1)):
    """tf = shift by (-10.25, -20.5): crop pixel (x, y) reads the source at (x + 10.25, y + 20.5); the coefficients and the radius 0.125 are exact in f32"""
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = t
    K = np.array([[100, 0, 32], [0, 50, 24], [0, 0, 1]], np.float32)
    return ref.warp_ref(rgb, depth, K, pose, np.array(tf, np.float32), diameter), K


def test_warp_ref_hand_cases():
    rgb = np.zeros((48, 64, 3), np.uint8)
    depth = np.ones((48, 64), np.float32)
    # crop (0, 0) reads (10.25, 20.5): weights 3/4, 1/4 in x and 1/2, 1/2 in y between four known pixels
    rgb[20, 10], rgb[20, 11], rgb[21, 10], rgb[21, 11] = (8, 0, 1), (16, 0, 1), (40, 0, 2), (80, 4, 2)
    # channel 0: (3/4 8 + 1/4 16 + 3/4 40 + 1/4 80) / 2 = (10 + 50) / 2 = 30; channel 1: 4 / 8 = 0.5 -> tie, rounds to the EVEN 0;
    # channel 2: (1 + 2) / 2 = 1.5 -> tie, rounds to the EVEN 2 (truncation gives 1, round-half-up gives 1 for channel 1)
    out, K = _hand_warp(rgb, depth)
    np.testing.assert_allclose(out[0, 0, :3], [30 / 255, 0.0, 2 / 255], rtol=0, atol=1e-15)
    # the nearest tap of (10.25, 20.5) is column floor(10.75) = 10, row floor(21.0) = 21 -- a .5 goes UP
    depth[21, 10], depth[20, 10] = 0.75, 0.5
    out, K = _hand_warp(rgb, depth)
    np.testing.assert_allclose(out[0, 0, 3:], [(10 - 32) * 0.75 / 100 / 0.125, (21 - 24) * 0.75 / 50 / 0.125, (0.75 - 1.0) / 0.125], rtol=1e-15)
    # a tap half outside the frame: crop x = 53 reads x = 63.25, i.e. column 63 and the zero border
    rgb[20, 63], rgb[21, 63] = (100, 0, 0), (60, 0, 0)
    out, K = _hand_warp(rgb, depth)
    np.testing.assert_allclose(out[0, 53, 0], np.rint(0.75 * (100 + 60) / 2) / 255, atol=1e-15)            # 60 exactly
    assert out[0, 54, 0] == 0 and (out[0, 54, 3:] == 0).all()                                             # x = 64.25: outside, tap 64 invalid
    # ... and above the frame: tf shifting by +0.5 rows reads row -0.5 = half of row 0
    rgb[0, 10] = (200, 0, 0)
    out, K = _hand_warp(rgb, depth, tf=(1, 0, -10, 0, 1, 0.5, 0, 0, 1))
    np.testing.assert_allclose(out[0, 0, 0], 100 / 255, atol=1e-15)
    # an invalid depth zeroes the whole pixel; a valid 0.001 does not (its z - t_z = -9.99 falls to the 4.0 cut, x and y stay)
    depth[22, 10] = 0.0009
    depth[23, 10] = 0.001
    out, K = _hand_warp(rgb, depth)
    assert (out[1, 0, 3:] == 0).all()
    d = float(np.float32(0.001))
    np.testing.assert_allclose(out[2, 0, 3:], [(10 - 32) * d / 100 / 0.125, (23 - 24) * d / 50 / 0.125, 0.0], rtol=1e-15)
    # the 4.0 cut is per component: z - t_z just over 0.5 = 4.0 radii -> zero, x and y stay; exactly 4.0 stays
    depth[24, 10] = np.float32(1.5 + 1e-5)
    out, K = _hand_warp(rgb, depth)
    d = float(depth[24, 10])
    assert out[3, 0, 5] == 0 and (d - 1.0) / 0.125 > 4.0
    np.testing.assert_allclose(out[3, 0, 3:5], [(10 - 32) * d / 100 / 0.125, 0.0], rtol=1e-15)
    depth[25, 10] = 1.5                                                                                   # (1.5 - 1.0) / 0.12525 = 4.0 exactly
    out, K = _hand_warp(rgb, depth, diameter=0.25)
    assert out[4, 0, 5] == 4.0


def test_shade_ref_and_bary_ref_on_a_hand_triangle():
    """one triangle seen head-on at 1 m: bary_ref returns what plane geometry says, shade_ref what the shading rule says"""
    v = np.array([[-0.0625, -0.0625, 0], [0.0625, -0.0625, 0], [-0.0625, 0.0625, 0]], np.float32)
    n = np.array([[0, 0, -1], [0, 0.6, -0.8], [0, 0, 0]], np.float32)                 # diffuse 1, 0.8 and 0 (zero normal)
    uv = np.array([[0.25, 0.75], [0.75, 0.75], [0.25, 0.25]], np.float32)             # (u, 1 - v) = texel centres of a 2 x 2 texture
    tex = _texels(2, 2)
    mesh = syn.Mesh("tri", v, n, uv, np.array([[0, 1, 2]], np.int32), tex, diameter=0.25, center=np.zeros(3, np.float32))
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 1.0
    K = syn.intrinsics()
    tf = np.array([2, 0, -2 * 282, 0, 2, -2 * 202, 0, 0, 1], np.float32)       # window [282, 362) x [202, 282) at twice the size
    tid = np.zeros((160, 160), np.int64)
    tid[159 - 60, 70] = 1                                                      # output row 60 = raster row 99
    # sample point: (b0, b2) = (282, 282 + 159 / 2): u = 282 + 70.5 * 79.5 / 160, v = 202 + 60.5 * 79.5 / 160; on the plane z = 1
    X, Y = (282 + 70.5 * 79.5 / 160 - 320) / 320, (202 + 60.5 * 79.5 / 160 - 240) / 320
    b1, b2 = (X + 0.0625) / 0.125, (Y + 0.0625) / 0.125
    got = ref.bary_ref(mesh, pose, K, tf, tid)[159 - 60, 70]
    np.testing.assert_allclose(got, [1 - b1 - b2, b1, 100.1 / 99.9 - 20 / 99.9], rtol=1e-12)
    assert np.isnan(ref.bary_ref(mesh, pose, K, tf, tid)[0, 0]).all()
    rast = np.zeros((160, 160, 4), np.float32)
    rast[159 - 60, 70] = (0.5, 0.25, 0.8, 1)
    out = ref.shade_ref(mesh, pose, rast)
    assert (out[59] == 0).all() and (out[60, :70] == 0).all()
    # uv = 0.5 (0.25, 0.25) + 0.25 (0.75, 0.25) + 0.25 (0.25, 0.75) = (0.375, 0.375): x = y = 0.25 -> weights 9/16, 3/16, 3/16, 1/16
    texel = np.array(_fr(tex, (Fr(9, 16), 0, 0), (Fr(3, 16), 0, 1), (Fr(3, 16), 1, 0), (Fr(1, 16), 1, 1)))
    dif = 0.5 * 1.0 + 0.25 * 0.8 + 0.25 * 0.0
    np.testing.assert_allclose(out[60, 70, :3], np.clip(texel * (0.8 + 0.5 * dif), 0, 1), rtol=1e-7)       # (f32 0.6, 0.8)
    np.testing.assert_allclose(out[60, 70, 3:], [-0.03125 / 0.125, -0.03125 / 0.125, 0.0], rtol=1e-12, atol=1e-15)   # p = p0 / 2 + p1 / 4 + p2 / 4 = (-1/32, -1/32, 1)


# ---- the oracle against the references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmad", [True, False])
@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_render_matches_shade_ref(name, fmad):
    c = case(name)
    for ratio in c.ratios:
        o = oracle_outputs(name, ratio, fmad)
        s = check_case_shade(c, o["render"], o["rast"])
        print_row("shade", name, ratio, s, f"fmad={int(fmad)}")
        assert s["colour"] < HALF and s["xyz"] < HALF, "a peak above half of its bound: the derivation of the bound is wrong"


@pytest.mark.parametrize("fmad", [True, False])
@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_rast_matches_bary_ref(name, fmad):
    c = case(name)
    for ratio in c.ratios:
        o = oracle_outputs(name, ratio, fmad)
        s = check_case_bary(c, ratio, o["rast"], o["tri"])
        print_row("bary", name, ratio, s, f"fmad={int(fmad)}")


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_crop_matches_warp_ref(name):
    c = case(name)
    for ratio in c.ratios:
        s = check_case_warp(c, ratio, oracle_crop(name, ratio))
        print_row("warp", name, ratio, s)


def measure_constants(outputs=oracle_outputs, crops=oracle_crop, fmads=(True, False)):
    """(eta, eta_w) as the peak over CPU_CASES of what `outputs(name, ratio, fmad)` and `crops(name, ratio)` return: the checks run with loose constants and report
    the equivalent position errors they needed"""
    eta = eta_w = 0.0
    for name in CPU_CASES:
        c = case(name)
        for ratio in c.ratios:
            for fmad in fmads:
                eta = max(eta, check_case_bary(c, ratio, outputs(name, ratio, fmad)["rast"], eta=1.0)["eta"])
            eta_w = max(eta_w, check_case_warp(c, ratio, crops(name, ratio), eta_w=1.0)["eta_w"])
    return eta, eta_w


def test_measured_constants_have_their_margin():
    """ETA and ETA_W are the oracle's peaks over the case list times a margin of 2 (the kernels' expressions are the oracle's): re-measured
    here, so that neither a stale constant nor a generous one survives"""
    eta, eta_w = measure_constants()
    print(f"  oracle: eta {eta:.5f} px (ETA {ETA}), eta_w {eta_w:.3e} px (ETA_W {ETA_W:.1e})")
    assert 2.0 * eta <= ETA <= 2.5 * eta, (eta, ETA)
    assert 2.0 * eta_w <= ETA_W <= 2.5 * eta_w, (eta_w, ETA_W)


# ---- negative controls: each wrong rule must fail its assertion on every case -----------------------------------------------------------------
def _clamp_sampler(tex, u, v):
    """clamp-to-edge addressing instead of wrap"""
    th, tw = tex.shape[:2]
    t = tex.astype(np.float64) / 255.0
    x, y = np.clip(u, 0, 1) * tw - 0.5, np.clip(v, 0, 1) * th - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    cx, cy = lambda i: np.clip(i, 0, tw - 1), lambda i: np.clip(i, 0, th - 1)
    return ((t[cy(y0), cx(x0)] * (1 - ax) + t[cy(y0), cx(x0 + 1)] * ax) * (1 - ay)
            + (t[cy(y0 + 1), cx(x0)] * (1 - ax) + t[cy(y0 + 1), cx(x0 + 1)] * ax) * ay)


WRONG_SAMPLERS = {
    "no_v_flip": lambda tex, u, v: ref.texture_ref(tex, u, 1.0 - v),                      # (interpolating 1 - v and flipping after are the same)
    "texel_corner": lambda tex, u, v: ref.texture_ref(tex, u + 0.5 / tex.shape[1], v + 0.5 / tex.shape[0]),
    "bgr": lambda tex, u, v: ref.texture_ref(tex[..., ::-1], u, v),
    "th_tw_swapped": lambda tex, u, v: ref.texture_ref(tex.reshape(tex.shape[1], tex.shape[0], 3), u, v),
    "clamp": _clamp_sampler,
}
MEAN_FLOOR = {"no_v_flip": 0.07, "texel_corner": 0.035, "bgr": 0.10}       # the measured mean colour errors of the three, at least


def _applies(rule, c):
    th, tw = c.mesh.texture.shape[:2]
    if rule == "th_tw_swapped":
        return th != tw                                                     # a square texture reads the same either way
    if rule == "clamp":
        return np.abs(ref.vertex_uv(c.mesh) - 0.5).max() > 0.5              # within [0, 1] clamp and wrap differ only in the seam's half texel
    return True


@pytest.mark.parametrize("rule", list(WRONG_SAMPLERS))
@pytest.mark.parametrize("name", CPU_CASES)
def test_a_wrong_texture_rule_fails_the_colour_bound(name, rule):
    c = case(name)
    if not _applies(rule, c):
        assert name == "ellipsoid"                                          # (the only case with a square texture and uv within [0, 1])
        return
    for ratio in c.ratios:
        o = oracle_outputs(name, ratio)
        with pytest.raises(AssertionError, match="colour off"):
            check_case_shade(c, o["render"], o["rast"], WRONG_SAMPLERS[rule])
        if rule in MEAN_FLOOR:
            errs = []
            for n in range(len(c.poses)):
                want, d = ref.shade_ref(c.mesh, c.poses[n], o["rast"][n], WRONG_SAMPLERS[rule], details=True)
                errs.append(np.abs(o["render"][n][..., :3] - want[..., :3])[d["fg"]])
            mean = np.concatenate(errs).mean()
            assert mean >= MEAN_FLOOR[rule], (rule, mean)


@pytest.mark.parametrize("name", CPU_CASES)
def test_a_sample_point_without_the_half_pixel_fails_the_bary_bound(name):
    c = case(name)
    for ratio in c.ratios:
        o = oracle_outputs(name, ratio)
        with pytest.raises(AssertionError, match="values off"):
            check_case_bary(c, ratio, o["rast"], offset=(0.0, 0.0))


def _wrong_warp(c, ratio, rule):
    """the observed crops of a case under one wrong warp rule, built from the reference's own pieces"""
    out = []
    for pose, tf in zip(warp_poses(c.name, ratio), window_tf(c, ratio, warp_poses(c.name, ratio))):
        sx, sy = ref.warp_source(tf)
        taps, ax, ay = ref.bilinear_taps(c.rgb, sx, sy)
        if rule == "weights_swapped":
            ax, ay = 1 - ax, 1 - ay
        val = ref.bilinear_value(taps, ax, ay)
        col = np.clip(np.floor(val) if rule == "truncate" else np.rint(val), 0, 255) / 255.0
        cx, cy = (np.floor(sx), np.floor(sy)) if rule == "tap_floor" else (np.floor(sx + 0.5), np.floor(sy + 0.5))
        xyz = ref.nearest_xyz(c.depth, c.K, pose, c.mesh.diameter, cx.astype(np.int64), cy.astype(np.int64))
        out.append(np.concatenate([col, xyz], -1))
    return np.stack(out)


@pytest.mark.parametrize("rule,message", [("truncate", "rgb values a step off although|one step off"),
                                          ("tap_floor", "warped xyz off"),
                                          ("weights_swapped", "u8 steps|rgb values a step off although|one step off")])
@pytest.mark.parametrize("name", CPU_CASES)
def test_a_wrong_warp_rule_fails(name, rule, message):
    c = case(name)
    for ratio in c.ratios:
        assert check_case_warp(c, ratio, _wrong_warp(c, ratio, "none"))["steps"] == 0      # the builder itself is the reference
        with pytest.raises(AssertionError, match=message):
            check_case_warp(c, ratio, _wrong_warp(c, ratio, rule))
