"""tests/frame_render_ref.py (the numpy restatement of DESIGN.md section 4.8 that tests/test_frame_render_gpu.py holds fp_render_pose to)
against things it did not come from: the analytic ray-cast ellipsoid of synthetic.make_scene, and cases derived by hand."""
import numpy as np
import pytest

import frame_render_ref as FR
from foundationpose_cpp_amd import synthetic as syn

EPS = float(np.finfo(np.float32).eps)

# The share of analytic pixels the reference may miss.  The mesh is inscribed in the ellipsoid, so its silhouette lies inside the true
# one by at most the sagitta of a silhouette chord: with edges of ~4 degrees (icosphere, 4 subdivisions) that is r (1 - cos 2 deg) =
# 6e-4 r, a band of 2 * 6e-4 = 0.12 % of the area of a disc.  Snapping moves every vertex by up to 1/32 px per axis: a band of 1/32 px
# along the perimeter, 2 / (32 r_px) of the area -- 0.8 % at the smallest object here (r_px ~ 8 at 160x120), less at the others.  The sum
# stays under 1 %; the cap is twice that.  Measured with this reference: 640x480 0 of 1908 (0 %), 160x120 1 of 235 (0.43 %), 1280x720
# 6 of 7637 (0.08 %); no reference pixel outside the analytic mask in any of the three.
MISS_CAP = 0.02
SCENES = {"640x480": (640, 480, (0.02, -0.01, 0.70)), "160x120": (160, 120, (0.02, -0.01, 0.50)), "1280x720": (1280, 720, (0.02, -0.01, 0.70))}


def _analytic_depth(pose, K, H, W, dx=0.0, dy=0.0):
    """noise-free ray / ellipsoid depth at the image points (c + dx, r + dy): make_scene's ray-cast, restated (Scene.depth carries noise).
    -> (hit [H,W] bool, z [H,W] f64)"""
    R, t = np.asarray(pose, np.float64)[:3, :3], np.asarray(pose, np.float64)[:3, 3]
    K = np.asarray(K, np.float64)
    ax = np.array(syn.SEMI_AXES)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(xx + dx - K[0, 2]) / K[0, 0], (yy + dy - K[1, 2]) / K[1, 1], np.ones_like(xx)], -1) @ R
    o = R.T @ (-t)
    oo, dd = o / ax, d / ax
    A, B, C = (dd * dd).sum(-1), 2 * (dd * oo).sum(-1), (oo * oo).sum() - 1.0
    disc = B * B - 4 * A * C
    hit = disc > 0
    s = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0))) / (2 * A), 0.0)
    return hit & (s > 0), s


def _dilate(m):
    o = m.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            o[max(dy, 0):m.shape[0] + min(dy, 0), max(dx, 0):m.shape[1] + min(dx, 0)] |= m[max(-dy, 0):m.shape[0] + min(-dy, 0), max(-dx, 0):m.shape[1] + min(-dx, 0)]
    return o


@pytest.fixture(scope="module")
def rendered(syn_mesh):
    """the reference's rendering of each scene at its ground-truth pose, computed once"""
    out = {}
    for name, (W, H, t) in SCENES.items():
        sc = syn.make_scene(syn_mesh, W=W, H=H, t=t)
        out[name] = (sc, FR.render(FR.centred(syn_mesh), syn_mesh.faces, sc.gt_pose, sc.K, sc.rgb, sc.depth))
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_silhouette_against_the_analytic_ellipsoid(rendered, syn_mesh, name):
    sc, out = rendered[name]
    hit = sc.mask > 0                                    # the analytic mask (a ray-cast, no rasteriser)
    model = out["model_mask"] > 0
    assert set(np.unique(out["model_mask"])) <= {0, 255}
    assert not (model & ~_dilate(hit)).any()             # inscribed + at most one pixel of snapping
    missing = (hit & ~model).sum() / hit.sum()
    print(f"{name}: reference {model.sum()} px, analytic {hit.sum()} px, outside {(model & ~hit).sum()}, missing share {missing:.4%}")
    assert missing < MISS_CAP
    assert np.array_equal(out["tri_id"] > 0, model) and np.array_equal(out["model_depth"] > 0, model)
    assert out["tri_id"].max() <= len(syn_mesh.faces)


@pytest.mark.parametrize("name", list(SCENES))
def test_depth_is_behind_the_analytic_surface(rendered, name):
    """An inscribed surface lies behind the true one along every ray.  The reference interpolates the depth at barycentrics taken from
    SNAPPED vertices, so the point Q it evaluates -- a convex combination of the triangle's corners, hence inside the ellipsoid -- lies
    on a ray up to h = 1/32 px (the snap) + 1/1024 px (f32 rounding of the projection, ~8 ulp of 1280) per axis beside the pixel's own:
    z_ref >= z_true(ray of Q).  1 / z_true is a concave function g of the image point (the ellipsoid stays convex in (x/z, y/z, 1/z)), so
    g(c + d) <= g(c) + max(0, g(c) - g(c -+ h e_x)) + max(0, g(c) - g(c -+ h e_y)) for |d| <= h per axis (one-sided secants of a concave
    function bound its slope).  The margin on top is 16 eps z: the ~10 roundings of the vertex transform, the three quotients, the sum and
    the reciprocal.  Pixels with a neighbouring ray that misses the ellipsoid (the silhouette itself) have no such bound and are left out."""
    sc, out = rendered[name]
    H, W = sc.depth.shape
    h = 1.0 / 32 + 1.0 / 1024
    hit, z = _analytic_depth(sc.gt_pose, sc.K, H, W)
    assert np.array_equal(hit, sc.mask > 0)
    g = 1.0 / np.where(hit, z, 1.0)
    bound, ok = g.copy(), hit.copy()
    for axis in ((h, 0.0), (0.0, h)):
        slope = np.zeros_like(g)
        for sign in (-1.0, 1.0):
            hn, zn = _analytic_depth(sc.gt_pose, sc.K, H, W, sign * axis[0], sign * axis[1])
            ok &= hn
            slope = np.maximum(slope, g - 1.0 / np.where(hn, zn, 1.0))
        bound += slope
    check = ok & (out["model_mask"] > 0)
    assert check.sum() > 0.8 * hit.sum()
    zr = out["model_depth"].astype(np.float64)[check]
    zmin = 1.0 / bound[check]
    short = zmin - zr
    print(f"{name}: {check.sum()} px checked, worst shortfall {short.max():.3e} m against a margin of {16 * EPS * zr.max():.3e} m; "
          f"behind the surface by up to {(zr - z[check]).max() * 1e3:.3f} mm")
    assert (zr >= zmin - 16 * EPS * zr).all()
    assert (zr - z[check]).max() < 0.004       # ... and not far behind: the sagitta of a 4-degree chord seen at a grazing angle stays within millimetres


# ---- hand-derived cases: vertices on pixel centres (K = identity, z = 1: the image point of (c, r, 1) is pixel (c, r)) ------------------
K1 = np.eye(3, dtype=np.float32)
EYE = np.eye(4, dtype=np.float32)


def _flat(points, faces, H=8, W=9, depth=None, z=1.0, tol=0.005):
    v = np.array([(x, y, z) for x, y in points], np.float32)
    rgb = np.full((H, W, 3), 90, np.uint8)
    d = np.zeros((H, W), np.float32) if depth is None else depth
    return FR.render(v, np.array(faces, np.int32), EYE, K1, rgb, d, tol)


def _pixels(mask):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(mask))}


def test_sample_point_and_top_left_rule_both_windings():
    """right triangle (2,1) (6,1) (2,5): the top edge (row 1) and the left edge (column 2) belong to it, the hypotenuse x + y = 7 does not;
    the sample point of pixel (c, r) is (c, r) itself -- with c + 0.5 the set would be another one"""
    want = {(x, y) for x in range(2, 7) for y in range(1, 6) if x + y < 7}
    assert len(want) == 10
    for faces in ([(0, 1, 2)], [(0, 2, 1)]):
        out = _flat([(2, 1), (6, 1), (2, 5)], faces)
        assert _pixels(out["model_mask"]) == want
        assert np.array_equal(out["tri_id"] > 0, out["model_mask"] > 0)
        assert set(np.unique(out["model_depth"])) == {np.float32(0), np.float32(1)}
    # the mirror image (1,1) (5,1) (5,5): top edge in, RIGHT edge (column 5) out, the hypotenuse x = y is a left edge: in
    want = {(x, y) for x in range(1, 5) for y in range(1, 5) if y <= x}
    for faces in ([(0, 1, 2)], [(0, 2, 1)]):
        assert _pixels(_flat([(1, 1), (5, 1), (5, 5)], faces)["model_mask"]) == want


def test_shared_edge_every_pixel_exactly_once():
    pts = [(1, 1), (6, 2), (7, 7), (2, 5)]            # a quadrilateral split along the diagonal 0 - 2 (x = y); no edge is axis-aligned
    a = _flat(pts, [(0, 1, 2)])["model_mask"] > 0
    b = _flat(pts, [(0, 2, 3)])["model_mask"] > 0
    both = _flat(pts, [(0, 1, 2), (0, 2, 3)])
    assert a.any() and b.any() and not (a & b).any()
    assert np.array_equal(both["model_mask"] > 0, a | b)
    assert {(x, x) for x in range(2, 7)} <= _pixels(a | b), "the sample points on the shared edge belong to one of the two"
    # an axis-aligned square split along x = y: 16 pixels, each once
    sq = [(1, 1), (5, 1), (5, 5), (1, 5)]
    a = _flat(sq, [(0, 1, 2)])["model_mask"] > 0
    b = _flat(sq, [(0, 2, 3)])["model_mask"] > 0
    assert not (a & b).any() and _pixels(a | b) == {(x, y) for x in range(1, 5) for y in range(1, 5)}


def test_coincident_triangles_lower_index_wins_and_zero_area_draws_nothing():
    pts = [(2, 1), (6, 1), (2, 5), (4, 3), (6, 5)]
    out = _flat(pts, [(0, 3, 4), (0, 1, 2), (0, 2, 1), (0, 1, 2)])      # face 0 is collinear (zero area), faces 1-3 coincide
    assert set(np.unique(out["tri_id"])) == {0, 2}
    assert (out["model_mask"] > 0).sum() == 10
    nothing = _flat(pts, [(0, 3, 4), (1, 1, 2), (3, 3, 3)])
    assert not nothing["model_mask"].any() and not nothing["tri_id"].any() and not nothing["model_depth"].any()
    assert np.array_equal(nothing["overlay"], np.full((8, 9, 3), 90, np.uint8))
    # nearer wins whatever the index: the same triangle at z = 0.5 listed last
    v = np.array([(2, 1, 1), (6, 1, 1), (2, 5, 1), (1, 0.5, 0.5), (3, 0.5, 0.5), (1, 2.5, 0.5)], np.float32)
    out = FR.render(v, np.array([(0, 1, 2), (3, 4, 5)], np.int32), EYE, K1, np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.float32))
    assert set(np.unique(out["tri_id"])) == {0, 2} and set(np.unique(out["model_depth"])) == {np.float32(0), np.float32(0.5)}


def test_occluder_splits_the_visible_mask_exactly_and_missing_depth_is_visible(rendered, syn_mesh):
    sc, base = rendered["160x120"]
    H, W = sc.depth.shape
    model = base["model_mask"] > 0
    cols = np.nonzero(model.any(0))[0]
    c0 = int(cols[len(cols) // 2])
    z = base["model_depth"]
    tol = np.float32(0.005)
    depth = np.where(np.arange(W)[None, :] < c0, z - np.float32(0.02), z + np.float32(0.02)).astype(np.float32)   # in front | behind
    mesh = syn_mesh
    out = FR.render(FR.centred(mesh), mesh.faces, sc.gt_pose, sc.K, sc.rgb, depth, tol)
    want = model & (np.arange(W)[None, :] >= c0)
    assert want.any() and (model & ~want).any()
    assert np.array_equal(out["visible_mask"] > 0, want)
    assert np.array_equal(out["model_mask"], base["model_mask"]) and np.array_equal(out["model_depth"], z)
    changed = (out["overlay"] != sc.rgb).any(-1)
    assert not (changed & ~want).any() and changed[want].mean() > 0.9      # occluded and background pixels keep the frame's rgb
    # D == z - tol exactly is not "in front"; one ulp nearer is; D = 0 (missing) and D below the validity threshold count as visible
    edge = (z - tol).astype(np.float32)
    assert np.array_equal(FR.render(FR.centred(mesh), mesh.faces, sc.gt_pose, sc.K, sc.rgb, edge, tol)["visible_mask"], base["model_mask"])
    nearer = np.nextafter(edge, np.float32(0))
    assert not FR.render(FR.centred(mesh), mesh.faces, sc.gt_pose, sc.K, sc.rgb, nearer, tol)["visible_mask"].any()
    for missing in (np.zeros((H, W), np.float32), np.full((H, W), 0.0009, np.float32), np.full((H, W), np.nan, np.float32)):
        assert np.array_equal(FR.render(FR.centred(mesh), mesh.faces, sc.gt_pose, sc.K, sc.rgb, missing, tol)["visible_mask"], base["model_mask"])


def test_overlay_formula_by_hand():
    """a triangle facing the camera (normal along z: Lambert term 1, shade 255) over rgb 90: (90 + tint + 1) >> 1 per channel; seen at
    60 degrees (normal (0, sin, cos) 60 deg: term 0.5, shade 64 + rint(95.5) = 160): tint * 160 rounded to nearest of / 255"""
    out = _flat([(2, 1), (6, 1), (2, 5)], [(0, 1, 2)])
    px = out["overlay"][2, 3]
    assert tuple(px) == tuple((90 + t + 1) >> 1 for t in FR.TINT)
    assert tuple(out["overlay"][0, 0]) == (90, 90, 90)
    v = np.array([(0, 0, 2), (2, 0, 2), (0, 1, 2 + np.sqrt(3.0))], np.float32)    # edge b - a = (0, 1, sqrt 3): normal (0, -sqrt 3, 1) * 2
    k = int(FR.shade(v, np.array([(0, 1, 2)]), np.array([0]))[0])
    assert k == 64 + 96                                                          # rint(95.5) = 96 (half to even)
    assert [(t * k + 127) // 255 for t in FR.TINT] == [25, 138, 75]


def test_refusals_come_from_the_vertices():
    mesh = syn.make_mesh(1)
    K = syn.intrinsics()
    v = FR.centred(mesh)
    ok = syn.pose_matrix(np.eye(3), (0, 0, 0.5))
    assert FR.refused(v, ok, K) is None
    assert FR.refused(v, syn.pose_matrix(np.eye(3), (0, 0, 0.10)), K) == "near"            # the ellipsoid reaches z = 0.005 < 0.01
    assert FR.refused(v, syn.pose_matrix(np.eye(3), (0, 0, -1.0)), K) == "near"
    assert FR.refused(v, syn.pose_matrix(np.eye(3), (4000.0, 0, 0.2)), K) == "range"       # 320 * 4000 / 0.2 * 16 > 2^26
    assert FR.refused(v, syn.pose_matrix(np.eye(3), (np.nan, 0, 0.5)), K) == "range"
    with pytest.raises(FR.Refused, match="near"):
        FR.render(v, mesh.faces, syn.pose_matrix(np.eye(3), (0, 0, 0.10)), K, np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32))
