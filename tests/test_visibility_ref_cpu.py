"""Which triangle, if any, a pixel shows: the float64 ray-cast of tests/visibility_ref.py held to hand answers, and the CPU oracle
(oracle/fp_oracle.c) and the frame-resolution numpy reference (tests/frame_render_ref.py) held to its rules R1-R5.

The triangle ids of the kernels are bit-exact to the oracle, and sections 2.1's barycentric comparison takes the id as data: a pixel that
shows a triangle BEHIND the nearest one, or is wrongly left as background, passes both.  Here coverage is asked for exactly wherever no
open edge lies within delta = sqrt(2)/32 px + the f32 allowance of the sample point, the shown triangle has to contain the sample to
within delta and to be no deeper than any triangle that certainly covers it; ties are out of scope.  delta, the caps and the tolerances come
from the 1/16-px snap and the reference's own images, none from a device; every rule has wrong twins that must fail it.
tests/test_visibility_gpu.py imports cases, rules, delta and caps from here and applies them to the device's outputs unchanged.

Measured (oracle, both float models alike | frame reference): zero violations; coverage differs from hit(s) up to D = 0.0316 px | 0.0192 px
(delta 0.0448 | 0.0462); uncertain share per image <= 11.5 % (rnd5; every other case <= 7.9 %) | <= 5.1 %, over all images 1.73 % against
1.70 % by the reference alone | 1.31 % against 1.24 % (torus_plate); R4 live on 79.6 % of the closed meshes' foreground (>= 53.6 % per case).

One disagreement was found and fixed.  CudaRaster culls a triangle when its SNAPPED corners are collinear, so the collinear triangle of
`fine` surfaced in the oracle (far pose, ratio 1.2: a sample exactly on a snapped corner of the sliver, depth tie won by the later triangle)
and failed R3.  The loader now stores a face whose centred corners are exactly collinear as (i0, i0, i0), which no pose can open up."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

import frame_render_ref as FR
import test_shade_warp_ref_cpu as C
import visibility_cases as VC
import visibility_ref as V
from foundationpose_cpp_amd import synthetic as syn
from oracle import fp_oracle as fo

assert V.DELTA_CROP == V.SNAP + C.ETA             # the f32 allowance of the sample point is section 2.1's

CAP_IMAGE = 0.15               # share of an image's (foreground u hit) pixels that may lie within delta of an open edge ...
CAP_MIN_PIXELS = 1000          # ... for images with at least this many of them; smaller images are checked but not capped
CAPPED_PER_CASE = 2            # every case must have this many capped images
AGG_FACTOR = 1.5               # the share over all images of a run: at most this times what the reference alone gives on the same images
LIVE_MIN = 0.5                 # share of a closed mesh's foreground on which R4 can fail


# ---- references and images, computed once ---------------------------------------------------------------------------------------------
def crop_grids(c, ratio, **kw):
    return [V.crop_grid(tf, **kw) for tf in C.window_tf(c, ratio)]


@functools.lru_cache(maxsize=None)
def crop_references(name, ratio, delta=V.DELTA_CROP):
    """one Reference per pose; independent of the float model"""
    c = VC.case(name)
    return [V.reference(c.mesh, c.poses[n], c.K, g, delta) for n, g in enumerate(crop_grids(c, ratio))]


@functools.lru_cache(maxsize=None)
def oracle_images(name, ratio, fmad=True):
    """[(id, zw)] per pose in output orientation; R5 (rast[..., 3] == id buffer) is asserted on the way"""
    c = VC.case(name)
    fo.set_fmad(fmad)
    try:
        _, tri, rast = fo.render(fo.OracleMesh(c.mesh), syn.to_colmajor(c.poses), c.K, c.hw, ratio, debug=True)
    finally:
        fo.set_fmad(True)
    return crop_buffers(tri, rast)


def crop_buffers(tri, rast):
    assert (rast[..., 3].astype(np.int64) == tri).all(), "R5: rast id != triangle-id buffer"
    return [V.crop_images(tri[n], rast[n]) for n in range(len(tri))]


@functools.lru_cache(maxsize=None)
def frame_references(name, delta=V.DELTA_FRAME):
    c = VC.frame_case(name)
    return [V.reference(c.mesh, p, c.K, V.frame_grid(*c.hw), delta, znear=float(FR.NEAR), zfar=np.inf, depth="z") for p in c.poses]


@functools.lru_cache(maxsize=None)
def frame_ref_images(name):
    c = VC.frame_case(name)
    out = []
    for p in c.poses:
        r = FR.render(FR.centred(c.mesh), c.mesh.faces, p, c.K, np.zeros(c.hw + (3,), np.uint8), np.zeros(c.hw, np.float32))
        out.append((r["tri_id"].astype(np.int64), r["model_depth"].astype(np.float64)))
    return out


def own_images(refs):
    """the reference's own image per pose: what `the reference alone` means in the caps"""
    return [(r.tid, r.zw) for r in refs]


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def check_images(refs, images, what, rules=True):
    """R1-R4 on every image -> the per-image statistics; every image is checked before the first failure is raised"""
    stats = [V.check(r, tid, zw) for r, (tid, zw) in zip(refs, images)]
    if rules:
        bad = [f"pose {n}: " + ", ".join(f"{k} {s[k]}" for k in V.RULES if s[k]) + f" (of {s['n']} pixels, coverage differs up to D = {s['dmax']:.4f} px)"
               for n, s in enumerate(stats) if any(s[k] for k in V.RULES)]
        assert not bad, f"{what}: pixels violating " + "; ".join(bad)
    return stats


def check_caps(stats, what):
    """at most CAP_IMAGE of a capped image is uncertain, and the case has CAPPED_PER_CASE capped images"""
    capped = [s for s in stats if s["n"] >= CAP_MIN_PIXELS]
    for s in capped:
        assert s["uncertain"] <= CAP_IMAGE * s["n"], f"{what}: {s['uncertain'] / s['n']:.1%} of an image within delta of an open edge (cap {CAP_IMAGE:.0%})"
    assert len(capped) >= CAPPED_PER_CASE, f"{what}: {len(capped)} images of at least {CAP_MIN_PIXELS} pixels"
    return max(s["uncertain"] / s["n"] for s in capped)


def share(stats, num="uncertain", den="n"):
    return sum(s[num] for s in stats) / max(sum(s[den] for s in stats), 1)


def check_aggregate(stats, own, what):
    """the uncertain share over all images of a run against AGG_FACTOR x the reference's own on the same images"""
    got, ref = share(stats), share(own)
    print(f"  {what}: uncertain share over {len(stats)} images {got:.3%}, the reference alone {ref:.3%}, cap {AGG_FACTOR * ref:.3%}")
    assert got <= AGG_FACTOR * ref, (what, got, ref)
    return got, ref


def print_row(kind, name, extra, stats):
    print(f"  {kind:7s} {name:12s} {extra}: images {len(stats)} pixels {sum(s['n'] for s in stats)} uncertain {share(stats):.2%} "
          f"(worst image {max(s['uncertain'] / max(s['n'], 1) for s in stats):.2%}) live {share(stats, 'live', 'fg'):.1%} dmax {max(s['dmax'] for s in stats):.4f}")


# ---- (a) hand answers for the reference itself ---------------------------------------------------------------------------------------------
def _quad(half=0.05):
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float32)
    return syn.Mesh("quad", v, np.tile(np.float32([0, 0, -1]), (4, 1)), np.zeros((4, 2), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32),
                    np.full((2, 2, 3), 200, np.uint8), diameter=0.2, center=np.zeros(3, np.float32))


def _at(z, rx=0.0):
    return syn.pose_matrix(C._rot(rx, 0, 0), (0, 0, z))


def test_the_quad_of_the_known_answer_test_covers_columns_and_rows_47_to_113():
    """tests/test_oracle_kat.py::test_render_quad_geometry_and_fill_rule: a 0.1 m square at 1 m spans u in [304, 336]; the window [282, 282 + 159 / s],
    s = 160 / 76, puts crop pixel centre c + 1/2 at u = 282 + (c + 1/2) 159 / (160 s): (u - 282) 160 s / 159 in [46.61, 114.40] -> c in 47..113"""
    mesh = _quad()
    for rx in (0.0, 180.0):                                  # ... and the open quad is covered from BEHIND as well: nothing is culled
        pose = _at(1.0, rx)
        tf = fo.crop_window_tf(syn.to_colmajor(pose[None]), syn.intrinsics(), 1.2, mesh.diameter)[0]
        np.testing.assert_allclose([tf[0], tf[2], tf[5]], [160 / 76, -282 * 160 / 76, -202 * 160 / 76], rtol=1e-6)
        ref = V.reference(mesh, pose, syn.intrinsics(), V.crop_grid(tf), V.DELTA_CROP)
        ys, xs = np.nonzero(ref.hit)
        assert (xs.min(), xs.max(), ys.min(), ys.max()) == (47, 113, 47, 113) and ref.hit.sum() == 67 * 67
        assert set(np.unique(ref.tid)) == {0, 1, 2}
        np.testing.assert_allclose(ref.zw[ref.hit], 100.1 / 99.9 - 20 / 99.9, rtol=1e-12)
        # the boundary is open, the diagonal is not: D is the distance to the square's outline
        g = 160 * (160 / 76) / 159
        np.testing.assert_allclose(ref.D[80, 47], 47.5 - (304 - 282) * g, atol=1e-4)      # (tf is f32 data: its offset 593.7 carries 3e-5)
        assert ref.D[80, 80] > V.D_CAP
        tid, _ = V.render_by_rule(mesh, pose, syn.intrinsics(), V.crop_grid(tf), "cull_back")
        # ((p1 - p0) x (p2 - p0) of this quad is +z: it points away from a camera that looks along +z, so the unturned quad is the BACK face)
        assert (tid > 0).sum() == (0 if rx == 0 else 67 * 67)


def test_a_triangle_across_the_near_plane_is_cut_where_the_fractions_say():
    """camera-space corners (-1/16, 0, 1/4), (1/16, 0, 1/4), (0, -3/64, 1/16) under fx = fy = 320, c = (320, 240): the two lower corners project to
    (240, 240) and (400, 240); the edges to the apex meet z = 1/10 at t = (1/10 - 1/4) / (1/16 - 1/4) = 4/5, i.e. at (-+1/80, -3/80, 1/10) -> (280, 120) and
    (360, 120).  P is the trapezoid between rows 120 and 240 whose left side is u = 280 - (r - 120) / 3 and right side u = 360 + (r - 120) / 3"""
    v = np.array([[-1 / 16, 0, 1 / 4], [1 / 16, 0, 1 / 4], [0, -3 / 64, 1 / 16]], np.float32)
    mesh = syn.Mesh("tri", v, np.zeros((3, 3), np.float32), np.zeros((3, 2), np.float32), np.array([[0, 1, 2]], np.int32), np.zeros((2, 2, 3), np.uint8),
                    diameter=0.25, center=np.zeros(3, np.float32))
    pose = np.eye(4, dtype=np.float32)
    grid = V.frame_grid(480, 640)
    ref = V.reference(mesh, pose, syn.intrinsics(), grid, V.DELTA_CROP)
    g = ref.geo
    assert g.n[0] == 4 and g.clipped[0]
    want = {(240, 240), (400, 240), (360, 120), (280, 120)}
    assert {tuple(int(x) for x in np.rint(q)) for q in g.Q[0]} == want and np.abs(g.Q[0] - np.rint(g.Q[0])).max() < 1e-9
    left, right = [[280 - Fr(int(y) - 120, 3) for y in range(480)], [360 + Fr(int(y) - 120, 3) for y in range(480)]]
    inside = np.array([[120 < y < 240 and left[y] < x < right[y] for x in range(640)] for y in range(480)])
    on_edge = np.array([[120 <= y <= 240 and left[y] <= x <= right[y] for x in range(640)] for y in range(480)]) & ~inside
    assert (ref.hit[~on_edge] == inside[~on_edge]).all() and inside.sum() > 14000 and on_edge.sum() > 200      # (area (160 + 80) / 2 * 120 = 14400)
    assert not ref.hit[:120].any() and not ref.hit[241:].any()
    # the cut is an open edge, and so is every other edge of a clipped triangle
    np.testing.assert_allclose(ref.D[121, 300:341], 1.0, rtol=1e-9)
    np.testing.assert_allclose(ref.D[239, 300:341], 1.0, rtol=1e-9)
    # depth: at the cut z = 1/10, i.e. z/w = -1; on the lower edge z = 1/4
    np.testing.assert_allclose(g.value(g.z(np.array([0]), np.array([320.0]), np.array([120.0]))), -1.0, atol=1e-9)
    np.testing.assert_allclose(g.z(np.array([0]), np.array([320.0]), np.array([240.0])), 0.25, rtol=1e-12)
    # another near plane cuts elsewhere: at 1/16 the whole triangle shows, up to its apex at row 240 - 320 * 3/4 = 0
    tid, _ = V.render_by_rule(mesh, pose, syn.intrinsics(), grid, "znear=0.0625")
    assert (tid > 0)[1:120].any(1).all()
    tid, _ = V.render_by_rule(mesh, pose, syn.intrinsics(), grid, "znear=0.2")      # t = 4/15: rows above 240 - 320 * (3/64 * 4/15) / 0.2 = 220 are cut off
    assert not (tid > 0)[:220].any() and (tid > 0)[221:240].any(1).all()


def test_of_two_plates_1_mm_apart_the_nearer_one_shows_from_either_side():
    for name, front, back in (("plates_a", {3, 4}, {1, 2}), ("plates_b", {1, 2}, {3, 4})):       # (a: the farther quad is listed first)
        refs = crop_references(name, 1.2)
        for n, ids in ((0, front), (1, front), (2, back), (3, back)):
            both = refs[n].n_certain == 2                     # (seen at an angle the farther quad shows beside the nearer one)
            assert set(np.unique(refs[n].tid[both])) == ids, (name, n)
            assert both.sum() > 5000 and (refs[n].n_certain <= 2).all()


def _offset_quad_reference(dx, delta=V.DELTA_CROP):
    """a square [8, 24]^2 px (fx = fy = 64, corners at 1/8 and 3/8 m, 1 m away) sampled at columns 8 + dx + i, rows j + 1/4"""
    v = np.array([[1 / 8, 1 / 8, 0], [3 / 8, 1 / 8, 0], [3 / 8, 3 / 8, 0], [1 / 8, 3 / 8, 0]], np.float32)
    mesh = syn.Mesh("sq", v, np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.zeros((2, 2, 3), np.uint8),
                    diameter=0.5, center=np.zeros(3, np.float32))
    grid = V.Grid(8.0 + dx + np.arange(-8, 24), np.arange(32) + 0.25, 1.0, 0.0, 1.0, 0.0)
    return V.reference(mesh, _at(1.0), np.array([[64, 0, 0], [0, 64, 0], [0, 0, 1]], np.float32), grid, delta)


def test_a_sample_half_a_delta_on_either_side_of_an_edge():
    d = V.DELTA_CROP
    col, row = 8, 12                                          # the column at x = 8 + dx, a row well inside
    for dx, hit in ((d / 2, True), (-d / 2, False)):
        ref = _offset_quad_reference(dx)
        assert bool(ref.hit[row, col]) == hit and ref.hit[row, col + 1] and not ref.hit[row, col - 1]
        np.testing.assert_allclose(ref.D[row, col], d / 2, rtol=1e-9)
        np.testing.assert_allclose(ref.geo.dist(np.array([1]), ref.geo.grid.xs[[col]], ref.geo.grid.ys[[row]]), dx, rtol=1e-9)
        assert ref.n_certain[row, col] == 0 and ref.n_certain[row, col + 1] == 1
        for shown in (0, 2):                                  # within delta of the open edge either answer passes every rule
            tid, zw = ref.tid.copy(), ref.zw.copy()
            tid[row, col], zw[row, col] = shown, ref.zw[row, col + 1]
            s = V.check(ref, tid, zw)
            assert not any(s[k] for k in V.RULES) and s["uncertain"] > 0
    # two deltas outside: shown -> R1 and R3; two deltas inside: not shown -> R1 and R2
    ref = _offset_quad_reference(-2 * d)
    tid, zw = ref.tid.copy(), ref.zw.copy()
    tid[row, col], zw[row, col] = 2, ref.zw[row, col + 1]
    s = V.check(ref, tid, zw)
    assert (s["R1"], s["R2"], s["R3"], s["R4"]) == (1, 0, 1, 0)
    ref = _offset_quad_reference(2 * d)
    tid = ref.tid.copy()
    tid[row, col] = 0
    s = V.check(ref, tid, ref.zw)
    assert (s["R1"], s["R2"], s["R3"], s["R4"]) == (1, 1, 0, 0)


def test_a_triangle_of_exactly_zero_area_is_no_cover_and_fails_membership():
    c = VC.case("fine")
    ref = crop_references("fine", 1.2)[1]
    zero = np.nonzero(ref.geo.zero)[0]
    assert len(zero) == 2 and (zero >= len(c.mesh.faces) - 2).all()          # the repeated index and the collinear corners, nothing else
    assert not np.isin(ref.tid - 1, zero).any()
    iy, ix = np.argwhere(ref.hit & (ref.D > V.DELTA_CROP))[0]
    tid = ref.tid.copy()
    tid[iy, ix] = zero[1] + 1
    assert V.check(ref, tid, ref.zw)["R3"] == 1


def test_a_collinear_face_is_stored_so_that_no_pose_can_open_it():
    """the disagreement this module found: drawn as it is listed, `fine`'s collinear triangle snaps to a sliver in the far pose at ratio 1.2 and the
    oracle shows it at one pixel (R3); stored as (i0, i0, i0) it cannot.  The oracle's and the frame reference's stored faces agree with the rule's
    definition of zero area"""
    c = VC.case("fine")
    ref = crop_references("fine", 1.2)[2]
    raw = np.asarray(c.mesh.faces, np.int32)
    om = fo.OracleMesh(c.mesh)
    stored = om.faces.copy()
    changed = np.nonzero((stored != raw).any(1))[0]
    assert list(changed) == [len(raw) - 2, len(raw) - 1] and (stored[-2:] == raw[-2:, :1]).all()      # (a repeated index is collinear too)
    assert np.array_equal(FR.stored_faces(FR.centred(c.mesh), raw), stored)
    assert np.array_equal(np.nonzero(ref.geo.zero)[0], [len(raw) - 2, len(raw) - 1])
    om.faces[:] = raw                                      # (the C side reads this very array)
    _, tri, rast = fo.render(om, syn.to_colmajor(c.poses[2:3]), c.K, c.hw, 1.2, debug=True)
    s = V.check(ref, *V.crop_images(tri[0], rast[0]))
    assert (s["R1"], s["R2"], s["R3"], s["R4"]) == (0, 0, 1, 0), s
    om.faces[:] = stored
    _, tri, rast = fo.render(om, syn.to_colmajor(c.poses[2:3]), c.K, c.hw, 1.2, debug=True)
    s = V.check(ref, *V.crop_images(tri[0], rast[0]))
    assert not any(s[k] for k in V.RULES), s


# ---- (b) the oracle against R1-R5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmad", [True, False])
@pytest.mark.parametrize("name", VC.NEW_CASES + VC.OLD_CASES)
def test_oracle_obeys_the_visibility_rules(name, fmad):
    c = VC.case(name)
    for ratio in c.ratios:
        refs = crop_references(name, ratio)
        stats = check_images(refs, oracle_images(name, ratio, fmad), f"{name} ratio {ratio} fmad={int(fmad)}")
        print_row("oracle", name, f"ratio {ratio} fmad={int(fmad)}", stats)
        check_caps(stats, name)
        check_caps(check_images(refs, own_images(refs), name), f"{name} (the reference alone)")
        if name in VC.CLOSED_CASES:
            assert share(stats, "live", "fg") >= LIVE_MIN, f"R4 is live on {share(stats, 'live', 'fg'):.1%} of the foreground only"


# ---- (c) the frame-resolution numpy reference against R1-R4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.FRAME_CASES)
def test_frame_render_ref_obeys_the_visibility_rules(name):
    c = VC.frame_case(name)
    assert all(FR.refused(FR.centred(c.mesh), p, c.K) is None for p in c.poses)
    refs = frame_references(name)
    stats = check_images(refs, frame_ref_images(name), f"frame {name}")
    print_row("frame", name, "", stats)
    check_caps(stats, name)
    check_caps(check_images(refs, own_images(refs), name), f"{name} (the reference alone)")
    check_aggregate(stats, check_images(refs, own_images(refs), name), f"frame {name}")


# ---- (d), (e) measured values and the aggregate cap -----------------------------------------------------------------------------------------
def test_measured_values_and_the_aggregate_cap():
    """printed for DESIGN.md section 2.3: the largest D at which the oracle's coverage differs from hit(s) (it must not exceed delta: there is no
    half rule, the snap does reach its worst case), the uncertain share over all images against the reference's own, the live share of R4"""
    stats, own, closed = [], [], []
    for name in VC.NEW_CASES + VC.OLD_CASES:
        for ratio in VC.case(name).ratios:
            refs = crop_references(name, ratio)
            for fmad in (True, False):
                s = check_images(refs, oracle_images(name, ratio, fmad), name)
                stats += s
                own += check_images(refs, own_images(refs), name)
                closed += s if name in VC.CLOSED_CASES else []
    dmax = max(s["dmax"] for s in stats)
    print(f"  oracle: coverage differs from hit(s) up to D = {dmax:.4f} px (delta {V.DELTA_CROP:.4f}); R4 live on {share(closed, 'live', 'fg'):.1%} of the closed meshes' foreground")
    assert 0 < dmax <= V.DELTA_CROP
    check_aggregate(stats, own, "oracle, every case")
    fs = [s for name in VC.FRAME_CASES for s in check_images(frame_references(name), frame_ref_images(name), name)]
    print(f"  frame reference: coverage differs up to D = {max(s['dmax'] for s in fs):.4f} px (delta {V.DELTA_FRAME:.4f})")
    assert 0 < max(s["dmax"] for s in fs) <= V.DELTA_FRAME


# ---- (f) negative controls ---------------------------------------------------------------------------------------------------------------------
def control_images(name, ratio, rule, poses=None):
    """the reference's own images of a case under a wrong rule"""
    c = VC.case(name)
    tfs = C.window_tf(c, ratio)
    return [V.render_by_rule(c.mesh, c.poses[n], c.K, V.crop_grid(tfs[n]), rule, grid_of=functools.partial(V.crop_grid, tfs[n]))
            for n in (range(len(c.poses)) if poses is None else poses)]


def control_counts(name, ratio, rule, poses=None):
    """violations per rule, summed over the images, of the reference's own images under a wrong rule"""
    refs = crop_references(name, ratio)
    refs = refs if poses is None else [refs[n] for n in poses]
    stats = check_images(refs, control_images(name, ratio, rule, poses), name, rules=False)
    return {k: sum(s[k] for s in stats) for k in V.RULES}, stats


@pytest.mark.parametrize("name", VC.NEW_CASES + VC.OLD_CASES)
def test_the_reference_under_its_own_rule_passes(name):
    for ratio in VC.case(name).ratios:
        n, _ = control_counts(name, ratio, "nearest")
        assert not any(n.values())


@pytest.mark.parametrize("znear", [0.05, 0.2])
@pytest.mark.parametrize("name", list(VC.NEAR_POSES))
def test_another_near_plane_fails_coverage(name, znear):
    """a nearer plane shows what must be cut away (R1, and R3: shown pixels outside every P_k), a farther one cuts what must show (R1, R2)"""
    for pose in VC.NEAR_POSES[name]:
        n, _ = control_counts(name, 1.2, f"znear={znear}", [pose])
        print(f"  znear={znear} {name} pose {pose}: {n}")
        assert n["R1"] > 0 and (n["R3"] > 0 if znear < V.ZNEAR else n["R2"] > 0), n


@pytest.mark.parametrize("name", [n for n in VC.NEW_CASES + VC.OLD_CASES if n != "wquad"])       # (one quad has no second surface)
def test_the_farthest_surface_fails_the_depth_order(name):
    for ratio in VC.case(name).ratios:
        n, stats = control_counts(name, ratio, "farthest")
        print(f"  farthest {name} ratio {ratio}: {n} of {sum(s['fg'] for s in stats)} foreground pixels")
        assert n["R4"] > 0 and n["R1"] == n["R2"] == n["R3"] == 0, n


@pytest.mark.parametrize("name", ["torus_plate", "plates_a", "plates_b"])
def test_back_face_culling_fails_coverage(name):
    for ratio in VC.case(name).ratios:
        n, _ = control_counts(name, ratio, "cull_back")
        assert n["R1"] > 0 and n["R2"] > 0, n


@pytest.mark.parametrize("rule", ["no_half_pixel", "no_flip"])
@pytest.mark.parametrize("name", VC.NEW_CASES + VC.OLD_CASES)
def test_a_wrong_sample_grid_fails_coverage(name, rule):
    for ratio in VC.case(name).ratios:
        n, _ = control_counts(name, ratio, rule)
        assert n["R1"] > 0, n


def _single_cover(ref):
    """a pixel whose only cover is certain (d >= delta), and that triangle -- or None"""
    iy, ix = np.nonzero(ref.hit & (ref.n_certain == 1))
    k = ref.tid[iy, ix] - 1
    ok = ref.geo.dist(k, ref.geo.grid.xs[ix], ref.geo.grid.ys[iy]) >= ref.delta
    c = ref.geo.covers()
    alone = np.bincount(c["pix"], minlength=ref.hit.size).reshape(ref.hit.shape)[iy, ix] == 1
    i = np.nonzero(ok & alone)[0]
    return (int(k[i[0]]), int(iy[i[0]]), int(ix[i[0]])) if len(i) else None


@pytest.mark.parametrize("name", VC.NEW_CASES + VC.OLD_CASES)
def test_a_dropped_triangle_leaves_a_hole_or_shows_what_lies_behind(name):
    """without a triangle that certainly covers a pixel: R2 where nothing lies behind it (every mesh with a single-covered pixel), R4 on a
    closed surface, where its back shows instead"""
    c = VC.case(name)
    refs = crop_references(name, 1.2)
    tfs = C.window_tf(c, 1.2)
    tried = 0
    for n, ref in enumerate(refs):
        pick = _single_cover(ref)
        if pick is None and name in VC.CLOSED_CASES + ["edge"] and ref.hit.any():
            live = np.argwhere((ref.n_certain >= 2) & (ref.zfloor > ref.zcap + V.ZTOL))
            if not len(live):
                continue
            iy, ix = live[len(live) // 2]
            k = int(ref.tid[iy, ix] - 1)
            if ref.geo.dist(np.array([k]), ref.geo.grid.xs[[ix]], ref.geo.grid.ys[[iy]])[0] < ref.delta:
                continue
            pick = (k, iy, ix)
        if pick is None:
            continue
        k, iy, ix = pick
        tid, zw = V.render_by_rule(c.mesh, c.poses[n], c.K, V.crop_grid(tfs[n]), f"drop_triangle={k}")
        s = V.check(ref, tid, zw)
        assert (s["R2"] > 0 and tid[iy, ix] == 0) if ref.n_certain[iy, ix] == 1 else s["R4"] > 0, (name, n, s)
        tried += 1
    assert tried >= 2 or name == "edge"
    if name not in VC.CLOSED_CASES + ["edge"]:
        assert any(_single_cover(r) is not None for r in refs)


@pytest.mark.parametrize("name", VC.NEW_CASES + VC.OLD_CASES)
def test_one_wrong_pixel_fails(name):
    """the oracle's image with one interior pixel cleared (R1 + R2) or one background pixel far from every open edge set (R1)"""
    for ratio in VC.case(name).ratios:
        done = 0
        for ref, (tid, zw) in zip(crop_references(name, ratio), oracle_images(name, ratio)):
            inner = np.argwhere((ref.n_certain > 0) & (ref.D > ref.delta) & (tid > 0))
            outer = np.argwhere(~ref.hit & (ref.D > ref.delta) & (tid == 0))
            if not len(inner) or not len(outer):
                continue
            t = tid.copy()
            t[tuple(inner[len(inner) // 2])] = 0
            s = V.check(ref, t, zw)
            assert (s["R1"], s["R2"], s["R3"], s["R4"]) == (1, 1, 0, 0), s
            t = tid.copy()
            t[tuple(outer[len(outer) // 2])] = tid.max()
            s = V.check(ref, t, zw)
            assert s["R1"] == 1 and s["R2"] == 0, s
            done += 1
        assert done >= 2


DELTA0_CASES = VC.NEW_CASES + ["rnd1", "rnd5", "ellipsoid", "edge"]


def test_without_the_exemption_the_oracle_fails_coverage_on_most_images():
    """delta = 0: the oracle must FAIL R1 on most images -- the exemption is needed, and the check resolves 1/32 px"""
    failed = images = 0
    for name in DELTA0_CASES:
        refs = crop_references(name, 1.2, 0.0)
        stats = check_images(refs, oracle_images(name, 1.2), name, rules=False)
        failed += sum(s["R1"] > 0 for s in stats)
        images += len(stats)
    print(f"  delta = 0: the oracle fails R1 on {failed} of {images} images")
    assert failed > images / 2
