"""The references of the frame-resolution pose calls under a GENERAL camera (tests/camera_cases.py), before a
kernel sees them: (a) every f32 restatement against its float64 reference per case and pose pair, (b) the same comparison with the
restatement given a camera broken on purpose -- fx and fy exchanged, cx and cy exchanged, the principal point truncated, fy taken for
fx -- which must leave the cap, the bound or the interval that (a) keeps, (c) what was wrong with the float64 reference of VSD, (d) the
values the GPU tests of tests/test_camera_sweep_gpu.py are held to, measured here.  The last test is a pure host function of the test
build: no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import camera_cases as CC
import frame_render_ref as FR
import geometry_cases as GC
import icp_ref as IR
import pose_error_ref as PR
import search_ref as SR
import vsd_ref as VR
from foundationpose_cpp_amd import _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p
from test_search_ref_cpu import MAX_DIFF_SHARE

MAX_CLASS_SHARE = 0.02          # of n_model: the cap of tests/test_icp_ref_cpu.py, a condition, not a measurement
PAIRS = [(seed, i) for seed in CC.SEEDS for i in range(len(CC.POSES))]
SEARCH_STEPS, SEARCH_TOL = 5, 0.05          # steps of diameter / 16; the tolerance in diameters
# an interval as wide as the object shows nothing: the uncertain pixels stay below a third of n_union (tests/test_vsd_ref_cpu.py asks for
# 5 % at 88 x 72 and f = 44; here a pixel is up to six times finer in metres, the thresholds 0.05 d and delta cut through the
# distribution of the differences, and the snap band of vsd_ref.CMP_BAND makes every pixel near a threshold uncertain)
MAX_UNSURE_SHARE = 1.0 / 3.0


def _id(pair):
    return f"{pair[0]}-{CC.POSES[pair[1]]}"


# ---- the cases are what they say --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", CC.SEEDS)
def test_the_cases_meet_their_conditions(seed):
    c = CC.camera_case(seed)
    W, H = c.W, c.H
    fx, fy, cx, cy = (float(c.K[0, 0]), float(c.K[1, 1]), float(c.K[0, 2]), float(c.K[1, 2]))
    assert (W, H) == CC.SIZES[seed] and c.depth.shape == (H, W) and c.rgb.shape == (H, W, 3)
    assert 0.6 * W <= fx <= 1.4 * W and (0.7 <= fy / fx <= 0.9 or 1.1 <= fy / fx <= 1.4)
    assert 0.3 * W <= cx <= 0.7 * W and 0.3 * H <= cy <= 0.7 * H
    for p in (cx, cy):
        assert min(p % 0.5, 0.5 - p % 0.5) >= 0.2 - 1e-6
    assert (c.K.ravel()[[1, 3, 6, 7]] == 0).all() and c.K[2, 2] == 1
    assert CC.is_convex(c.convex) and not CC.is_convex(c.mesh)
    assert np.abs(c.mesh.center).max() > 5e-3 and np.abs(c.convex.center).max() > 5e-3          # off-centre: the symmetries get conjugated
    v = FR.centred(c.mesh).astype(np.float64)
    for i, kind in enumerate(CC.POSES):
        for P in (c.G[i], c.E[i]):
            assert (v @ np.asarray(P, np.float64)[2, :3] + float(P[2, 3])).min() >= CC.MIN_Z
        z = CC.model_depth(c.mesh, c.G[i], c.K, H, W)
        assert (z != 0).sum() >= CC.MIN_MODEL_PIXELS
        deg, dist = IR.pose_gap(c.E[i], c.G[i])
        assert abs(deg - 3.0) < 1e-3 and abs(dist - 0.03 * c.mesh.diameter) < 1e-6
        if kind == "inside":
            assert not (z[0] != 0).any() and not (z[-1] != 0).any() and not (z[:, 0] != 0).any() and not (z[:, -1] != 0).any()
        if kind == "vertical_edge":
            assert (z[:, 0] != 0).any() or (z[:, -1] != 0).any()
        if kind == "horizontal_edge":
            assert (z[0] != 0).any() or (z[-1] != 0).any()
        if kind == "near":
            assert c.G[i][2, 3] < 0.17 and len(CC.tiles_of(z)) >= 4
    on = CC.model_depth(c.mesh, c.G[0], c.K, H, W) != 0
    D = c.depth[on]
    with np.errstate(invalid="ignore"):
        assert np.isnan(D).sum() >= 4 and np.isposinf(D).sum() >= 4 and ((D > 0) & (D < FR.MIN_DEPTH)).sum() >= 4 and (D == 0).sum() >= 0.05 * on.sum()
    assert 0.05 < (c.depth == 0).mean() < 0.2
    assert len({CC.camera_case(s).K[1, 1] > CC.camera_case(s).K[0, 0] for s in CC.SEEDS}) == 2          # fy above fx and below it


# ---- (a) the restatements against float64, (b) with a broken camera ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _icp64(seed, i):
    c = CC.camera_case(seed)
    return IR.evaluate64(c.mesh, c.E[i], c.K, c.depths[i], c.gate)


def _icp(seed, i, K):
    """(a) under the camera K against (b) under the true one, like icp_ref.compare"""
    c = CC.camera_case(seed)
    a = IR.sums(FR.centred(c.mesh), c.mesh.faces, c.E[i], K, c.depths[i], c.gate, c.mesh.diameter, maps=True)
    b = _icp64(seed, i)
    A, bb = IR.system(a["sums"])
    ca, cb = a["cls"], b["cls"]
    diff = (ca != cb) | (((ca == IR.USED) | (cb == IR.USED)) & (a["tri"] != b["tri"]))
    n_same = int(((ca == IR.USED) & (cb == IR.USED) & ~diff).sum())
    bound_A, bound_b = IR.bounds(c.mesh, c.E[i], c.K, c.gate, n_same, int(diff.sum()))
    return dict(n_model=max(a["n_model"], b["n_model"]), n_class=int((ca != cb).sum()), dA=float(np.abs(A - b["A"]).max()),
                db=float(np.abs(bb - b["b"]).max()), bound_A=bound_A, bound_b=bound_b, n_used=a["n_used"])


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_icp_restatement_against_float64(pair):
    seed, i = pair
    c = CC.camera_case(seed)
    r = _icp(seed, i, c.K)
    print(f"{_id(pair)}: {r['n_class']} of {r['n_model']} pixels classified differently, n_used {r['n_used']}, dA {r['dA']:.3e} of {r['bound_A']:.3e}, "
          f"db {r['db']:.3e} of {r['bound_b']:.3e}")
    assert r["n_used"] >= 300
    assert r["n_class"] <= MAX_CLASS_SHARE * r["n_model"] and r["dA"] <= r["bound_A"] and r["db"] <= r["bound_b"]
    for how in CC.BROKEN:
        w = _icp(seed, i, CC.broken(c.K, how))
        print(f"  {how}: {w['n_class']} of {w['n_model']}, dA {w['dA']:.3e} of {w['bound_A']:.3e}, db {w['db']:.3e} of {w['bound_b']:.3e}")
        assert w["n_class"] > MAX_CLASS_SHARE * w["n_model"] or w["dA"] > w["bound_A"] or w["db"] > w["bound_b"], (seed, i, how)


def _search_args(c, i):
    return (FR.centred(c.mesh), SR.normals_of(c.mesh), c.E[i:i + 1]), (c.depths[i], SEARCH_STEPS, np.float32(c.mesh.diameter) / np.float32(16),
                                                                         SEARCH_TOL * c.mesh.diameter)


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_search_restatement_against_float64(pair):
    seed, i = pair
    c = CC.camera_case(seed)
    head, tail = _search_args(c, i)
    cb, rb = SR.classify64(*head, c.K, *tail)
    assert not rb.any()

    def against(K):
        ca, ra = SR.classify(*head, K, *tail)
        assert not ra.any()
        return int(((ca != SR.NOT_FACING) | (cb != SR.NOT_FACING)).sum()), int((ca != cb).sum())

    n_facing, n_diff = against(c.K)
    print(f"{_id(pair)}: {n_diff} of {n_facing} facing triples differ")
    assert n_facing >= 50 and n_diff <= MAX_DIFF_SHARE * n_facing
    for how in CC.BROKEN:
        n_facing, n_diff = against(CC.broken(c.K, how))
        print(f"  {how}: {n_diff} of {n_facing}")
        assert n_diff > MAX_DIFF_SHARE * n_facing, (seed, i, how)


def _mspd64(c, E, G, S, step):
    """MSPD by a plain float64 projection with the FULL matrix K: p = K x, pixel = p[:2] / p[2]"""
    v = FR.centred(c.mesh).astype(np.float64)[::step]
    K = np.asarray(c.K, np.float64)
    E, G = np.asarray(E, np.float64), np.asarray(G, np.float64)
    centre = np.asarray(c.mesh.center, np.float64)
    to_mesh, to_centred = np.eye(4), np.eye(4)
    to_mesh[:3, 3], to_centred[:3, 3] = centre, -centre

    def pixels(T):
        p = (K @ (T[:3, :3] @ v.T + T[:3, 3:4])).T
        return p[:, :2] / p[:, 2:3]

    return min(float(np.linalg.norm(pixels(E) - pixels(G @ X), axis=1).max()) for X in [np.eye(4)] + [to_centred @ s @ to_mesh for s in S])


@pytest.mark.parametrize("seed", CC.SEEDS)
@pytest.mark.parametrize("step", [1, 3])
def test_mspd_reference_against_the_full_matrix(seed, step):
    c = CC.camera_case(seed)
    S = CC.symmetries(c.mesh)
    v = FR.centred(c.mesh)
    ref = PR.pose_errors(v, c.mesh.center, c.K, c.E, c.G, S, step)
    for i, r in enumerate(ref):
        assert abs(r["mspd_px"] - _mspd64(c, c.E[i], c.G[i], S, step)) < 1e-9 and r["mspd_px"] > 1.0
    for how in CC.BROKEN:
        w = PR.pose_errors(v, c.mesh.center, CC.broken(c.K, how), c.E, c.G, S, step)
        gaps = [abs(x["mspd_px"] - r["mspd_px"]) for x, r in zip(w, ref)]
        bounds = [PR.pixel_bound(r, c.K, r["mspd_px"]) for r in ref]
        print(f"seed {seed} step {step} {how}: " + " ".join(f"{g:.2e}/{b:.1e}" for g, b in zip(gaps, bounds)))
        if how in ("swap_cx_cy", "principal_point_truncated"):
            # MSPD is a difference of two projections: the principal point cancels, so no case can see these two in this field (the
            # projection itself is held to them through ICP, the search and VSD above and below)
            assert max(gaps) < 1e-9
        else:
            assert sum(g > b for g, b in zip(gaps, bounds)) >= 3, (seed, step, how)          # (one pair's largest move may lie along x alone)


VSD_TAUS = (0.05, 0.2, 0.5)          # BOP's smallest, a middle one and its largest


def _vsd_delta(c):
    return 0.15 * c.convex.diameter


@functools.lru_cache(maxsize=None)
def _vsd_intervals(seed, i):
    c = CC.camera_case(seed)
    return VR.intervals(c.convex, c.E[i], c.G[i], c.depths[i], c.K, _vsd_delta(c), VSD_TAUS)


def _vsd_record(seed, i, K):
    c = CC.camera_case(seed)
    return VR.vsd(c.convex, c.E[i:i + 1], c.G[i:i + 1], c.depths[i], K, _vsd_delta(c), VSD_TAUS)[0]


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_vsd_restatement_inside_the_float64_intervals(pair):
    seed, i = pair
    c = CC.camera_case(seed)
    rec = _vsd_record(seed, i, c.K)
    iv, n_unsure = _vsd_intervals(seed, i)
    print(f"{_id(pair)}: uncertain {n_unsure} of n_union {rec['n_union']}; " + "; ".join(f"{k} {rec[k]} in {iv[k]}" for k in VR.COUNTS)
          + f"; n_fail {rec['n_fail'][:3]} in {iv['n_fail']}")
    assert n_unsure <= MAX_UNSURE_SHARE * rec["n_union"]
    assert VR.inside(rec, iv) == [] and rec["status"] == 0 and 0 < rec["n_inter"] < rec["n_union"]


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_vsd_counts_with_a_broken_camera(seed):
    """The counts are areas: a silhouette wholly inside the frame keeps its area when the two focal lengths change places or when it moves
    by less than a pixel, so the pairs that cross an edge of the frame are the ones that must notice; each control leaves the intervals
    of at least one pair of every case, and the two exchanges leave those of both edge pairs."""
    c = CC.camera_case(seed)
    for how in CC.BROKEN:
        bad = [VR.inside(_vsd_record(seed, i, CC.broken(c.K, how)), _vsd_intervals(seed, i)[0]) for i in range(len(CC.POSES))]
        print(f"seed {seed} {how}: " + "; ".join(f"{kind}: {len(b)} counts outside" for kind, b in zip(CC.POSES, bad)))
        assert any(bad), (seed, how)
        if how.startswith("swap"):
            assert bad[1] and bad[2], (seed, how)


# ---- (c) what was wrong with the float64 reference of VSD -------------------------------------------------------------------------------
def test_the_float64_vsd_reference_is_for_convex_meshes():
    """The two pairs that first left their intervals (geometry_cases.random_case(2), poses 1 and 5) are of a DENTED mesh: the hull is not
    its silhouette (4 701 pixels of pose 1's hull are not covered by the body) and it has occlusion contours inside the silhouette,
    where a snap changes which surface a pixel sees.  `intervals` now says so instead of answering."""
    mesh, K, _, depth, poses, (H, W) = GC.random_case(2)
    assert not VR.is_convex(mesh)
    with pytest.raises(AssertionError, match="convex"):
        VR.intervals(mesh, poses[5], poses[5], depth, K)
    assert all(VR.is_convex(CC.camera_case(s).convex) for s in CC.SEEDS)


def test_the_constant_band_was_too_narrow():
    """... and on a convex mesh the band of 1e-5 m alone is too narrow for the 1/16 px snap on a leaning facet: with it three of the 24
    pairs leave their intervals in n_fail at thresholds that cut through the differences (0.02 d, 0.05 d); with the snap band derived at
    vsd_ref.CMP_BAND every one is inside (and the pairs above are, at BOP's thresholds)"""
    taus = (0.02, 0.05, 0.2)
    missed = []
    for seed, i in ((0, 1), (4, 1), (4, 2), (2, 0)):
        c = CC.camera_case(seed)
        rec = VR.vsd(c.convex, c.E[i:i + 1], c.G[i:i + 1], c.depths[i], c.K, _vsd_delta(c), taus)[0]
        narrow, _ = VR.intervals(c.convex, c.E[i], c.G[i], c.depths[i], c.K, _vsd_delta(c), taus, snap_band=False)
        derived, _ = VR.intervals(c.convex, c.E[i], c.G[i], c.depths[i], c.K, _vsd_delta(c), taus)
        print(f"seed {seed} {CC.POSES[i]}: outside the constant band's intervals {VR.inside(rec, narrow)}, outside the derived band's {VR.inside(rec, derived)}")
        missed.append(VR.inside(rec, narrow))
        assert VR.inside(rec, derived) == []
    assert missed == [["n_fail[1]"], ["n_fail[0]"], ["n_fail[1]"], []]


# ---- (d) the values the device is held to, measured here --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", CC.SEEDS)
def test_icp_iteration_bounds_are_what_was_recorded(seed):
    c = CC.camera_case(seed)
    a = IR.icp32(c.mesh, c.E[0], c.K, c.depth, c.gate, CC.ICP_ITERATIONS)
    b = IR.icp64(c.mesh, c.E[0], c.K, c.depth, c.gate, CC.ICP_ITERATIONS)
    ab = IR.pose_gap(a["pose"], b["pose"])
    gt = [max(x) for x in zip(IR.pose_gap(a["pose"], c.G[0]), IR.pose_gap(b["pose"], c.G[0]))]
    print(f"seed {seed}: (a) against (b) {ab[0]:.4f} deg {ab[1] * 1e3:.4f} mm; the farther of the two from the truth {gt[0]:.4f} deg {gt[1] * 1e3:.4f} mm; "
          f"(a) {a['iterations']} iterations, status {a['status']}, n_used {a['last']['n_used']}; (b) {b['iterations']} iterations, status {b['status']}")
    assert abs(ab[0] - CC.ICP_AB[seed][0]) <= CC.ICP_SLACK[0] and abs(ab[1] * 1e3 - CC.ICP_AB[seed][1]) <= CC.ICP_SLACK[1]
    assert abs(gt[0] - CC.ICP_GT[seed][0]) <= CC.ICP_SLACK[0] and abs(gt[1] * 1e3 - CC.ICP_GT[seed][1]) <= CC.ICP_SLACK[1]
    start = IR.pose_gap(c.E[0], c.G[0])
    assert gt[0] < 0.05 * start[0] and gt[1] < 0.05 * start[1]          # both do converge: from 3 deg and 3 % of the diameter to a twentieth


def test_register_reference_is_what_was_recorded():
    from oracle import fp_oracle as fo
    c = CC.camera_case(CC.REGISTER_SEED)
    rgb, D, mask, G = CC.register_scene()
    hyp = syn.from_colmajor(fo.get_hyp_poses(D, mask, c.K, inplane_step=60))
    assert hyp.shape == (252, 4, 4)
    r = SR.register_ref(c.mesh, hyp, c.K, D, IR.icp64, 16, 0.005, 15)
    got = CC.mssd(c.mesh, r["pose"], G) * 1e3
    print(f"hypothesis {r['hypothesis']}, rank_key {r['rank_key']}, MSSD {got:.3f} mm (recorded {CC.REF_MSSD_MM:.3f})")
    assert abs(got - CC.REF_MSSD_MM) <= CC.REF_SLACK_MM


# ---- the tile bound under this camera: a pure host function -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bound():
    L = _lib.test_lib()
    L.fpt_frame_tile_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]

    def call(pose, K, radius, H, W):
        out = np.zeros(4, np.int32)
        assert L.fpt_frame_tile_bound(_p(syn.to_colmajor(np.asarray(pose, np.float32))), _p(np.ascontiguousarray(K, np.float32)), radius, H, W, _p(out)) == 0
        return [int(v) for v in out]
    return call


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_tile_bound_contains_every_covered_tile(bound, seed):
    c = CC.camera_case(seed)
    ntx, nty = -(-c.W // CC.TILE), -(-c.H // CC.TILE)
    spared = 0
    for mesh in (c.mesh, c.convex):
        radius = float(np.sqrt((FR.centred(mesh).astype(np.float64) ** 2).sum(1).max()))
        for P in list(c.G) + list(c.E):
            tx0, ty0, tx1, ty1 = bound(P, c.K, radius, c.H, c.W)
            assert 0 <= tx0 and 0 <= ty0 and tx1 < ntx and ty1 < nty
            tiles = CC.tiles_of(CC.model_depth(mesh, P, c.K, c.H, c.W))
            assert tiles and all(tx0 <= x <= tx1 and ty0 <= y <= ty1 for x, y in tiles), (seed, mesh.name, P)
            spared += (tx1 - tx0 + 1) * (ty1 - ty0 + 1) < ntx * nty
    assert spared >= 2
