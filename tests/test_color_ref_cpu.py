"""The references of fp_pose_color and fp_resolve_symmetry (tests/color_ref.py) before a kernel sees them: the f32
restatement (a) against the float64 restatement (b) on the four GPU scenes under an 8 x 8 texture, one negative control per rule, the
hand answers, the invariances of the correlation, and the resolution rule after the weight-free Register of the reference on the eight
scenes against the ground truth."""
import functools

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import frame_render_ref as FR
import icp_cases as IC
import icp_ref as IR
import search_cases as SC
import search_ref as SR
from foundationpose_cpp_amd import synthetic as syn

MAX_TEXEL_SHARE = 0.02         # of the pixels both restatements compare: a condition, not a measurement
MAX_COVER_SHARE = 0.02         # of the pixels either covers: coverage, visibility or winning triangle


def _a(mesh, pose, rgb, D, wrong=None):
    return CR.sums_of_mesh(mesh, pose, CC.K, rgb, D, CC.TOL, wrong=wrong, maps=True)


@functools.lru_cache(maxsize=None)
def _scene_b(seed):
    s = CC.scene(seed)
    return CR.color64(CC.mesh2_tex8(), s.gt_pose, s.K, s.rgb, s.depth, CC.TOL)


@functools.lru_cache(maxsize=None)
def _quad_b():
    return CR.color64(CC.quad(), CC.QUAD_P, CC.K, CC.noise_rgb(6), np.full((CC.H, CC.W), IC.WALL, np.float32), CC.TOL)


def _quad_a(wrong=None):
    return _a(CC.quad(), CC.QUAD_P, CC.noise_rgb(6), np.full((CC.H, CC.W), IC.WALL, np.float32), wrong)


@pytest.mark.parametrize("seed", CC.GPU_SEEDS)
def test_f32_restatement_agrees_with_float64(seed):
    s = CC.scene(seed)
    a, b = _a(CC.mesh2_tex8(), s.gt_pose, s.rgb, s.depth), _scene_b(seed)
    cover, texel, n = CR.compare(a, b)
    print(f"seed {seed}: {100 * cover:.2f} % differ in coverage or triangle, {100 * texel:.2f} % of {n} pixels pick another texel; "
          f"zncc {a['zncc64']:.4f} (a) {b['zncc64']:.4f} (b)")
    assert n > 500 and a["n_nocolor"] == 0
    assert cover <= MAX_COVER_SHARE and texel <= MAX_TEXEL_SHARE


def test_the_quad_agrees_with_float64():
    """the quad of the negative controls below passes the caps with the rules as they are: strong foreshortening, wraps, negative coordinates"""
    cover, texel, n = CR.compare(_quad_a(), _quad_b())
    print(f"quad: {100 * cover:.2f} % coverage, {100 * texel:.2f} % of {n} texels")
    assert n > 500 and cover <= MAX_COVER_SHARE and texel <= MAX_TEXEL_SHARE


@pytest.mark.parametrize("wrong", ["v_not_flipped", "uv_swapped", "half_pixel"])
def test_a_broken_rule_fails_the_comparison_on_a_scene(wrong):
    s = CC.scene(1)
    cover, texel, n = CR.compare(_a(CC.mesh2_tex8(), s.gt_pose, s.rgb, s.depth, wrong), _scene_b(1))
    print(f"{wrong}: {100 * texel:.2f} % of {n}")
    assert texel > MAX_TEXEL_SHARE


@pytest.mark.parametrize("wrong", ["affine", "clamp"])
def test_a_broken_rule_fails_the_comparison_on_the_quad(wrong):
    cover, texel, n = CR.compare(_quad_a(wrong), _quad_b())
    print(f"{wrong}: {100 * texel:.2f} % of {n}")
    assert texel > MAX_TEXEL_SHARE


def _hand(name, **kw):
    c = CC.case(name)
    m = c["mesh"]
    return CR.sums(FR.centred(m), m.faces, c["poses"][0], c["K"], c["rgb"], c["D"], CC.TOL, uvs=CR.stored_uvs(m), tex=m.texture, colors=c["colors"], **kw)


@pytest.mark.parametrize("tw", [2, 3])
def test_hand_answer_of_the_textured_triangle(tw):
    got, ref = _hand(f"hand_{tw}x2"), CC.hand_expected(tw)
    for k in CR.COUNTS + CR.SUMS + ("status",):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert (got["n_model"], got["n_visible"], got["n_compared"], got["n_nocolor"], got["status"]) == (78, 78, 78, 0, 0)
    # the table's columns: 7 + 6 + ... of the 78 pixels per texel, written out for the 2 x 2 texture's red channel
    if tw == 2:
        count = {(0, 1): 0, (1, 1): 0, (0, 0): 0, (1, 0): 0}
        for _, _, k, j in CC.hand_pixels():
            count[(0 if k <= 6 else 1, 1 if j <= 6 else 0)] += 1
        assert count == {(0, 1): 48, (1, 1): 15, (0, 0): 15, (1, 0): 0}
        assert got["sum_m"][0] == 48 * 70 + 15 * 100 + 15 * 10 and got["sum_mm"][0] == 48 * 4900 + 15 * 10000 + 15 * 100
    assert got["zncc"] == np.float32(CR.zncc_of(78, *(ref[k] for k in CR.SUMS))[1])


def test_bgr_for_rgb_changes_the_sums():
    good, bad = _hand("hand_3x2"), _hand("hand_3x2", wrong="bgr")
    assert good["sum_m"] != bad["sum_m"] and good["sum_mo"] != bad["sum_mo"] and good["sum_o"] == bad["sum_o"]
    assert bad["sum_m"] == good["sum_m"][::-1]


def test_hand_answer_of_the_vertex_colours():
    r = _hand("hand_vcol", maps=True)
    assert (r["n_model"], r["n_compared"], r["n_nocolor"], r["status"]) == (78, 78, 0, 0)
    for (c, row), want in CC.HAND_VCOL_AT.items():
        assert tuple(int(x) for x in r["values"][row, c]) == want, ((c, row), r["values"][row, c], want)
    assert np.rint(np.float32(12.5)) == 12 and np.rint(np.float32(13.5)) == 14          # half to even, as rintf


def test_a_plate_in_front_and_the_grey_default():
    r = CC.expected("plate_in_front")[0]
    assert r["n_model"] > 500 and r["n_visible"] == 0 and r["n_compared"] == 0 and r["status"] == CR.TOO_FEW and r["zncc"] == 0
    g = CC.expected("grey")[0]
    assert g["n_compared"] > 500 and g["status"] == CR.FLAT and g["zncc"] == 0
    assert g["sum_m"] == [100 * g["n_compared"]] * 3 and g["sum_mm"] == [10000 * g["n_compared"]] * 3


def test_refused_poses_of_the_cases():
    assert [r["status"] for r in CC.expected("refused")] == [0, CR.REFUSED_NEAR, 0, CR.REFUSED_RANGE, 0]
    assert CC.expected("batch_512")[5]["n_model"] == 0 and CC.expected("batch_512")[5]["status"] == CR.TOO_FEW          # wholly outside
    assert all(r["n_visible"] == r["n_compared"] + r["n_nocolor"] for name in CC.CASES for r in CC.expected(name))


def test_the_correlation_ignores_gain_and_offsets_and_is_one_on_the_models_own_picture():
    c = CC.case("batch_512")
    m, P = c["mesh"], c["poses"][0]
    rgb = (CC.noise_rgb(11) // 4 + 20).astype(np.uint8)                              # 20 .. 83: 3 o + b stays below 256
    base = _a(m, P, rgb, c["D"])
    assert base["status"] == 0
    for gain, offset in ((2, (0, 0, 0)), (1, (5, 60, 17)), (3, (1, 0, 6))):
        moved = (rgb.astype(np.int64) * gain + np.array(offset)).astype(np.uint8)
        assert (moved.astype(np.int64) == rgb.astype(np.int64) * gain + np.array(offset)).all()          # nothing clipped
        r = _a(m, P, moved, c["D"])
        assert abs(r["zncc64"] - base["zncc64"]) <= 1e-12, (gain, offset, r["zncc64"], base["zncc64"])
        assert r["sum_m"] == base["sum_m"] and r["sum_o"] != base["sum_o"]
    own = _a(m, P, CR.painted(base, rgb), c["D"])
    assert own["sum_m"] == own["sum_o"] and own["sum_mm"] == own["sum_oo"] == own["sum_mo"] and own["zncc64"] == 1.0 and own["zncc"] == 1


def test_equivalents_and_the_winner_rule():
    m = CC.mesh3()
    G = CC.scene(1).gt_pose
    E = CC.scene_equivalents(1)
    assert E.shape == (4, 4, 4) and E.dtype == np.float32 and E[0].tobytes() == np.asarray(G, np.float32).tobytes()
    for s, S in enumerate(SC.SYMMETRIES):
        assert np.abs(E[s + 1].astype(np.float64) - G.astype(np.float64) @ S).max() < 1e-6
    R = lambda status, z: dict(status=status, zncc=np.float32(z))   # noqa: E731
    assert CR.resolve([R(0, 0.2), R(0, 0.7), R(0, 0.7), R(CR.FLAT, 0.9)]) == 1          # ties to the lower index, flagged records never
    assert CR.resolve([R(CR.TOO_FEW, 0.0), R(CR.REFUSED_NEAR, 0.0)]) is None
    assert CR.resolve([R(0, -0.5)]) == 0
    assert len(m.vertices) == 642


@functools.lru_cache(maxsize=None)
def _hypotheses(seed):
    """the oracle's 252-pose grid at the sampler's translation"""
    from oracle import fp_oracle as fo
    sc = SC.scene(seed)
    return syn.from_colmajor(fo.get_hyp_poses(sc.depth, sc.mask, sc.K, inplane_step=60))


def _plain_mssd(m, P, G):
    v = FR.centred(m).astype(np.float64)
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    return float(np.linalg.norm((v @ P[:3, :3].T + P[:3, 3]) - (v @ G[:3, :3].T + G[:3, 3]), axis=1).max())


@pytest.mark.parametrize("seed", CC.SCENE_SEEDS)
def test_the_resolution_rule_finds_the_equivalent_nearest_the_truth(seed):
    """the weight-free Register of the reference lands on AN equivalent; the colour of the scene's own 512^2 texture picks the true one"""
    m, sc = CC.mesh3(), CC.scene(seed)
    assert sc.depth.tobytes() == SC.scene(seed).depth.tobytes()                      # the textured mesh changes the picture only
    r = SR.register_ref(SC.mesh(), _hypotheses(seed), sc.K, sc.depth, IR.icp64, SC.TOP_K, SC.TOL, SC.ITERATIONS)
    E = CC.scene_equivalents(seed, np.asarray(r["pose"], np.float32))
    recs = [CR.sums_of_mesh(m, P, sc.K, sc.rgb, sc.depth, CC.TOL) for P in E]
    errs = [_plain_mssd(m, P, sc.gt_pose) for P in E]
    win = CR.resolve(recs)
    z = sorted((float(x["zncc"]) for x in recs), reverse=True)
    print(f"seed {seed}: plain MSSD of the Register {errs[0] * 1e3:.2f} mm, of the winner {errs[win] * 1e3:.2f} mm; zncc winner {z[0]:.3f}, "
          f"runner-up {z[1]:.3f}; all {[round(float(x['zncc']), 3) for x in recs]}")
    assert all(x["status"] == 0 for x in recs)
    assert win == int(np.argmin(errs))
    assert errs[win] < 2e-3
