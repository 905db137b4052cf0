"""The references of fp_pose_search and fp_register_depth (tests/search_ref.py) before a kernel sees them: the f32
restatement (a) against the float64 restatement (b) on the eight noisy scenes, one negative control per rule, the hand answers of the
small cases the GPU test uses, and steps 2 to 5 with the float64 ICP on the eight scenes against the ground truth."""
import functools

import numpy as np
import pytest

import frame_render_ref as FR
import icp_cases as IC
import icp_ref as IR
import search_cases as SC
import search_ref as SR
from foundationpose_cpp_amd import synthetic as syn

MAX_DIFF_SHARE = 0.02          # of the facing (pose, step, point) triples: a condition, not a measurement


@functools.lru_cache(maxsize=None)
def hypotheses(seed):
    """the oracle's 252-pose grid at the sampler's translation"""
    from oracle import fp_oracle as fo
    sc = SC.scene(seed)
    hyp = syn.from_colmajor(fo.get_hyp_poses(sc.depth, sc.mask, sc.K, inplane_step=60))
    assert hyp.shape == (252, 4, 4)
    return hyp


def _compare(seed, wrong=None, poses=None):
    m = SC.mesh()
    sc = SC.scene(seed)
    return SR.compare(FR.centred(m), SR.normals_of(m), hypotheses(seed) if poses is None else poses, sc.K, sc.depth, 9, SC.step_of(m), SC.TOL,
                      SR.smallest_step(len(m.vertices)), wrong=wrong)


@pytest.mark.parametrize("seed", SC.SCENE_SEEDS)
def test_f32_restatement_agrees_with_float64(seed):
    c = _compare(seed)
    print(f"seed {seed}: {c['n_diff']} of {c['n_facing']} facing triples classified differently")
    assert c["refused_equal"] and c["n_facing"] > 400000
    assert c["n_diff"] <= MAX_DIFF_SHARE * c["n_facing"]


@pytest.mark.parametrize("wrong", ("step_direction", "no_facing_test", "half_pixel"))
def test_a_broken_rule_fails_the_comparison(wrong):
    c = _compare(1, wrong=wrong)
    print(f"{wrong}: {c['n_diff']} of {c['n_facing']}")
    assert c["n_diff"] > MAX_DIFF_SHARE * c["n_facing"]


def _tie_scene():
    """`>=` for `>` shows only where dz == tol_m exactly, in f32 and in float64 alike: a plate of 9 x 9 vertices at multiples of 1/128 m,
    facing the camera from exactly 0.5 m, under a wall exactly 2^-8 m behind it, with tol_m = 2^-8"""
    g = (np.arange(9) - 4) / 128.0
    v = np.stack([np.repeat(g, 9), np.tile(g, 9), np.zeros(81)], 1).astype(np.float32)
    n = np.tile(np.array([[0, 0, -1]], np.float32), (81, 1))
    return v, n, IC.pose(t=(0.0, 0.0, 0.5))[None], np.full((IC.H, IC.W), np.float32(0.5 + 2.0 ** -8)), 2.0 ** -8


def test_ties_belong_to_the_inliers():
    v, n, P, D, tol = _tie_scene()
    args = (v, n, P, IC.K, D, 1, 0.0, tol)
    ok = SR.compare(*args)
    assert ok["n_facing"] == 81 and ok["n_diff"] == 0
    assert SR.records(*args)[0]["n_inlier"] == 81
    bad = SR.compare(*args, wrong="ge_for_gt")
    assert bad["n_diff"] == 81
    assert SR.records(*args, wrong="ge_for_gt")[0]["n_behind"] == 81


def test_hand_answers_of_the_small_cases():
    E = {name: SC.expected(name) for name in SC.RECORD_CASES}
    for name, recs in E.items():
        for r in recs:
            assert r["n_facing"] == r["n_inlier"] + r["n_front"] + r["n_behind"] + r["n_outside"] + r["n_missing"], name
            assert r["score"] == r["n_inlier"] - r["n_behind"] - r["n_outside"], name
    assert [r["n_points"] for r in E["batch"]] == [162] * 7
    assert E["batch"][0]["n_inlier"] > 20 and E["batch"][5]["n_outside"] == E["batch"][5]["n_facing"] > 20
    assert 0 < E["edge"][0]["n_outside"] < E["edge"][0]["n_facing"]
    assert E["outside"][0]["n_outside"] == E["outside"][0]["n_facing"] > 20 and E["outside"][0]["score"] < 0
    assert E["plate_in_front"][0]["n_front"] == E["plate_in_front"][0]["n_facing"] > 20
    # NaN, 0 and +inf are each missing: every kind alone takes points of its own away, and together they take the sum
    m2 = IC.ico(2)
    _, nzi_poses, _, nzi_steps, nzi_step, _ = SC.record_case("nan_zero_inf")

    def at_step_0(kinds):
        cls, _ = SR.classify(FR.centred(m2), SR.normals_of(m2), nzi_poses, SC.K, SC.holes(kinds), 1, nzi_step, SC.TOL)
        return int((cls == SR.MISSING).sum()), int((cls == SR.BEHIND).sum())
    alone = {k: at_step_0((k,)) for k in SC.HOLES}
    assert at_step_0(()) == (0, at_step_0(())[1]) and all(n >= 2 for n, _ in alone.values()), alone
    assert at_step_0(tuple(SC.HOLES))[0] == sum(n for n, _ in alone.values())
    assert alone["inf"][1] == at_step_0(())[1]                                       # (+inf is not "behind")
    assert E["nan_zero_inf"][0]["best_step"] == 0 and E["nan_zero_inf"][0]["n_missing"] == at_step_0(tuple(SC.HOLES))[0]
    cls, refused = SC.classified("near_step")
    assert refused[0].tolist() == [True, False, False, False] and E["near_step"][0]["best_step"] >= 1 and E["near_step"][0]["status"] == 0
    blank = dict.fromkeys(SR.FIELDS, 0)
    assert E["all_refused"][0] == dict(blank, best_step=-1, status=SR.REFUSED_NEAR, n_points=162) and E["all_refused"][1]["status"] == 0
    assert E["cloud257"][0]["n_points"] == 257 and E["cloud4096"][0]["n_points"] == 4096 and E["vertex_step_3"][0]["n_points"] == 214
    assert all(r["best_step"] == 0 for r in E["zero_step"] + E["one_step"])
    assert len({r["best_step"] for r in E["max_steps"]}) > 1 and max(r["best_step"] for r in E["max_steps"]) > 8
    # the lowest step wins a tie, and a refused step competes with no score
    c = np.zeros((1, 3, 4), np.int8)
    c[0, 1] = c[0, 2] = SR.INLIER
    assert SR.summarise(c, np.zeros((1, 3), bool))[0]["best_step"] == 1
    assert SR.summarise(c, np.array([[False, True, False]]))[0]["best_step"] == 2
    c[0, 0] = SR.BEHIND
    assert SR.summarise(c, np.array([[False, True, True]]))[0]["score"] == -4


def test_candidates_and_winner_rules():
    recs = [dict(score=s, status=st) for s, st in ((5, 0), (9, 0), (9, 1), (9, 0), (-3, 0))]
    assert SR.pick_candidates(recs, 3) == [1, 3, 0] and SR.pick_candidates(recs, 16) == [1, 3, 0, 4]
    R = lambda status, used, behind, e2: dict(status=status, n_used=used, n_behind=behind, e2=e2)   # noqa: E731
    assert SR.pick_winner([7, 3, 9], [R(0, 100, 10, 5), R(0, 95, 5, 4), R(IR.TOO_FEW, 500, 0, 1)]) == 1          # the smaller sum e^2
    assert SR.pick_winner([7, 3], [R(0, 100, 10, 5), R(IR.CONVERGED, 95, 5, 5)]) == 1                           # then the lower hypothesis
    assert SR.pick_winner([7], [R(IR.REFUSED_NEAR, 100, 0, 1)]) is None
    P = SR.at_step(IC.pose(t=(0.1, -0.2, 0.5)), 2, 0.01)
    assert np.allclose(P[:3, 3], [0.104, -0.208, 0.52], atol=1e-7)


@pytest.mark.parametrize("seed", SC.SCENE_SEEDS)
def test_register_ref_reaches_an_equivalent_of_the_truth(seed):
    """steps 2 to 5 with the float64 ICP: the value recorded in search_cases.REF_MSSD_MM, which bounds the device.  The depth noise is
    1 mm; a wrong minimum of the ICP lies centimetres away, a near miss by a degree of rotation 2 mm or more (the semi-axis is 95 mm)."""
    m = SC.mesh()
    sc = SC.scene(seed)
    r = SR.register_ref(m, hypotheses(seed), sc.K, sc.depth, IR.icp64, SC.TOP_K, SC.TOL, SC.ITERATIONS)
    assert r is not None and r["n_candidates"] == SC.TOP_K
    got = SC.mssd_sym(m, r["pose"], sc.gt_pose) * 1e3
    print(f"seed {seed}: hypothesis {r['hypothesis']}, rank_key {r['rank_key']}, MSSD {got:.3f} mm (recorded {SC.REF_MSSD_MM[seed]:.3f})")
    assert got < 2.0
    assert abs(got - SC.REF_MSSD_MM[seed]) <= SC.REF_SLACK_MM
