"""The references of fp_refine_depth (tests/icp_ref.py) before a kernel is held to them: a hand answer, the f32
restatement (a) against the float64 ray-cast ICP (b) with a bound derived in icp_ref.bounds, a negative control per rule, and (b)
against the ground truth of the synthetic scenes."""
import numpy as np
import pytest

import frame_render_ref as FR
import icp_cases as IC
import icp_ref as IR
from foundationpose_cpp_amd import synthetic as syn


def _one_step(mesh, P, D, translation_only):
    ev = IR.sums(FR.centred(mesh), mesh.faces, P, IC.K, D, IC.GATE, mesh.diameter)
    A, b = IR.system(ev["sums"])
    xi, rank, cond = IR.solve64(A, b, translation_only)
    return ev, xi, rank, IR.twist(np.asarray(P, np.float64), xi, float(np.float32(mesh.diameter) * np.float32(0.5)))


def test_hand_answer_plate():
    """a plate facing the camera at z0 under a depth of z0 + 3 mm: one iteration moves it 3 mm along z and nowhere else.  Only z and the
    rotations about x and y are observable (rank 3); with the translation-only flag only z (rank 1)."""
    m = IC.plate()
    ev, xi, rank, Q = _one_step(m, IC.PLATE_G, IC.PLATE_D, False)
    assert ev["n_used"] == ev["n_model"] == ev["n_valid"] > 500 and ev["n_front"] == ev["n_behind"] == ev["n_grazing"] == 0
    assert rank == 3
    assert abs(Q[2, 3] - (IC.PLATE_Z0 + 0.003)) < 1e-6                      # (f32 depth and z0: 3e-8 each)
    assert abs(Q[0, 3]) < 1e-12 and abs(Q[1, 3]) < 1e-12 and abs(xi[2]) < 1e-12
    assert np.abs(xi[:2]).max() < 1e-4                                      # the system is consistent: no rotation explains a constant offset
    ev, xi, rank, Q = _one_step(m, IC.PLATE_G, IC.PLATE_D, True)
    assert rank == 1 and np.all(xi[:5] == 0) and abs(Q[2, 3] - (IC.PLATE_Z0 + 0.003)) < 1e-6
    # the float64 reference gives the same answer
    r = IR.icp64(m, IC.PLATE_G, IC.K, IC.PLATE_D, IC.GATE, 1)
    assert r["rank"] == 3 and abs(r["pose"][2, 3] - (IC.PLATE_Z0 + 0.003)) < 1e-6 and IR.pose_gap(r["pose"], Q)[0] < 1e-3


CMP_CASES = [(seed, k) for seed in IC.SCENE_SEEDS for k in (0, 1)]


@pytest.mark.parametrize("seed,k", CMP_CASES)
def test_restatement_against_float64(seed, k):
    """one evaluation at the start pose: A and b of (a) within icp_ref.bounds of (b)'s; the pixels the two treat differently are counted
    and capped at 2 % of n_model for the classes"""
    c = IR.compare(IC.ico(4), IC.start(seed, k), IC.K, IC.scene(seed).depth, IC.GATE)
    print({key: v for key, v in c.items() if key not in ("a", "b")})
    assert c["n_model"] > 500 and c["a"]["n_used"] > 300
    assert c["n_class"] <= 0.02 * c["n_model"]
    assert c["dA"] <= c["bound_A"] and c["db"] <= c["bound_b"]
    for key in IR.COUNTS:
        assert abs(c["a"][key] - c["b"][key]) <= c["n_class"] + 1, key


def _gate_case():
    """an object near the frame's corner (l = 1.13 there), 19 mm nearer than what was observed: dz * l is beyond the 20 mm gate, dz is not"""
    m = IC.ico(3)
    G = IC.pose(syn.random_rotation(4), (0.15, 0.10, 0.35))
    return m, IC.moved(G, (0, 0, -0.019)), IC.rendering(m, G)


@pytest.mark.parametrize("wrong", ["sign_of_e", "t_not_subtracted", "gate_on_dz", "normal_not_normalised"])
def test_negative_controls_fail(wrong):
    """each rule broken on purpose leaves the bound or the 2 % cap of test_restatement_against_float64, which the unbroken rules keep"""
    if wrong == "gate_on_dz":
        m, P, D = _gate_case()
    else:
        m, P, D = IC.ico(4), IC.start(31, 1), IC.scene(31).depth
    good = IR.compare(m, P, IC.K, D, IC.GATE)
    assert good["n_class"] <= 0.02 * good["n_model"] and good["dA"] <= good["bound_A"] and good["db"] <= good["bound_b"]
    bad = IR.compare(m, P, IC.K, D, IC.GATE, wrong=wrong)
    print(wrong, {key: v for key, v in bad.items() if key not in ("a", "b")})
    assert bad["n_class"] > 0.02 * bad["n_model"] or bad["dA"] > bad["bound_A"] or bad["db"] > bad["bound_b"]


@pytest.mark.parametrize("seed", IC.SCENE_SEEDS)
def test_float64_icp_reaches_the_ground_truth(seed):
    """(b) on the noisy scenes from both starts: gate 0.02 m, 10 iterations.  Measured with the subdiv-4 mesh (degrees / mm from the truth,
    start 5 deg / 10 mm then 8 deg / 15 mm): seed 1 0.337 / 0.455 and 0.338 / 0.455, seed 11 0.126 / 0.124 and 0.138 / 0.125, seed 21
    0.219 / 0.206 twice, seed 31 0.312 / 0.114 twice.  0.455 mm is above the prototype's 0.3 mm, so the bound is twice (b)'s own worst."""
    ends = []
    for k in (0, 1):
        r = IC.refined64(seed, k)
        deg, dist = IR.pose_gap(r["pose"], IC.scene(seed).gt_pose)
        print(f"seed {seed} start {k}: {deg:.3f} deg {dist * 1e3:.3f} mm after {r['iterations']} updates, status {r['status']}, cond {r['cond']:.2e}, "
              f"last update {r['steps'][-1][0]:.1e} rad")
        assert deg <= IC.GT_BOUND_DEG and dist <= IC.GT_BOUND_M
        assert 1e-4 < r["cond"] < 1e-1
        ends.append(r["pose"])
    deg, dist = IR.pose_gap(ends[0], ends[1])                                # the same fixed point from both starts
    assert deg <= IC.AB_BOUND_DEG and dist <= IC.AB_BOUND_M


def test_iteration_on_the_integer_sums_follows_float64():
    """the library's iteration restated on (a)'s sums ends where (b) ends, within the bound the GPU test uses (one scene here; all four
    scenes and both starts were measured for icp_cases.AB_BOUND_*)"""
    seed = 21
    a = IR.icp32(IC.ico(4), IC.start(seed, 0), IC.K, IC.scene(seed).depth, IC.GATE, 10)
    deg, dist = IR.pose_gap(a["pose"], IC.refined64(seed, 0)["pose"])
    print(f"(a) against (b): {deg:.4f} deg {dist * 1e3:.4f} mm")
    assert deg <= IC.AB_BOUND_DEG and dist <= IC.AB_BOUND_M
    deg, dist = IR.pose_gap(a["pose"], IC.scene(seed).gt_pose)
    assert deg <= IC.GT_BOUND_DEG and dist <= IC.GT_BOUND_M
