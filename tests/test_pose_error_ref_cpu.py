"""tests/pose_error_ref.py (the float64 reference of fp_pose_errors) against hand answers, the cases of tests/pose_error_cases.py against
what each is for, and the pure-numpy helpers recall / auc.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import pose_error_cases as PC
import pose_error_ref as PR
from foundationpose_cpp_amd import api

K = PC.K
PAIR = np.array([[-0.25, 0, 0], [0.25, 0, 0]])


def test_two_points_by_hand():
    E = PC.rigid(np.eye(3), (0, 0, 2))
    G = PC.rigid(np.eye(3), (Fraction(3, 8), 0, 2))
    r = PR.pose_error(PAIR, (0, 0, 0), K, E, G)
    # G u = (1/8, 5/8): the nearest E v are 1/4 (1/8 away) and 1/4 (3/8 away)
    assert r["add_m"] == Fraction(3, 8) and r["adds_m"] == Fraction(1, 4) and r["mssd_m"] == Fraction(3, 8)
    assert r["mspd_px"] == 320 * Fraction(3, 8) / 2 and r["best_sym"] == 0 and r["best_sym_mspd"] == 0
    assert r["rot_deg"] < 1e-12 and r["trans_m"] == Fraction(3, 8) and r["n_vertices"] == 2


def test_pure_translation():
    v = np.random.default_rng(1).normal(size=(50, 3)) * 0.05
    E = PC.rigid(PC.rot((1, 2, 3), 0.7), (0.1, -0.2, 0.9))
    G = E.copy()
    G[:3, 3] += np.array([3, 4, 12]) / 100.0
    r = PR.pose_error(v, (0, 0, 0), K, E, G)
    assert abs(r["add_m"] - 0.13) < 1e-15 and abs(r["mssd_m"] - 0.13) < 1e-15 and abs(r["trans_m"] - 0.13) < 1e-15
    assert r["adds_m"] <= r["add_m"] and r["rot_deg"] < 1e-12


def test_flip_of_a_symmetric_pair():
    flip = PC.rigid(PC.rot((0, 0, 1), np.pi))
    E = PC.rigid(PC.rot((0, 1, 0), 0.3), (0.02, 0.01, 1.5))
    G = E @ flip
    r = PR.pose_error(PAIR, (0, 0, 0), K, E, G)
    assert abs(r["add_m"] - 0.5) < 1e-15 and abs(r["mssd_m"] - 0.5) < 1e-15 and r["adds_m"] < 1e-15
    assert abs(r["rot_deg"] - 180.0) < 1e-6
    r = PR.pose_error(PAIR, (0, 0, 0), K, E, G, symmetries=[flip])
    assert abs(r["add_m"] - 0.5) < 1e-15 and r["adds_m"] < 1e-15 and r["mssd_m"] < 1e-15 and r["mspd_px"] < 1e-10
    assert r["best_sym"] == 1 and r["best_sym_mspd"] == 1 and r["rot_deg"] < 1e-6


def test_every_step_th_vertex_and_the_near_plane():
    v = np.random.default_rng(2).normal(size=(23, 3)) * 0.05
    E, G = PC.rigid(PC.rot((1, 0, 1), 0.2), (0, 0, 0.5)), PC.rigid(np.eye(3), (0.01, 0, 0.5))
    assert PR.pose_error(v, (0, 0, 0), K, E, G, step=7)["n_vertices"] == 4
    assert PR.pose_error(v, (0, 0, 0), K, E, G, step=7)["add_m"] == PR.pose_error(v[::7], (0, 0, 0), K, E, G)["add_m"]
    v = np.array([[0, 0, 0], [0, 0, -0.495]])
    r = PR.pose_error(v, (0, 0, 0), K, E, G)           # the second vertex has z = 0.005 under G
    assert r["mspd_px"] == float("inf") and r["best_sym_mspd"] == -1 and np.isfinite(r["mssd_m"]) and r["best_sym"] == 0


def test_recall_and_auc_by_hand():
    assert api.recall([0.01, 0.02, 0.03, float("nan")], 0.02) == 0.5
    assert api.recall([], 0.1) == 0.0 and api.recall([0.0], 0.0) == 1.0 and api.recall([float("inf")], 1e9) == 0.0
    assert api.auc([0.0, 0.0]) == pytest.approx(1.0, abs=1e-12)
    assert api.auc([0.2]) == 0.0
    # recall steps from 0 to 1 at the threshold 0.05: 50 whole steps of recall 1 and half of the step before them
    assert api.auc([0.05]) == pytest.approx((50 + 0.5) / 100, abs=1e-12)
    # half the poses perfect, half lost: the curve is flat at 1/2
    assert api.auc([0.0, 1.0]) == pytest.approx(0.5, abs=1e-12)
    assert api.auc([0.25], max_value=0.5, step=0.25) == pytest.approx(0.75, abs=1e-12)


def test_bound_is_below_1e_5_at_the_scale_of_the_cases():
    rec = dict(r=0.2, tE=1.0, tG=1.0)
    assert PR.metric_bound(rec, 0.2) < 1e-5
    assert PR.point_bound(0.2, 1.0, 1.0) == 2.0 ** -24 * 53.6


def test_box_lattice_is_what_it_is_for():
    mesh = PC.box()
    assert len(mesh.vertices) == 150 and np.abs(mesh.center - np.array(PC.BOX_OFFSET, np.float32)).max() < 1e-7
    v = PC.centred(mesh)
    for ax in np.eye(3):                                # invariant under the three rotations, as a set
        w = v.astype(np.float64) @ PC.rot(ax, np.pi).T
        assert np.abs(w[:, None, :] - v[None, :, :].astype(np.float64)).sum(-1).min(1).max() < 1e-7
    E, Gs = PC.box_poses()
    recs = [PR.pose_error(v, mesh.center, K, E, G, PC.box_symmetries()) for G in Gs]
    for k, r in enumerate(recs):
        assert abs(r["adds_m"] - 2.481e-3) < 1e-6 and abs(r["mssd_m"] - 4.342e-3) < 1e-6, (k, r["adds_m"], r["mssd_m"])
        assert abs(r["adds_m"] - recs[0]["adds_m"]) < 1e-7 and abs(r["mssd_m"] - recs[0]["mssd_m"]) < 1e-7
        assert r["best_sym"] == k and r["best_sym_mspd"] == k
        assert np.sort(r["per_sym_mssd"])[1] - r["mssd_m"] > 0.17 and np.sort(r["per_sym_mspd"])[1] - r["mspd_px"] > 130
        assert abs(r["rot_deg"] - np.degrees(0.02)) < 1e-4 and abs(r["trans_m"] - 0.002) < 1e-6
    adds = [r["add_m"] for r in recs]
    assert adds[0] == recs[0]["adds_m"] and 0.13 < min(adds[1:]) and 0.17 < max(adds) < 0.18     # (k = 0: no flip, ADD = ADD-S)


def test_negative_control_search_direction():
    """ADD-S searched the wrong way -- mean over E's points of the nearest G point -- misses the reference by a thousand bounds"""
    mesh = PC.cloud257()
    v = PC.centred(mesh).astype(np.float64)
    E, G = PC.cloud257_poses()
    r = PR.pose_error(v, mesh.center, K, E, G)
    wrong = PR.nearest_mean(v @ E[:3, :3].T + E[:3, 3], v @ G[:3, :3].T + G[:3, 3])
    assert abs(wrong - r["adds_m"]) > 1.4e-3 > 300 * PR.metric_bound(r, r["adds_m"])


def test_negative_control_centre_conjugation():
    """MSSD with the mesh-frame symmetries applied to the centred vertices as they are misses the reference"""
    mesh = PC.box()
    v = PC.centred(mesh)
    E, Gs = PC.box_poses()
    sym = PC.box_symmetries()
    r = PR.pose_error(v, mesh.center, K, E, Gs[2], sym)
    a = v.astype(np.float64) @ E[:3, :3].T + E[:3, 3]
    wrong = min(np.linalg.norm(a - (v.astype(np.float64) @ (Gs[2] @ S)[:3, :3].T + (Gs[2] @ S)[:3, 3]), axis=1).max() for S in [np.eye(4)] + list(sym))
    assert abs(wrong - r["mssd_m"]) > 0.05 > 1000 * PR.metric_bound(r, r["mssd_m"])


@pytest.mark.parametrize("V,N,S,paired,step", [c for c in PC.RAGGED if c[0] >= 63])
def test_ragged_nearest_neighbours_lie_at_the_end(V, N, S, paired, step):
    mesh, est, gt, sym, ref = PC.ragged(V, N, S, paired, step)
    v = PC.centred(mesh).astype(np.float64)[::step]
    assert len(v) == ref[0]["n_vertices"] == -(-V // step)
    if step == 1:
        assert (v[V // 2] == v[V // 2 - 1]).all()       # duplicate vertices
    D = np.linalg.inv(est[0]) @ gt[0]
    q = v @ D[:3, :3].T + D[:3, 3]
    n = min(8, len(v) // 4)
    nearest = np.linalg.norm(q[:n, None, :] - v[None, :, :], axis=-1).argmin(1)
    assert (nearest == len(v) - 1 - np.arange(n)).all()
    # without those targets the mean moves by far more than the bound
    short = PR.nearest_mean(q, v[:len(v) - n])
    assert short - ref[0]["adds_m"] > 10 * PR.metric_bound(ref[0], ref[0]["adds_m"])
    assert all(r["tE"] <= 1 and r["tG"] <= 1 and r["r"] <= 0.2 for r in ref)


def test_ragged_list_covers_what_it_must():
    assert {c[0] for c in PC.RAGGED} == {1, 2, 63, 64, 65, 1023, 1024, 1025} and {c[1] for c in PC.RAGGED} == {1, 3, 65}
    assert {c[2] for c in PC.RAGGED} == {0, 1, 7} and {c[3] for c in PC.RAGGED} == {True, False} and {c[4] for c in PC.RAGGED} == {1, 2, 3, 7}
