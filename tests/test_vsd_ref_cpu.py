"""tests/vsd_ref.py, the references of fp_pose_vsd, held to each other and to hand answers without a GPU: the
float32 restatement lies inside the float64 ray-cast's intervals, the hand answers of the section come out exactly, and a restatement
with one rule broken fails the case that is there for that rule."""
import numpy as np
import pytest

import vsd_cases as VC
import vsd_ref as VR


def _one(name, wrong=None):
    recs = VC.expected(name, wrong)
    assert len(recs) == 1
    return recs[0]


def _T(name):
    return len(VC.case(name)["taus"])


@pytest.mark.parametrize("name", VC.F64_CASES)
def test_restatement_lies_inside_the_float64_intervals(name):
    c = VC.case(name)
    mesh = VC.mesh_of(c["mesh"])
    for i, rec in enumerate(VC.expected(name)):
        G = c["gt"][i if len(c["gt"]) > 1 else 0]
        iv, n_unsure = VR.intervals(mesh, c["est"][i], G, c["D"], VC.K, c["delta"], c["taus"], c["normalized"])
        print(f"{name}[{i}]: uncertain {n_unsure} of n_union {rec['n_union']}; " + "; ".join(f"{k} {rec[k]} in {iv[k]}" for k in VR.COUNTS)
              + f"; n_fail {rec['n_fail'][:len(c['taus'])]} in {iv['n_fail']}")
        assert n_unsure <= 0.05 * rec["n_union"], (name, n_unsure, rec["n_union"])          # FIRST: an interval as wide as the object shows nothing
        assert VR.inside(rec, iv) == [], (name, i)


def test_the_meshes_and_the_frame_are_what_the_kernels_need():
    assert len(VC.box().faces) == 12 and len(VC.ico().faces) == 320 > 256          # a 256-thread stride loops twice
    assert (VC.W % 32, VC.H % 32) == (24, 8) and (-(-VC.W // 32), -(-VC.H // 32)) == (3, 3)
    assert _one("box_same")["n_model_gt"] > 1500                                   # about 50 px across, over several tiles


@pytest.mark.parametrize("name", ["box_same", "box_same_nan", "box_same_missing"])
def test_equal_poses_give_zero(name):
    r = _one(name)
    assert r["n_inter"] == r["n_union"] == r["n_model_est"] == r["n_model_gt"] == r["n_visib_est"] == r["n_visib_gt"] > 0
    assert r["n_fail"] == [0] * 16 and all(v == 0 for v in r["vsd"][:10]) and all(np.isnan(v) for v in r["vsd"][10:]) and r["status"] == 0


def test_a_shift_in_depth_between_two_thresholds():
    r = _one("box_zshift")                                   # rigid: the deeper box is smaller, so the masks differ too
    assert r["n_inter"] == r["n_model_est"] < r["n_model_gt"] == r["n_union"]
    assert r["n_fail"][:2] == [r["n_inter"], 0] and r["vsd"][0] == 1.0 and r["vsd"][1] == VR.host_vsd(0, r["n_union"], r["n_inter"])
    r = _one("box_scaled")                                   # the same silhouette: exactly 1 and 0
    assert r["n_inter"] == r["n_union"] == r["n_model_gt"] > 1500
    assert r["n_fail"][:2] == [r["n_inter"], 0] and list(r["vsd"][:2]) == [1.0, 0.0]


def test_a_lateral_shift_counts_only_the_masks():
    r = _one("box_lateral")
    assert 0 < r["n_inter"] < r["n_model_gt"] < r["n_union"] and r["n_fail"][0] == 0
    assert r["vsd"][0] == np.float32((r["n_union"] - r["n_inter"]) / r["n_union"]) and 0.4 < r["vsd"][0] < 0.8


def test_outside_the_frame():
    r = _one("box_est_outside")
    assert (r["n_model_est"], r["n_inter"]) == (0, 0) and r["n_union"] == r["n_model_gt"] > 0 and all(v == 1.0 for v in r["vsd"][:10])
    r = _one("box_both_outside")
    assert all(r[k] == 0 for k in VR.COUNTS) and all(v == 1.0 for v in r["vsd"][:10]) and r["status"] == 0
    r = _one("box_half_outside")
    assert 0 < r["n_model_gt"] < 0.55 * _one("box_same")["n_model_gt"] and r["n_inter"] > 0


def test_an_occluding_plate_takes_its_pixels_from_the_visible_truth():
    c = VC.case("box_plate")
    z = VR.model_depth(VC.FR.centred(VC.box()), VC.box().faces, c["gt"][0], VC.K, VC.H, VC.W)
    covered = int((z[:, :44] != 0).sum())
    r = _one("box_plate")
    assert covered > 800 and r["n_visib_gt"] == r["n_model_gt"] - covered == r["n_visib_est"] == r["n_union"] and r["vsd"][0] == 0


def test_a_refused_pose_is_a_record_not_an_error():
    c = VC.case("box_same")
    behind = VC.moved(c["gt"][0], (0, 0, -0.5))
    recs = VR.vsd(VC.box(), [c["est"][0], behind], [behind, c["gt"][0]], c["D"], VC.K, taus=(0.2, 0.4))
    assert [r["status"] for r in recs] == [VR.GT_NEAR, VR.EST_NEAR]
    for r in recs:
        assert all(r[k] == 0 for k in VR.COUNTS) and list(r["vsd"][:2]) == [1.0, 1.0] and np.isnan(r["vsd"][2])


# ---- negative controls: one rule broken, the case that is there for it must notice ----------------------------------------------------
def test_control_without_the_visible_truth_clause():
    right, wrong = _one("ico_behind"), _one("ico_behind", "no_vis_g_clause")
    assert right["n_visib_est"] == right["n_model_est"] > 200                      # more than delta behind the observed surface, yet visible
    assert wrong["n_visib_est"] < 0.5 * right["n_visib_est"] and wrong["n_inter"] < right["n_inter"] and wrong["vsd"][1] != right["vsd"][1]


def test_control_z_instead_of_distance():
    right, wrong = _one("box_corner"), _one("box_corner", "z_not_distance")
    assert right["n_fail"][0] > 100 and wrong["n_fail"][0] == 0 and wrong["vsd"][0] < right["vsd"][0]


def test_control_strict_threshold():
    right, wrong = _one("box_tau0"), _one("box_tau0", "strict_threshold")
    assert right["n_fail"][:2] == [right["n_inter"], 0] and list(right["vsd"][:2]) == [1.0, 0.0]
    assert wrong["n_fail"][:2] == [0, 0] and wrong["vsd"][0] == 0.0


def test_control_missing_depth_hides():
    right, wrong = _one("box_same_missing"), _one("box_same_missing", "missing_hides")
    assert right["n_union"] == right["n_model_gt"] and wrong["n_union"] == 0 and wrong["vsd"][0] == 1.0
    nan_right, nan_wrong = _one("box_same_nan"), _one("box_same_nan", "missing_hides")
    assert all(nan_right[k] == right[k] == nan_wrong[k] for k in VR.COUNTS)        # (a NaN hides nothing under either rule)
