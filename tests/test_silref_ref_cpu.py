"""tests/silref_ref.py on its own, without a GPU: the hand answers, the identity of the classes, the f32 restatement (a) against the float64
reference (b) with every negative control failing, the iteration's convergence on the wedge.  And the ABI of the
record."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_cases as IC
import silref_cases as SC
import silref_ref as RR
from foundationpose_cpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
f32 = np.float32


# ---- the hand case -----------------------------------------------------------------------------------------------------------------------
def test_the_hand_counts_and_the_hand_rms():
    ev = SC.expected0("hand")[0]
    assert {k: ev[k] for k in RR.COUNTS} == SC.HAND
    s = float(ev["scale_px"])
    assert abs(s - 100 * 0.06 * np.sqrt(2)) < 1e-5
    # sum e^2 = sum psi^2 / s^2 up to 44 roundings of a f32 division, a f32 product and a 2^-25 quantum each
    assert abs(ev["sums"][27] / 2.0 ** 24 * s * s - SC.HAND_SUM_PSI2) < 44 * (4 * 2.0 ** -24 * 4 + 2.0 ** -25 * s * s)
    assert abs(float(RR.rms_px(ev["sums"], ev["n_used"], ev["scale_px"])) - SC.HAND_RMS_PX) < 1e-5


def test_the_hand_values_of_psi():
    c = SC.case("hand")
    ev = RR.sums(RR.FR.centred(c["mesh"]), c["mesh"].faces, c["poses"][0], c["K"], SC.signed(("hand",)), c["mesh"].diameter, maps=True)
    psi = ev["psi"]
    assert all(psi[(r, 94)] == 2.0 for r in range(69, 81))                                  # outside, two columns from the mask
    assert all(psi[(r, 105)] == -2.0 for r in range(71, 79))                                # inside, three columns from the background
    assert psi[(70, 105)] == -1.0 and psi[(79, 105)] == -1.0 and psi[(69, 105)] == 0.0       # ... but the rows 68 and 81 are nearer
    assert all(psi[(r, c)] == 0.0 for r in (69, 80) for c in range(96, 106))                # the mask's own contour pixels
    assert psi[(69, 95)] == 1.0 and psi[(80, 95)] == 1.0                                    # the first ring outside
    assert len(psi) == 44


def test_the_hand_iteration():
    c = SC.case("hand")
    one = RR.silref32(c["mesh"], c["poses"][0], c["K"], c["mask"], 1, translation_only=True, sd=SC.signed(("hand",)))
    dx = float(one["pose"][0, 3]) - float(c["poses"][0][0, 3])
    assert SC.HAND_STEP_X_M[0] <= dx <= SC.HAND_STEP_X_M[1], dx
    assert one["rank"] == 3 and one["iterations"] == 1
    two = SC.iterated("hand")[0]                                                            # two updates, three evaluations
    assert two["iterations"] == 2 and two["last"]["n_used"] == 44
    assert two["last"]["sums"][27] == 0 and all(v == 0 for v in two["last"]["sums"][21:27])   # every contour pixel on one of the mask's
    # the full solve would turn the two-triangle plate by 0.79 rad at once: the cap holds it to MAX_STEP_RAD
    full = RR.silref32(c["mesh"], c["poses"][0], c["K"], c["mask"], 1, sd=SC.signed(("hand",)))
    rot, _, scale = full["steps"][0]
    assert rot > 0.5 and abs(rot * scale - RR.MAX_STEP_RAD) < 1e-12
    assert abs(IC.IR.pose_gap(full["pose"], c["poses"][0])[0] - np.degrees(RR.MAX_STEP_RAD)) < 1e-3


# ---- identities ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SC.RECORD_CASES if n != "batch_47"])
def test_n_contour_is_the_sum_of_the_classes(name):
    for ev in SC.expected0(name):
        if isinstance(ev, int):
            continue
        assert ev["n_contour"] == ev["n_used"] + ev["n_occluded"] + ev["n_far"] + ev["n_flat"] + ev["n_steep"]
        assert ev["n_contour"] <= ev["n_model"]


def test_the_cases_reach_their_classes():
    assert SC.expected0("refused") [1] == RR.REFUSED_NEAR and SC.expected0("refused")[3] == RR.REFUSED_RANGE
    assert all(SC.expected0("outside")[0][k] == 0 for k in RR.COUNTS)
    wall, occl = SC.expected0("wall"), SC.expected0("wall_occlusion")
    assert all(w["n_occluded"] == 0 for w in wall) and all(o["n_occluded"] > 20 and o["n_used"] > 20 for o in occl)
    assert all(w["n_contour"] == o["n_contour"] for w, o in zip(wall, occl))
    g1, g3, g0 = SC.expected0("gate_1"), SC.expected0("gate_3"), SC.expected0("ragged")
    assert sum(e["n_far"] for e in g1) > sum(e["n_far"] for e in g3) > 0 == sum(e["n_far"] for e in g0)
    edge = SC.expected0("edge")[0]                                                          # the frame's edge cuts the outline open
    inside = SC.expected0("ragged")[0]
    assert 0 < edge["n_contour"] < inside["n_contour"] and edge["n_model"] < inside["n_model"]


# ---- (a) against (b) -----------------------------------------------------------------------------------------------------------------------
COMPARE = (("wedge", 1), ("wedge", 21), ("edge", 0))


def _compare(which, wrong=None):
    if which[0] == "wedge":
        seed = which[1]
        return RR.compare(SC.wedge(), SC.wedge_start(seed, 0), SC.K, SC.wedge_mask(seed), wrong=wrong, sd=SC.signed(("wedge", seed)))
    c = SC.case("edge")
    return RR.compare(c["mesh"], c["poses"][1], c["K"], c["mask"], wrong=wrong, sd=SC.signed(c["sd_key"]))


def _holds(r):
    return r["n_unexplained"] == 0 and r["dA"] <= r["bound_A"] and r["db"] <= r["bound_b"]


@pytest.mark.parametrize("which", COMPARE)
def test_the_f32_restatement_agrees_with_float64(which):
    r = _compare(which)
    print(which, {k: r[k] for k in ("n_contour", "n_same", "n_class", "n_diff", "n_unexplained", "dA", "bound_A", "db", "bound_b")})
    assert r["n_same"] >= 0.7 * r["n_contour"] and r["n_same"] >= 40
    assert _holds(r)
    # the bound means something: a tenth of the system's own size at the most
    b = r["b"]
    assert r["bound_A"] < 0.1 * np.abs(b["A"]).max() and r["bound_b"] < 0.1 * np.abs(b["b"]).max()


@pytest.mark.parametrize("wrong", RR.WRONG)
def test_every_negative_control_fails(wrong):
    which = ("edge", 0) if wrong == "outside_is_background" else ("wedge", 1)
    r = _compare(which, wrong=wrong)
    print(wrong, {k: r[k] for k in ("n_contour", "n_same", "n_class", "n_diff", "n_unexplained", "dA", "bound_A", "db", "bound_b")})
    assert not _holds(r)


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SC.WEDGE_SEEDS)
@pytest.mark.parametrize("k", (0, 1))
def test_the_wedge_converges(seed, k):
    r = SC.wedge_refined(seed, k)
    start = SC.mssd(SC.wedge(), SC.wedge_start(seed, k), SC.wedge_truth(seed))
    end = SC.mssd(SC.wedge(), r["pose"], SC.wedge_truth(seed))
    print(seed, k, f"{start * 1e3:.3f} mm -> {end * 1e3:.3f} mm", r["status"], r["iterations"])
    assert start > 0.012
    assert abs(end * 1e3 - SC.REF_MSSD_MM[(seed, k)]) <= SC.REF_SLACK_MM
    assert SC.BOUND_M < 0.003                                                               # a tenth of a start, under one pixel (3.5 mm)
    ev = r["last"]
    assert ev["n_used"] >= 80 and ev["n_used"] >= 0.9 * ev["n_contour"] and float(RR.rms_px(ev["sums"], ev["n_used"], ev["scale_px"])) < 0.25


def test_the_ellipsoid_is_rank_deficient_and_translation_only_holds_it():
    full, trans = SC.iterated("ellipsoid")[0], SC.iterated("ellipsoid_translation")[0]
    c = SC.case("ellipsoid")
    import search_cases as SE
    G = SE.scene(1).gt_pose
    lateral = lambda P: float(np.linalg.norm((np.asarray(P, np.float64)[:2, 3] - np.asarray(G, np.float64)[:2, 3])))
    assert trans["rank"] == 3 and lateral(trans["pose"]) < 0.5 * lateral(c["poses"][0])
    assert full["cond"] < 0.02                                                              # the outline barely determines some direction
    first = SC.expected0("ellipsoid")[0]
    rms = lambda ev: float(RR.rms_px(ev["sums"], ev["n_used"], ev["scale_px"]))
    assert rms(trans["last"]) < rms(first)                                                  # (the scene's mask is the analytic ellipsoid's, not the mesh's: no zero)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
FIELDS = RR.INTS + RR.FLOATS + ("sums_q24",)


def test_the_abi_of_the_record():
    assert C.sizeof(_lib.FpSilhouetteRefine) == 288
    assert tuple(n for n, _ in _lib.FpSilhouetteRefine._fields_) == FIELDS
    offsets = {n: getattr(_lib.FpSilhouetteRefine, n).offset for n in FIELDS}
    assert offsets["n_steep"] == 24 and offsets["status"] == 36 and offsets["rms_px"] == 40 and offsets["last_trans_m"] == 56 and offsets["sums_q24"] == 64
    body = re.search(r"typedef struct fp_silhouette_refine \{(.*?)\} fp_silhouette_refine_t;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(int32_t|int64_t|float)\s+", "", decl.strip()).split(",")]
    assert tuple(names) == FIELDS

    def const(name):
        return re.search(rf"#define {name} +(\S+)", HEADER).group(1)

    assert int(const("FP_SILREF_MAX_ITERATIONS")) == RR.MAX_ITERATIONS == 32
    assert (int(const("FP_SILREF_TRANSLATION_ONLY")), int(const("FP_SILREF_OCCLUSION"))) == (RR.TRANSLATION_ONLY, RR.OCCLUSION) == (1, 2)
    assert const("FP_SILREF_MAX_TERM") == "64.0f" and float(RR.MAX_TERM) == 64.0
    assert float(const("FP_SILREF_MAX_STEP_RAD")) == RR.MAX_STEP_RAD == 0.2 and float(const("FP_SILREF_MAX_STEP_RADII")) == RR.MAX_STEP_RADII == 0.5
    assert int(const("FP_SILREF_MIN_PIXELS")) == RR.MIN_PIXELS == 16
    assert const("FP_SILREF_EPS_ROT_RAD") == "FP_ICP_EPS_ROT_RAD" and const("FP_SILREF_EPS_TRANS_M") == "FP_ICP_EPS_TRANS_M"
    assert tuple(int(const(n)) for n in ("FP_SILREF_CONVERGED", "FP_SILREF_TOO_FEW", "FP_SILREF_REFUSED_NEAR", "FP_SILREF_REFUSED_RANGE")) == \
        (RR.CONVERGED, RR.TOO_FEW, RR.REFUSED_NEAR, RR.REFUSED_RANGE) == (1, 2, 4, 8)
    assert re.search(r"#define FP_SILREF_MAX_WORK \d+LL", HEADER)
    assert "fp_refine_silhouette" in _lib.SYMBOLS and re.search(r"\bint fp_refine_silhouette\(", HEADER)
