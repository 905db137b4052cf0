"""tests/silhouette_ref.py on its own, without a GPU: the brute-force distance transform against a second, separable one; hand answers; the
identities of the record; and the signal on the synthetic scenes.  And the ABI of the record."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_cases as IC
import search_cases as SC
import silhouette_cases as SIC
import silhouette_ref as SR
from foundationpose_cpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()


def separable_edt2(seed):
    """the second implementation: per column the distance to the nearest seed above and below by running maxima / minima of seed rows,
    then per row the minimum over the columns of (c - c')^2 + g(r, c')^2.  No loop over seeds, no pixel-against-seed table."""
    seed = np.asarray(seed, bool)
    H, W = seed.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    far = np.int64(1) << 40
    above = np.maximum.accumulate(np.where(seed, rows, -far), axis=0)                      # the last seed row at or above r
    below = np.minimum.accumulate(np.where(seed, rows, far)[::-1], axis=0)[::-1]           # the first seed row at or below r
    g = np.minimum(rows - above, below - rows)                                             # >= 2^39 where the column has no seed
    none = g >= (far >> 1)
    g2 = np.where(none, far, g * g)
    cols = np.arange(W, dtype=np.int64)
    dc2 = (cols[:, None] - cols[None, :]) ** 2                                              # [c, c']
    out = (dc2[None, :, :] + g2[:, None, :]).min(axis=2)
    return np.where(out >= far, SR.D2_NONE, out)


@pytest.mark.parametrize("name", SIC.CPU_MASKS)
def test_brute_force_equals_the_separable_transform(name):
    on = SIC.mask_case(name) > 0
    d2m, d2b = SIC.mask_expected(name)
    assert d2m.dtype == np.int64 and d2m.shape == on.shape
    assert np.array_equal(d2m, separable_edt2(on)) and np.array_equal(d2b, separable_edt2(~on))
    assert np.array_equal(d2m == 0, on) or not on.any()
    assert np.array_equal(d2b == 0, ~on) or on.all()
    if on.any() and not on.all():
        assert d2b[on].min() >= 1 and d2m[~on].min() >= 1
    print(f"{name}: {on.shape}, {int(on.sum())} mask pixels, largest d2 to the mask {int(d2m.max())}, to the background {int(d2b.max())}")


def test_empty_and_full_sides_have_no_distance():
    m, b = SIC.mask_expected("empty")
    assert (m == SR.D2_NONE).all() and (b == 0).all()
    m, b = SIC.mask_expected("full")
    assert (m == 0).all() and (b == SR.D2_NONE).all()
    assert SIC.mask_expected("1x1_on")[1][0, 0] == SR.D2_NONE and SIC.mask_expected("1x1_off")[0][0, 0] == SR.D2_NONE


def test_corner_pixels():
    for name, (r0, c0) in {"corner_tl": (0, 0), "corner_tr": (0, 69), "corner_bl": (44, 0), "corner_br": (44, 69)}.items():
        r, c = np.mgrid[0:45, 0:70]
        m, b = SIC.mask_expected(name)
        assert np.array_equal(m, (r - r0) ** 2 + (c - c0) ** 2)
        assert b[r0, c0] == 1 and b.sum() == 1


def test_hand_answer_of_the_3x2_frame():
    m, b = SIC.mask_expected("hand_3x2")
    assert np.array_equal(m, SIC.HAND_D2_TO_MASK) and np.array_equal(b, SIC.HAND_D2_TO_BG)


def _same(got, ref):
    for k in SR.INTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in SR.FLOATS:
        assert np.float32(got[k]).tobytes() == np.float32(ref[k]).tobytes(), (k, got[k], ref[k])


@pytest.mark.parametrize("trunc", (0, 3))
def test_hand_answer_of_the_quad_half_over_a_rectangle(trunc):
    name = "hand_quad" if trunc == 0 else "hand_quad_trunc_3"
    got = SIC.expected(name)
    assert len(got) == 1
    print(name, got[0])
    _same(got[0], SIC.hand_quad_expected(trunc))
    on = SIC.hand_quad_mask() > 0
    assert int(SR.clip(SIC.case_maps(name)[1][on], trunc).sum()) == (15840 if trunc == 0 else 4192)


def _direct_miss(c, P, d2b):
    """sum_miss_d2 formed directly: over the mask pixels outside the visible model"""
    on = c["mask"] > 0
    _, visible = SR.pose_pixels(c["mesh"], P, c["K"], c["D"], c["tol"], c["amodal"])
    return int(SR.clip(d2b[on & ~visible], c["trunc"]).sum()), int((on & ~visible).sum())


@pytest.mark.parametrize("name", ("ragged", "trunc_3", "wall", "wall_amodal", "full_mask_trunc", "nan_zero_inf"))
def test_identities_of_the_record(name):
    c, recs = SIC.case(name), SIC.expected(name)
    for P, r in zip(c["poses"], recs):
        assert r["n_miss"] == r["n_mask"] - r["n_inter"] and r["n_visible"] == r["n_inter"] + r["n_spill"] <= r["n_model"]
        miss, n = _direct_miss(c, P, SIC.case_maps(name)[1])
        assert r["sum_miss_d2"] == miss and r["n_miss"] == n
        assert r["n_mask"] == int((c["mask"] > 0).sum())


def test_truncation():
    r0, r1, r3 = SIC.expected("ragged"), SIC.expected("trunc_1"), SIC.expected("trunc_3")
    for a, b, c in zip(r0, r1, r3):
        for k in ("n_model", "n_visible", "n_inter", "n_spill", "n_mask", "n_miss", "status", "iou"):
            assert a[k] == b[k] == c[k]
        # clipped to 1 every pixel of disagreement counts once: the sums are the counts
        assert b["sum_spill_d2"] == b["n_spill"] and b["sum_miss_d2"] == b["n_miss"]
        assert b["sum_spill_d2"] <= c["sum_spill_d2"] <= min(a["sum_spill_d2"], 9 * a["n_spill"])
        assert b["sum_miss_d2"] <= c["sum_miss_d2"] <= min(a["sum_miss_d2"], 9 * a["n_miss"])
    for k in ("sum_spill_d2", "sum_miss_d2"):                                                  # (the clip does bite, on some pose of the batch)
        print(k, [(a[k], c[k], b[k]) for a, b, c in zip(r0, r1, r3)])
        assert any(a[k] > c[k] > b[k] > 0 for a, b, c in zip(r0, r1, r3))


def test_amodal_equals_non_amodal_without_depth():
    c = SIC.case("ragged")
    zero = np.zeros_like(c["D"])
    a = SR.records(c["mesh"], c["poses"], c["K"], zero, c["mask"], c["tol"], 0, False, d2=SIC.case_maps("ragged"))
    b = SR.records(c["mesh"], c["poses"], c["K"], zero, c["mask"], c["tol"], 0, True, d2=SIC.case_maps("ragged"))
    assert a == b and a[0]["n_visible"] == a[0]["n_model"] > 500
    # ... and the amodal record does not depend on the depth at all
    assert b == SR.records(c["mesh"], c["poses"], c["K"], SIC.wall_depth(), c["mask"], c["tol"], 0, True, d2=SIC.case_maps("ragged"))


def test_a_wall_hides_half_the_model():
    c = SIC.case("wall")
    no_wall = SIC.case("ragged")["D"]                                            # the same depth without the wall
    frees = SR.records(c["mesh"], c["poses"], c["K"], no_wall, c["mask"], c["tol"], 0, False, d2=SIC.case_maps("wall"))
    for i, P in enumerate(c["poses"]):
        walled, free = SIC.expected("wall")[i], frees[i]
        _, seen = SR.pose_pixels(c["mesh"], P, c["K"], no_wall, c["tol"], False)
        hidden = seen & (np.arange(SIC.W)[None, :] <= 100)                       # what was visible and now lies behind the wall
        hidden_mask = int((hidden & (c["mask"] > 0)).sum())
        print(f"wall[{i}]: n_model {walled['n_model']}, visible {walled['n_visible']} of {free['n_visible']}, hidden mask pixels {hidden_mask}")
        assert walled["n_model"] == free["n_model"] and walled["n_visible"] == free["n_visible"] - int(hidden.sum()) < free["n_visible"]
        assert walled["n_miss"] == free["n_miss"] + hidden_mask > free["n_miss"]


@pytest.mark.parametrize("seed", SIC.SCENE_SEEDS)
def test_the_signal_on_the_scenes(seed):
    """at the truth the IoU is at least 0.98; moving the pose sideways by 2, 5, 10, 20 mm raises sum_spill_d2 + sum_miss_d2 strictly and lowers
    the IoU strictly"""
    s = SC.scene(seed)
    poses = [s.gt_pose] + [IC.moved(s.gt_pose, (mm * 1e-3, 0, 0)) for mm in SIC.SHIFTS_MM]
    recs = SR.records(SC.mesh(), poses, s.K, s.depth, s.mask, SIC.TOL, 0, False, d2=SIC.case_maps(f"scene_{seed}"))
    cost = [r["sum_spill_d2"] + r["sum_miss_d2"] for r in recs]
    iou = [float(r["iou"]) for r in recs]
    print(f"seed {seed}: iou {['%.4f' % v for v in iou]} cost {cost} at the truth: spill {recs[0]['n_spill']} miss {recs[0]['n_miss']}")
    assert iou[0] >= 0.98
    assert all(a < b for a, b in zip(cost, cost[1:])) and all(a > b for a, b in zip(iou, iou[1:]))


def test_the_abi_of_the_record():
    assert C.sizeof(_lib.FpPoseSilhouette) == 64
    assert tuple(n for n, _ in _lib.FpPoseSilhouette._fields_) == SR.FIELDS
    offsets = {n: getattr(_lib.FpPoseSilhouette, n).offset for n in SR.FIELDS}
    assert offsets["status"] == 24 and offsets["sum_spill_d2"] == 32 and offsets["sum_miss_d2"] == 40 and offsets["iou"] == 48
    body = re.search(r"typedef struct fp_pose_silhouette \{(.*?)\} fp_pose_silhouette_t;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(int32_t|int64_t|float)\s+", "", decl.strip()).split(",")]
    assert tuple(names) == SR.FIELDS

    def const(name):
        return int(re.search(rf"#define {name} (0x[0-9a-fA-F]+|\d+)", HEADER).group(1), 0)

    assert const("FP_SIL_AMODAL") == 1 and const("FP_SIL_D2_NONE") == SR.D2_NONE == 0x7FFFFFFF
    assert const("FP_SIL_MAX_DIM") == SR.MAX_DIM == 8192 and const("FP_SIL_MAX_TRUNC_PX") == SR.MAX_TRUNC_PX == 32767
    assert (const("FP_SIL_REFUSED_NEAR"), const("FP_SIL_REFUSED_RANGE"), const("FP_SIL_EMPTY")) == (SR.REFUSED_NEAR, SR.REFUSED_RANGE, SR.EMPTY) == (1, 2, 4)
    assert re.search(r"#define FP_SIL_MAX_WORK \d+LL", HEADER)
    for fn in ("fp_mask_distance", "fp_pose_silhouette"):
        assert fn in _lib.SYMBOLS and re.search(rf"\bint {fn}\(", HEADER)
