"""tests/pose_fit_ref.py on hand-built tensors with known answers, and the conditions tests/test_pose_fit_gpu.py relies on, checked with
the oracle alone (fo.render / fo.crop -> nn_in_ref.pack) so that the GPU tests cannot hide behind their fixtures: at the ground-truth pose
of every scene used there, with tol_m = 5 mm (five times the scenes' 1 mm depth noise), at least 90 % of the model pixels are inliers and
at most 2 % of them are uncertain under the oracle windows, in f16 and in bf16."""
import numpy as np
import pytest
import torch

import nn_in_ref as R
import pose_fit_ref as PF
from foundationpose_cpp_amd import synthetic as syn
from oracle import fp_oracle as fo

DTS = [R.F16, R.BF16]
NAME = {R.F16: "f16", R.BF16: "bf16"}
TOL_M = PF.TOL_M


def _images(dt, a_xyz, b_xyz, junk=False):
    """two nn_in images from per-pixel (x, y, z) arrays [160, 160, 3]; junk: fill rgb, the pad channels and the border with non-zeros"""
    blobs = np.zeros((2, 160, 160, 6), np.float32)
    blobs[0, ..., 3:], blobs[1, ..., 3:] = a_xyz, b_xyz
    if junk:
        blobs[..., :3] = 0.75
    t = R.pack(blobs, dt)
    if junk:
        inner = t[:, R.BORDER:-R.BORDER, R.BORDER:-R.BORDER].clone()
        inner = inner.reshape(2, 80, 80, 4, 8)
        inner[..., 6:] = 3.0                          # pad channels
        t[:] = -2.0                                   # border
        t[:, R.BORDER:-R.BORDER, R.BORDER:-R.BORDER] = inner.reshape(2, 80, 80, 32)
    return t


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_every_category_on_a_hand_built_tensor(dt):
    a = np.zeros((160, 160, 3), np.float32)
    b = np.zeros((160, 160, 3), np.float32)
    tol = np.float32(0.125)
    # rows 0-9: model at z = 0.5 (x = y = 0); row 10: model through x alone, row 11 through y alone (z = 0); the rest background
    a[0:10, :, 2] = 0.5
    a[10, :, 0] = 0.25
    a[11, :, 1] = -0.25
    b[0, :, 2] = 0.5             # inlier, d = 0
    b[1, :, 2] = 0.5625          # inlier, d = +1/16
    b[2, :, 2] = 0.625           # |d| == tol exactly: an inlier
    b[3, :, 2] = 0.375           # d == -tol exactly: an inlier
    b[4, :, 2] = 0.25            # front (d = -0.25)
    b[5, :, 2] = 1.0             # behind (d = +0.5)
    b[6, :, 0] = 0.5             # B.z == 0 with B.x != 0: not observed
    b[7, :, 2] = 0.0             # not observed
    b[8, :80, 2] = -0.5          # front (d = -1), half a row
    b[10, :, 2] = 0.0625         # model through x: d = 0.0625 - 0 -> inlier
    b[11, :, 2] = -1.0           # model through y: front
    b[20:30, :, 2] = 0.5         # depth where there is no model: ignored
    for junk in (False, True):
        t = _images(dt, a, b, junk)
        f = PF.pose_fit(t[0], t[1], tol, diameter=0.2)
        assert f.n_model == 12 * 160
        assert f.n_inlier == 5 * 160 and f.n_front == 160 + 80 + 160 and f.n_behind == 160
        assert f.n_observed == f.n_inlier + f.n_front + f.n_behind
        # d * 2^20 is exact for these values: (+1/16 + 1/8 - 1/8 + 1/16) * 160 rows
        assert f.sum_dz_q20 == 160 * (2 ** 16 + 2 ** 17 - 2 ** 17 + 2 ** 16)
        assert f.mean_dz_m == np.float32(f.sum_dz_q20 / 2 ** 20 / f.n_inlier * float(np.float32(0.2) / np.float32(2)))
    # nothing observed: no mean
    f = PF.pose_fit(t[0], torch.zeros_like(t[1]), tol, diameter=0.2)
    assert (f.n_model, f.n_observed, f.n_inlier, f.sum_dz_q20, float(f.mean_dz_m)) == (12 * 160, 0, 0, 0, 0.0)


def test_batch_layout_and_per_hypothesis_tolerance():
    a = np.zeros((160, 160, 3), np.float32)
    a[..., 2] = 0.5
    b = a.copy()
    b[..., 2] = 0.53125          # d = 1/32
    t = _images(R.F16, a, b)
    nn_in = torch.stack([t[0], t[0], t[1], t[1]])
    f = PF.pose_fit_batch(nn_in, 2, [0.0625, 0.015625], [0.2, 0.4])
    assert (f[0].n_inlier, f[0].n_behind) == (25600, 0) and (f[1].n_inlier, f[1].n_behind) == (0, 25600)
    assert float(f[0].mean_dz_m) == pytest.approx(0.1 / 32)
    assert PF.tol_n(0.005, 0.2) == np.float32(0.005) / np.float32(0.1)


def test_certain_counts_brackets_every_tensor_inside_the_windows():
    """the extremes of the windows, packed, give records inside [certain, certain + uncertain]"""
    rng = np.random.default_rng(0)
    ref_a = np.zeros((160, 160, 6), np.float32)
    ref_b = np.zeros((160, 160, 6), np.float32)
    ref_a[40:120, 40:120, 3:] = rng.uniform(-0.5, 0.5, (80, 80, 3))
    ref_b[30:110, 30:110, 5] = ref_a[30:110, 30:110, 5] + rng.choice([0.0, 0.03, 0.05, -0.2, 0.3], (80, 80))
    ref_b[60:64, :, 5] = 1e-6                       # window straddles zero
    tol = np.float32(0.05)
    for dt in DTS:
        c, unc = PF.certain_counts(ref_a, ref_b, dt, tol)
        assert unc > 0
        for da, db in ((-R.TOL, -R.TOL), (R.TOL, R.TOL), (-R.TOL, R.TOL), (R.TOL, -R.TOL), (0, 0)):
            t = R.pack(np.stack([np.where(ref_a != 0, ref_a + da, 0), np.where(ref_b != 0, ref_b + db, 0)]).astype(np.float32), dt)
            f = PF.pose_fit(t[0], t[1], tol)
            for k in PF.FIELDS:
                assert c[k] <= getattr(f, k) <= c[k] + unc, (NAME[dt], k, c[k], getattr(f, k), unc)


@pytest.mark.parametrize("crop_ratio", [1.2, 1.1])
def test_fixture_conditions_hold_under_the_oracle(syn_mesh, crop_ratio):
    om = fo.OracleMesh(syn_mesh)
    tol = PF.tol_n(TOL_M, syn_mesh.diameter)
    for name, scene in PF.gpu_scenes(syn_mesh):
        p16 = syn.to_colmajor(scene.gt_pose[None])
        hw = scene.depth.shape
        ra = fo.render(om, p16, scene.K, hw, crop_ratio)
        rb = fo.crop(scene.rgb, scene.depth, scene.K, p16, crop_ratio, syn_mesh.diameter)
        for dt in DTS:
            t = R.pack(np.concatenate([ra, rb]), dt)
            f = PF.pose_fit(t[0], t[1], tol, syn_mesh.diameter)
            c, unc = PF.certain_counts(ra[0], rb[0], dt, tol)
            print(f"{name} @{crop_ratio} {NAME[dt]}: {f.ints()} mean_dz {float(f.mean_dz_m) * 1e3:.3f} mm; certain {c}, uncertain {unc}")
            assert f.n_model > 2000, (name, f)
            assert f.n_inlier >= 0.9 * f.n_model, (name, NAME[dt], f)
            assert unc <= 0.02 * f.n_model, (name, NAME[dt], unc, f.n_model)
            for k in PF.FIELDS:
                assert c[k] <= getattr(f, k) <= c[k] + unc, (name, NAME[dt], k)
