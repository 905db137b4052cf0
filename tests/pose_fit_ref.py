"""Host reference of the pose fit (include/foundationpose_amd.h, fp_pose_fit) as a pure function of the networks'
input tensor nn_in (tests/nn_in_ref.py: [NB, 84, 84, 32] in a 2-byte type, channels r g b x y z 0 0 per pixel) and the f32 threshold tol_n.

Per crop pixel, A = the rendered image, B = the observed one, element values widened exactly to f32:
  model     (A.x, A.y, A.z) != (0, 0, 0)
  observed  model and B.z != 0
  d         B.z - A.z, one f32 subtraction
  inlier    observed and |d| <= tol_n;  front: observed and d < -tol_n;  behind: observed and d > tol_n
  sum_dz_q20 = sum over inliers of (int64) rint(d * 2^20)
The border and the two pad channels are never read.  `certain_counts` is the same classification over INTERVALS of values (the windows of
nn_in_ref.window around the oracle's f32 tensors): what every tensor inside the windows must give, and how many pixels are open."""
import dataclasses

import numpy as np
import torch

import nn_in_ref as R
from foundationpose_cpp_amd import synthetic as syn

TOL_M = 0.005      # the tests' threshold: five times the synthetic scenes' 1 mm depth noise


def gpu_scenes(mesh):
    """the scenes tests/test_pose_fit_gpu.py uses at their ground-truth poses; tests/test_pose_fit_ref_cpu.py holds them to the fixture
    conditions with the oracle alone"""
    return [("make_scene", syn.make_scene(mesh))] + [(f"heldout {i}", s) for i, s in enumerate(syn.heldout_scenes(mesh, 2))]


Q20 = np.float32(1048576.0)
FIELDS = ("n_model", "n_observed", "n_inlier", "n_front", "n_behind")


@dataclasses.dataclass
class Fit:
    n_model: int
    n_observed: int
    n_inlier: int
    n_front: int
    n_behind: int
    sum_dz_q20: int
    mean_dz_m: np.float32
    tol_n: np.float32

    def ints(self):
        return tuple(getattr(self, f) for f in FIELDS) + (self.sum_dz_q20,)


def tol_n(tol_m, diameter):
    """(float)tol_m / ((float)diameter / 2), in f32"""
    return np.float32(tol_m) / (np.float32(diameter) / np.float32(2))


def mean_dz_m(sum_dz_q20, n_inlier, diameter):
    """sum_dz_q20 / 2^20 / n_inlier * diam/2 in double, stored as f32; 0 without inliers"""
    if n_inlier == 0:
        return np.float32(0)
    return np.float32(float(sum_dz_q20) / 1048576.0 / float(n_inlier) * float(np.float32(diameter) / np.float32(2)))


def _xyz(img):
    """one image [84, 84, 32] (any float element type) -> x, y, z [160, 160] f32, exact"""
    blobs, _, _ = R.blobs_from_nn_in(torch.as_tensor(img)[None])
    b = blobs[0].to(torch.float32).numpy()
    return b[..., 3], b[..., 4], b[..., 5]


def pose_fit(img_a, img_b, tol, diameter=None):
    """the record of one hypothesis: img_a / img_b = its rendered / observed image of nn_in, tol = tol_n (f32)"""
    tol = np.float32(tol)
    ax, ay, az = _xyz(img_a)
    _, _, bz = _xyz(img_b)
    model = (ax != 0) | (ay != 0) | (az != 0)
    observed = model & (bz != 0)
    d = (bz - az).astype(np.float32)
    assert d.dtype == np.float32
    inlier = observed & (np.abs(d) <= tol)
    front = observed & (d < -tol)
    behind = observed & (d > tol)
    q = np.rint(d * Q20).astype(np.int64)
    s = int(q[inlier].sum(dtype=np.int64))
    n_in = int(inlier.sum())
    return Fit(int(model.sum()), int(observed.sum()), n_in, int(front.sum()), int(behind.sum()), s,
               mean_dz_m(s, n_in, diameter) if diameter is not None else np.float32(0), tol)


def pose_fit_batch(nn_in, n, tol, diameter=None, b_of=None):
    """records of hypotheses 0..n-1 of a tapped tensor: image i against image b_of(i) (default n + i, Register's and Track's layout);
    tol / diameter: one value or one per hypothesis"""
    tols = np.broadcast_to(np.asarray(tol, np.float32), (n,))
    diams = [None] * n if diameter is None else np.broadcast_to(np.asarray(diameter, np.float32), (n,))
    return [pose_fit(nn_in[i], nn_in[b_of(i) if b_of else n + i], tols[i], diams[i]) for i in range(n)]


def certain_counts(ref_a, ref_b, dt, tol):
    """ref_a / ref_b: the oracle's f32 blobs [160, 160, 6] of one hypothesis.  Every value the device may store lies in the window of
    nn_in_ref.window around the oracle's; a pixel is CERTAIN when its class -- not model / model but not observed / inlier / front /
    behind -- is the same for every choice of values inside the windows.  -> ({field: count over the certain pixels}, number of uncertain pixels)"""
    tol = np.float32(tol)

    def win(ref):
        # An oracle value of exactly 0 is structural -- background, a pixel without valid depth, a thresholded channel -- not a rounded
        # number: the device has to store 0 there too, so its window is [0, 0] (with nn_in_ref's +-2e-6 around it every background pixel
        # could be a model pixel and nothing would be certain).  This only narrows the windows: the bounds below get tighter, never wider.
        lo, hi = (w.numpy() for w in R.window(ref, dt))
        z = np.asarray(ref) == 0
        return np.where(z, 0.0, lo), np.where(z, 0.0, hi)
    (lo_a, hi_a), (lo_b, hi_b) = win(ref_a[..., 3:6]), win(ref_b[..., 5])
    zero_a = ((lo_a == 0) & (hi_a == 0)).all(-1)                       # every channel can only be 0
    nonzero_a = ((lo_a > 0) | (hi_a < 0)).any(-1)                      # some channel cannot be 0
    zero_b, nonzero_b = (lo_b == 0) & (hi_b == 0), (lo_b > 0) | (hi_b < 0)
    # d is monotone in B.z and in -A.z, and the f32 subtraction is monotone too: its range over the windows is spanned by the corners
    d_lo = (lo_b.astype(np.float32) - hi_a[..., 2].astype(np.float32)).astype(np.float32)
    d_hi = (hi_b.astype(np.float32) - lo_a[..., 2].astype(np.float32)).astype(np.float32)
    inl = (np.abs(d_lo) <= tol) & (np.abs(d_hi) <= tol)
    fro = d_hi < -tol
    beh = d_lo > tol
    obs_certain = nonzero_a & nonzero_b & (inl | fro | beh)
    certain = zero_a | (nonzero_a & zero_b) | obs_certain
    c = {"n_model": int((certain & nonzero_a).sum()), "n_observed": int(obs_certain.sum()), "n_inlier": int((obs_certain & inl).sum()),
         "n_front": int((obs_certain & fro).sum()), "n_behind": int((obs_certain & beh).sum())}
    return c, int((~certain).sum())
