"""The masks, meshes, frames and poses tests/test_silhouette_ref_cpu.py and the GPU tests of fp_mask_distance / fp_pose_silhouette share,
built without a GPU, and the hand answers.  The 200 x 150 frame (7 x 5 tiles of 32 px, ragged on both axes), the intrinsics and the
icospheres are those of tests/icp_cases.py, the scenes those of tests/search_cases.py.  References are computed once and shared; callers
must not modify them."""
import functools

import numpy as np

import icp_cases as IC
import search_cases as SC
import silhouette_ref as SR
from foundationpose_cpp_amd import synthetic as syn

f32 = np.float32
W, H, K = IC.W, IC.H, IC.K
TOL = 0.005
SCENE_SEEDS = SC.GPU_SEEDS                                        # 1, 11, 21, 31
SHIFTS_MM = (2, 5, 10, 20)                                        # gt_pose[0, 3] moved by these, for the signal

BEHIND = IC.moved(IC.ICO_G, (0, 0, -0.5))                        # behind the camera: refused, near
BEYOND = IC.pose(t=(20000.0, 0.0, 0.2))                          # 1e7 px to the right, every vertex beyond the near constant: refused, range
OUTSIDE = IC.moved(IC.ICO_G, (2.0, 0.0, 0.0))                    # wholly outside the frame


# ---- masks for the distance transform alone ------------------------------------------------------------------------------------------
def random_mask(h, w, density, seed):
    return np.where(np.random.default_rng(seed).uniform(size=(h, w)) < density, 255, 0).astype(np.uint8)


def one_pixel(h, w, r, c, value=255):
    m = np.zeros((h, w), np.uint8)
    m[r, c] = value
    return m


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """-> u8 [H,W].  The values of a mask pixel vary (1, 7, 255): the rule is byte > 0."""
    if name.startswith("random_"):                                # 45 x 70 at 0.5 %, 50 %, 99.5 %
        d = {"random_sparse": 0.005, "random_half": 0.5, "random_dense": 0.995}[name]
        m = random_mask(45, 70, d, 45 + int(d * 1000))
        return np.where(m > 0, np.random.default_rng(3).integers(1, 256, m.shape), 0).astype(np.uint8)
    if name == "empty":
        return np.zeros((45, 70), np.uint8)
    if name == "full":
        return np.full((45, 70), 1, np.uint8)
    if name.startswith("corner_"):
        r, c = {"corner_tl": (0, 0), "corner_tr": (0, 69), "corner_bl": (44, 0), "corner_br": (44, 69)}[name]
        return one_pixel(45, 70, r, c, 7)
    if name == "checkerboard":
        r, c = np.mgrid[0:45, 0:70]
        return np.where((r + c) % 2 == 0, 255, 0).astype(np.uint8)
    if name == "1x1_on":
        return np.full((1, 1), 255, np.uint8)
    if name == "1x1_off":
        return np.zeros((1, 1), np.uint8)
    if name == "1x9":
        return np.array([[0, 0, 255, 0, 0, 0, 0, 255, 255]], np.uint8)
    if name == "9x1":
        return np.array([[0, 0, 255, 0, 0, 0, 0, 255, 255]], np.uint8).T.copy()
    if name == "hand_3x2":
        return HAND_MASK
    # the GPU test's own: a row longer than a workgroup of the rows pass, W no multiple of 64; a scene's mask; one seed in the last pixel
    if name == "7x300":
        return random_mask(7, 300, 0.01, 7300)
    if name == "3x1300":
        m = random_mask(3, 1300, 0.002, 31300)
        m[1, 1299] = 255
        return m
    if name == "scene_mask":
        return SC.scene(SCENE_SEEDS[0]).mask
    if name == "last_pixel_64":
        return one_pixel(64, 64, 63, 63)
    raise KeyError(name)


CPU_MASKS = ("random_sparse", "random_half", "random_dense", "empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "checkerboard",
             "1x1_on", "1x1_off", "1x9", "9x1", "hand_3x2")
GPU_MASKS = CPU_MASKS + ("7x300", "3x1300", "scene_mask", "last_pixel_64")


@functools.lru_cache(maxsize=None)
def mask_expected(name):
    return SR.maps(mask_case(name))


# ---- poses against a mask -------------------------------------------------------------------------------------------------------------
def model_mask(mesh, P):
    """the mask a perfect segmenter gives the mesh under P: fp_render_pose's model_mask"""
    return np.where(IC.rendering(mesh, P) != IC.WALL, 255, 0).astype(np.uint8)


MASK_P = syn.perturb_pose(IC.ICO_G, deg=4.0, trans=0.004, seed=3)       # the pose the ico2 cases' mask shows


@functools.lru_cache(maxsize=None)
def ico2_mask():
    return model_mask(IC.ico(2), MASK_P)


def many_poses(n):
    """n poses of the 80-face icosphere around ICO_G, growing away from it; every 50th straddles the right edge, every 97th is wholly outside"""
    out = []
    for i in range(n):
        P = syn.perturb_pose(IC.ICO_G, deg=1.0 + 0.05 * i, trans=0.0004 * (i + 1), seed=100 + i)
        out.append(IC.moved(P, (0.33, 0, 0)) if i % 50 == 49 else IC.moved(P, (2.0, 0, 0)) if i % 97 == 96 else P)
    return np.stack(out)


def scene_poses(seed):
    """the truth of scene `seed` and seven poses growing away from it"""
    G = SC.scene(seed).gt_pose
    return np.stack([G] + [syn.perturb_pose(G, deg=1.0 * k, trans=0.002 * k, seed=seed + k) for k in range(1, 8)])


def wall_depth():
    """the rendering of ico2 under ICO_G with an occluding wall at 0.20 m over the left half of the frame (columns 0..100)"""
    D = IC.rendering(IC.ico(2), IC.ICO_G).copy()
    D[:, :101] = f32(0.20)
    return D


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(mesh, poses [N,4,4], K, D, mask, tol, trunc, amodal): the device records must equal silhouette_ref.records on each"""
    G = np.asarray(IC.ICO_G, f32)
    m2 = IC.ico(2)
    D2 = IC.rendering(m2, G)
    c = dict(mesh=m2, K=K, D=D2, mask=ico2_mask(), tol=TOL, trunc=0, amodal=False)
    if name.startswith("scene_"):                                 # 8 poses on a noisy scene against the scene's own mask
        s = SC.scene(int(name[6:]))
        c.update(mesh=SC.mesh(), poses=scene_poses(int(name[6:])), D=s.depth, mask=s.mask)
    elif name == "ragged":                                        # 7 poses: near, far off, one over the frame's edge, one wholly outside
        c.update(poses=IC.batch_poses(7))
    elif name in ("batch_47", "batch_512"):
        c.update(mesh=IC.ico(1), poses=many_poses(int(name[6:])))
    elif name == "nan_zero_inf":
        c.update(poses=np.stack([G, MASK_P]), D=SC.holes())
    elif name == "outside":
        c.update(poses=np.stack([OUTSIDE]))
    elif name == "outside_empty_mask":
        c.update(poses=np.stack([OUTSIDE, G]), mask=np.zeros((H, W), np.uint8))
    elif name == "refused":                                       # a near-refused and a range-refused pose between good ones
        c.update(poses=np.stack([G, BEHIND, IC.batch_poses(2)[1], BEYOND, G]))
    elif name in ("trunc_1", "trunc_3"):
        c.update(poses=IC.batch_poses(7), trunc=int(name[6:]))
    elif name == "wall":                                          # a wall in front of the left half
        c.update(poses=np.stack([G, MASK_P]), D=wall_depth())
    elif name == "wall_amodal":
        c.update(poses=np.stack([G, MASK_P]), D=wall_depth(), amodal=True)
    elif name == "empty_mask":
        c.update(poses=IC.batch_poses(3), mask=np.zeros((H, W), np.uint8))
    elif name == "full_mask":
        c.update(poses=IC.batch_poses(7), mask=np.full((H, W), 9, np.uint8))
    elif name == "full_mask_trunc":
        c.update(poses=IC.batch_poses(3), mask=np.full((H, W), 9, np.uint8), trunc=3)
    elif name in ("hand_quad", "hand_quad_trunc_3"):
        c.update(mesh=hand_quad(), poses=HAND_P[None], D=np.full((H, W), IC.WALL, f32), mask=hand_quad_mask(), trunc=3 if name.endswith("3") else 0)
    else:
        raise KeyError(name)
    return c


CASES = tuple(f"scene_{s}" for s in SCENE_SEEDS) + ("ragged", "batch_47", "batch_512", "nan_zero_inf", "outside", "outside_empty_mask", "refused",
                                                    "trunc_1", "trunc_3", "wall", "wall_amodal", "empty_mask", "full_mask", "full_mask_trunc",
                                                    "hand_quad", "hand_quad_trunc_3")


@functools.lru_cache(maxsize=None)
def case_maps(name):
    return SR.maps(case(name)["mask"])


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return SR.records(c["mesh"], c["poses"], c["K"], c["D"], c["mask"], c["tol"], c["trunc"], c["amodal"], d2=case_maps(name))


# ---- hand answers ------------------------------------------------------------------------------------------------------------------------
# (1) A frame of 2 rows and 3 columns whose only mask pixel is (row 0, column 2).  To the mask: the squared distances are (2 - c)^2 + r^2;
# to the background: every other pixel is background (0), and the mask pixel's nearest background pixel is its neighbour (1).
HAND_MASK = np.array([[0, 0, 255], [0, 0, 0]], np.uint8)
HAND_D2_TO_MASK = np.array([[4, 1, 0], [5, 2, 1]], np.int64)
HAND_D2_TO_BG = np.array([[0, 0, 1], [0, 0, 0]], np.int64)

# (2) A square of 0.12 m (two triangles) seen head-on at z = 1 m through f = 100 px, centre at the principal point (100, 75): corners at
# the pixels (94, 69) and (106, 81).  The top and the left edge belong to it, the bottom and the right edge do not, and the top-left rule
# gives every pixel of the shared diagonal to exactly one triangle: the pixels 94..105 x 69..80, 144 of them.  The depth is 1.5 m
# everywhere, behind the square: all 144 are visible.
# The mask is the rectangle of columns 100..119 and rows 60..89: 20 x 30 = 600 pixels.  The square's columns 100..105 lie on it (6 x 12 =
# 72 inter), its columns 94..99 do not (72 spill), and 600 - 72 = 528 mask pixels are missed.
#   spill: the rows 69..80 are rows of the mask, so the nearest mask pixel of (r, c) is (r, 100), 100 - c = 6, 5, 4, 3, 2, 1 away:
#          36 + 25 + 16 + 9 + 4 + 1 = 91 per row, 12 rows: 1 092
#   T:     a mask pixel is d = min(c - 99, 120 - c, r - 59, 90 - r) from the background; the ring at depth d has (22 - 2d)(32 - 2d) -
#          (20 - 2d)(30 - 2d) pixels: 96, 88, 80, 72, 64, 56, 48, 40, 32, 24 for d = 1..10 (600 in all), so
#          T = 96 + 88*4 + 80*9 + 72*16 + 64*25 + 56*36 + 48*49 + 40*64 + 32*81 + 24*100 = 15 840
#   inter: columns 100..105 are 1..6 from the left edge and the rows 69..80 at least 10 from the top and the bottom: d = c - 99, again 91
#          per row, 1 092; sum_miss_d2 = 15 840 - 1 092 = 14 748
#   iou = 72 / (600 + 72), rms_spill_px = sqrt(1092 / 72), rms_miss_px = sqrt(14748 / 528)
# With trunc_px = 3 every squared distance is clipped to 9: a row of spill or inter gives 9 + 9 + 9 + 9 + 4 + 1 = 41, 12 rows 492;
# T = 96 + 88*4 + (600 - 96 - 88)*9 = 4 192; sum_miss_d2 = 4 192 - 492 = 3 700.
HAND_P = IC.pose(t=(0.0, 0.0, 1.0))


def hand_quad():
    h = 0.06
    v = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], f32)
    n = np.tile(np.array([[0, 0, 1]], f32), (4, 1))
    return syn.Mesh("hand_quad", v, n, np.zeros((4, 2), f32), np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.full((2, 2, 3), 100, np.uint8)).finalize()


def hand_quad_mask():
    m = np.zeros((H, W), np.uint8)
    m[60:90, 100:120] = 255
    return m


def hand_quad_expected(trunc):
    spill, miss = (1092, 14748) if trunc == 0 else (492, 3700)
    r = dict(n_model=144, n_visible=144, n_inter=72, n_spill=72, n_mask=600, n_miss=528, status=0, sum_spill_d2=spill, sum_miss_d2=miss)
    r.update(iou=f32(72.0 / 672.0), rms_spill_px=f32(np.sqrt(spill / 72.0)), rms_miss_px=f32(np.sqrt(miss / 528.0)))
    return r
