"""The meshes, scenes and poses tests/test_search_ref_cpu.py and the GPU tests of fp_pose_search / fp_register_depth share, built without a
GPU.  The frame, the intrinsics and the icospheres are those of tests/icp_cases.py.  References are computed once and shared; callers
must not modify them."""
import functools

import numpy as np

import frame_render_ref as FR
import icp_cases as IC
import search_ref as SR
from foundationpose_cpp_amd import synthetic as syn

f32 = np.float32
W, H, K = IC.W, IC.H, IC.K
TOL = 0.005
SCENE_T = (0.01, -0.005, 0.35)
SCENE_SEEDS = (1, 11, 21, 31, 41, 51, 61, 71)          # rot_seed = s, noise / drop / bg seeds = s + 1, s + 2, s + 3
GPU_SEEDS = SCENE_SEEDS[:4]
TOP_K, ITERATIONS = 16, 15
# the ellipsoid's symmetries about its centre (beside the identity), as 4 x 4 matrices of the centred mesh's frame
SYMMETRIES = tuple(np.diag(np.array(d + (1,), np.float64)) for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1)))
# register_ref with the float64 ICP on the eight scenes (oracle grid of 252 poses, top_k 16, tol 5 mm, 15 iterations): MSSD over the 642
# vertices against the nearest of the four equivalents of the truth, in millimetres, measured on the CPU;
# tests/test_search_ref_cpu.py holds the reference to these
REF_MSSD_MM = {1: 0.805, 11: 0.370, 21: 0.407, 31: 0.641, 41: 0.524, 51: 0.396, 61: 1.155, 71: 0.785}
REF_SLACK_MM = 0.01                                   # what a recorded value may differ by on another numpy / BLAS
BOUND_M = 2 * max(REF_MSSD_MM.values()) * 1e-3      # the device: twice the reference's worst


def mesh():
    return IC.ico(3)


@functools.lru_cache(maxsize=None)
def scene(seed):
    return syn.make_scene(mesh(), W=W, H=H, t=SCENE_T, rot_seed=seed, noise_seed=seed + 1, drop_seed=seed + 2, bg_seed=seed + 3)


def step_of(m):
    return f32(m.diameter) / f32(16)


def mssd_sym(m, P, G):
    """MSSD of P against the best of G's four equivalents, over the centred vertices, in float64"""
    v = FR.centred(m).astype(np.float64)
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    a = v @ P[:3, :3].T + P[:3, 3]
    best = np.inf
    for S in (np.eye(4),) + SYMMETRIES:
        Q = G @ S
        best = min(best, float(np.linalg.norm(a - (v @ Q[:3, :3].T + Q[:3, 3]), axis=1).max()))
    return best


@functools.lru_cache(maxsize=None)
def cloud(n):
    """a random point cloud as a "mesh": n vertices in a 10 x 8 x 12 cm box with random unit normals and one face"""
    rng = np.random.default_rng(n)
    v = (rng.uniform(-1, 1, (n, 3)) * np.array([0.05, 0.04, 0.06])).astype(f32)
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(f32)
    return syn.Mesh(f"cloud{n}", v, nn, np.zeros((n, 2), f32), np.array([[0, 1, 2]], np.int32), np.full((2, 2, 3), 100, np.uint8)).finalize()


def mesh_of(name):
    return cloud(int(name[5:])) if name.startswith("cloud") else IC.mesh_of(name)


HOLES = {"nan": (slice(62, 74), slice(90, 102), np.nan), "zero": (slice(74, 86), slice(102, 114), 0.0), "inf": (slice(62, 74), slice(102, 114), np.inf)}


def holes(kinds=("nan", "zero", "inf")):
    """the rendering of ico2 under ICO_G with a 12 x 12 px block of each of `kinds` on the object, where facing points project"""
    D = IC.rendering(IC.ico(2), IC.ICO_G).copy()
    for k in kinds:
        rows, cols, value = HOLES[k]
        D[rows, cols] = value
    return D


def _rot_pose(seed, t=SCENE_T):
    return IC.pose(syn.random_rotation(seed), t)


@functools.lru_cache(maxsize=None)
def record_case(name):
    """-> (mesh name, poses [N,4,4], depth, n_steps, step_m, vertex_step): the device records must equal search_ref.records on each"""
    m2 = IC.ico(2)
    G = IC.ICO_G
    D = IC.rendering(m2, G)
    d16 = step_of(m2)
    if name == "batch":                      # 7 poses x 4 steps: near, far off, one over the frame's edge, one wholly outside
        return "ico2", IC.batch_poses(7), D, 4, d16, 1
    if name == "edge":
        return "ico2", np.stack([IC.moved(G, (0.33, 0.0, 0.0))]), D, 4, d16, 1
    if name == "outside":
        return "ico2", np.stack([IC.moved(G, (2.0, 0.0, 0.0))]), D, 4, d16, 1
    if name == "plate_in_front":             # everything the camera sees is 0.20 m away: every facing point is front
        return "ico2", np.stack([np.asarray(G, f32)]), np.full((H, W), f32(0.20)), 4, d16, 1
    if name == "nan_zero_inf":
        return "ico2", np.stack([np.asarray(G, f32)]), holes(), 4, d16, 1
    if name == "near_step":                  # the long axis towards the camera, 9 cm away: step 0 has points behind the near plane, step 1 has not
        return "ico2", np.stack([IC.pose(t=(0.0, 0.0, 0.09)), IC.pose(t=(0.004, 0.002, 0.10))]), D, 4, f32(0.03), 1
    if name == "all_refused":
        return "ico2", np.stack([IC.pose(t=(0.0, 0.0, 0.02)), np.asarray(G, f32)]), D, 2, f32(0.01), 1
    if name == "cloud257":                   # two rounds of the 256-thread loop, the second with one point
        return "cloud257", np.stack([_rot_pose(3), _rot_pose(4, (0.3, 0.0, 0.35))]), D, 3, f32(0.01), 1
    if name == "cloud4096":                  # the cap: sixteen full rounds
        return "cloud4096", np.stack([_rot_pose(5), _rot_pose(6)]), D, 3, f32(0.01), 1
    if name == "one_step":
        return "ico2", IC.batch_poses(3), D, 1, d16, 1
    if name == "max_steps":                  # 6 cm too near: a step around 30 wins
        return "ico2", np.stack([IC.moved(P, (0.0, 0.0, -0.06)) for P in IC.batch_poses(3)]), D, 64, f32(0.002), 1
    if name == "vertex_step_3":              # 642 vertices: 214 points
        return "ico3", np.stack([np.asarray(G, f32), syn.perturb_pose(G, deg=20.0, trans=0.01, seed=8)]), IC.rendering(IC.ico(3), G), 4, d16, 3
    if name == "zero_step":                  # step_m = 0: every step is the pose itself, the lowest wins
        return "ico2", IC.batch_poses(2), D, 3, f32(0.0), 1
    raise KeyError(name)


RECORD_CASES = ("batch", "edge", "outside", "plate_in_front", "nan_zero_inf", "near_step", "all_refused", "cloud257", "cloud4096", "one_step",
                "max_steps", "vertex_step_3", "zero_step")


@functools.lru_cache(maxsize=None)
def classified(name):
    mname, poses, D, n_steps, step_m, vstep = record_case(name)
    m = mesh_of(mname)
    return SR.classify(FR.centred(m), SR.normals_of(m), poses, K, D, n_steps, step_m, TOL, vstep)


@functools.lru_cache(maxsize=None)
def expected(name):
    return SR.summarise(*classified(name))
