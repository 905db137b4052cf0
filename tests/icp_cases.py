"""The meshes, scenes and poses tests/test_icp_ref_cpu.py and the GPU tests of fp_refine_depth share, built without a GPU.  A 200 x 150
frame (7 x 5 tiles of 32 px, ragged on both axes) with f = 100 px.  References are computed once and shared; callers must not modify
them."""
import functools

import numpy as np

import frame_render_ref as FR
import icp_ref as IR
from foundationpose_cpp_amd import synthetic as syn

W, H = 200, 150
K = syn.intrinsics(W, H)                 # fx = fy = 100, cx = 100, cy = 75
GATE = 0.02
WALL = np.float32(1.5)
SCENE_T = (0.01, -0.005, 0.35)
SCENE_SEEDS = (1, 11, 21, 31)
STARTS = ((5.0, 0.010), (8.0, 0.015))    # perturb_pose: degrees, metres
# what the float64 ICP (b) reaches on the four scenes with the subdiv-4 mesh, measured on the CPU: at worst
# 0.338 deg / 0.455 mm from the ground truth, above the 0.3 mm of the analytic-ellipsoid prototype, so the bound is twice (b)'s own worst
GT_BOUND_DEG, GT_BOUND_M = 2 * 0.338, 2 * 0.455e-3
# the iteration on (a)'s sums against (b), measured on the CPU over the four scenes and both starts: at worst 0.0557 deg / 0.0278 mm
# apart after 10 iterations (the 1 mm depth noise keeps both in a small cycle around the fixed point, the 1/16 px snap and f32 put them
# at different places of it), above 0.02 deg / 0.02 mm, so the device is held to twice the measured value
AB_BOUND_DEG, AB_BOUND_M = 2 * 0.0557, 2 * 0.0278e-3


@functools.lru_cache(maxsize=None)
def plate():
    """a square plate of 8 cm in the mesh's xy plane: two triangles"""
    h = 0.04
    v = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32)
    n = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    return syn.Mesh("plate", v, n, np.zeros((4, 2), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.full((2, 2, 3), 100, np.uint8)).finalize()


@functools.lru_cache(maxsize=None)
def ico(subdiv):
    return syn.make_mesh(subdiv, textured=False, name=f"ico{subdiv}")


def mesh_of(name):
    return plate() if name == "plate" else ico(int(name[3:]))


def pose(R=np.eye(3), t=(0, 0, 0)):
    return syn.pose_matrix(np.asarray(R, np.float64), t)


def moved(P, dt):
    Q = np.array(P, np.float32)
    Q[:3, 3] += np.asarray(dt, np.float32)
    return Q


def rendering(mesh, P, background=WALL):
    """fp_render_pose's own model_depth of the mesh under P, the background at `background`"""
    cam, snap, near, far = FR.project(FR.centred(mesh), np.asarray(P, np.float32), K)
    assert not near.any() and not far.any()
    keys = FR.rasterize(cam, snap, FR.stored_faces(FR.centred(mesh), mesh.faces), H, W)
    z = np.where(keys != FR.EMPTY, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(background))
    return np.ascontiguousarray(z, np.float32)


PLATE_Z0 = 0.30
PLATE_G = pose(t=(0.0, 0.0, PLATE_Z0))
PLATE_D = np.full((H, W), np.float32(PLATE_Z0) + np.float32(0.003), np.float32)
ICO_G = pose(syn.random_rotation(4), (0.01, -0.005, 0.35))          # inside the frame


@functools.lru_cache(maxsize=None)
def scene(seed):
    """the noisy scene of the issue: 1 mm depth noise, 2 % dropped pixels; the depth is the ANALYTIC ellipsoid's"""
    return syn.make_scene(ico(4), W=W, H=H, t=SCENE_T, rot_seed=seed, noise_seed=seed)


@functools.lru_cache(maxsize=None)
def start(seed, k):
    deg, trans = STARTS[k]
    return syn.perturb_pose(scene(seed).gt_pose, deg=deg, trans=trans)


@functools.lru_cache(maxsize=None)
def refined64(seed, k):
    """(b) from start k on scene `seed`: gate 0.02 m, 10 iterations"""
    return IR.icp64(ico(4), start(seed, k), K, scene(seed).depth, GATE, 10)


@functools.lru_cache(maxsize=None)
def record_case(name):
    """the I = 0 cases of the GPU test -> (mesh name, pose, depth): each is held to (a) exactly"""
    m = ico(2)
    G = ICO_G
    E = syn.perturb_pose(G, deg=4.0, trans=0.004, seed=3)
    if name == "inside":
        return "ico2", E, rendering(m, G)
    if name == "edge":                       # straddling the frame's right edge
        Ge = moved(G, (0.33, 0.0, 0.0))
        return "ico2", syn.perturb_pose(Ge, deg=3.0, trans=0.003, seed=4), rendering(m, Ge)
    if name == "outside":                    # wholly outside: every count 0
        return "ico2", moved(G, (2.0, 0.0, 0.0)), rendering(m, G)
    if name == "plate_in_front":             # an occluding plate at 0.20 m, 5 cm in front of the nearest point the object can reach, over the left half of the frame
        D = rendering(m, G)
        D[:, :101] = np.float32(0.20)
        return "ico2", E, D
    if name == "nan_and_zero":
        D = rendering(m, G)
        D[70:76, 95:101] = np.nan
        D[76:82, 101:107] = 0.0
        D[60, 100] = np.inf
        return "ico2", E, D
    if name == "ico3":                       # 1 280 faces: five rounds of the 256-thread stride
        m3 = ico(3)
        return "ico3", syn.perturb_pose(G, deg=6.0, trans=0.006, seed=5), rendering(m3, G)
    raise KeyError(name)


RECORD_CASES = ("inside", "edge", "outside", "plate_in_front", "nan_and_zero", "ico3")


@functools.lru_cache(maxsize=None)
def expected(name):
    mesh, P, D = record_case(name)
    m = mesh_of(mesh)
    return IR.sums(FR.centred(m), m.faces, P, K, D, GATE, m.diameter)


def batch_poses(n=7):
    """mixed poses around ICO_G: near, far off, partly outside"""
    out = []
    for i in range(n):
        P = syn.perturb_pose(ICO_G, deg=2.0 + 1.5 * i, trans=0.002 * (i + 1), seed=40 + i)
        out.append(moved(P, (0.33, 0, 0)) if i == 3 else moved(P, (2.0, 0, 0)) if i == 5 else P)
    return np.stack(out)
