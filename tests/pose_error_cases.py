"""The meshes and poses tests/test_pose_error_gpu.py hands to fp_pose_errors, built without a GPU so that tests/test_pose_error_ref_cpu.py
can hold each to what it is for before a kernel sees it.  Point sets only: the faces are one degenerate triangle (the call never reads
them).  References are computed once and shared; callers must not modify them."""
import functools

import numpy as np

import pose_error_ref as PR
from foundationpose_cpp_amd import synthetic as syn

K = syn.intrinsics()                      # fx = fy = 320, cx = 320, cy = 240
BOX_HALF = (0.10, 0.075, 0.05)
BOX_OFFSET = (0.03, -0.02, 0.05)          # a non-zero mesh centre: the symmetries have to be conjugated


def point_mesh(name, points, diameter=0.0):
    v = np.asarray(points, np.float32).reshape(-1, 3)
    n = np.tile(np.array([0, 0, 1], np.float32), (len(v), 1))
    return syn.Mesh(name, v, n, np.zeros((len(v), 2), np.float32), np.zeros((1, 3), np.int32), np.full((2, 2, 3), 100, np.uint8),
                    diameter=diameter).finalize()


def centred(mesh):
    """the vertices the library keeps: mesh frame minus the mesh centre, one f32 subtraction"""
    return mesh.vertices.astype(np.float32) - np.asarray(mesh.center, np.float32)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * X + (1 - np.cos(angle)) * (X @ X)


def rigid(R, t=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def about(T, centre):
    """the transform T (given about the origin) carried out about `centre`: T(c) T T(-c)"""
    return rigid(np.eye(3), centre) @ T @ rigid(np.eye(3), -np.asarray(centre, np.float64))


def f32(T):
    """what the library is handed: the matrices rounded to f32 (the reference reads the same values)"""
    return np.asarray(T, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def box():
    """the 7 x 6 x 5 lattice on the surface of a box with half-extents BOX_HALF: V = 150, invariant under the three 180 degree axis
    rotations about its centre; moved by BOX_OFFSET in the mesh frame"""
    g = np.stack(np.meshgrid(*[np.linspace(-h, h, n) for h, n in zip(BOX_HALF, (7, 6, 5))], indexing="ij"), -1).reshape(-1, 3)
    surface = (np.abs(np.abs(g) - np.array(BOX_HALF)) < 1e-12).any(1)
    return point_mesh("box", g[surface] + np.array(BOX_OFFSET))


@functools.lru_cache(maxsize=None)
def box_symmetries():
    """mesh frame, as BOP's models_info.json would list them: 180 degrees about x, y, z through the box's centre"""
    c = np.asarray(box().center, np.float64)
    return f32(np.stack([about(rigid(rot(ax, np.pi)), c) for ax in np.eye(3)]))


@functools.lru_cache(maxsize=None)
def box_poses():
    """E at about 0.45 m; G_k = E delta S_k^-1 (S_k about the CENTRED origin: S_0 = I), delta = 0.02 rad / 2 mm -> (E, [G_0..G_3])"""
    E = rigid(syn.random_rotation(21), (0.04, -0.03, 0.45))
    delta = rigid(rot((1.0, 2.0, -1.0), 0.02), np.array([1.0, -1.0, 1.0]) * 0.002 / np.sqrt(3.0))
    S = [np.eye(4)] + [rigid(rot(ax, np.pi)) for ax in np.eye(3)]
    return f32(E), f32(np.stack([E @ delta @ np.linalg.inv(s) for s in S]))


@functools.lru_cache(maxsize=None)
def cloud257():
    """257 points, sigma = (0.1, 0.03, 0.01) m, 40 of them shifted by 0.3 m: the two directions of ADD-S differ"""
    rng = np.random.default_rng(257)
    p = rng.normal(size=(257, 3)) * np.array([0.1, 0.03, 0.01])
    p[:40, 0] += 0.3
    return point_mesh("cloud", p)


@functools.lru_cache(maxsize=None)
def cloud257_poses():
    E = rigid(syn.random_rotation(31), (-0.05, 0.02, 0.8))
    G = E @ rigid(rot((0.2, 1.0, 0.4), 0.35), (0.01, -0.02, 0.015))
    return f32(E), f32(G)


NN_SHIFT = np.array([0.04, -0.035, 0.03])      # the ground truth of ragged() is the estimate moved by this, in the object frame


@functools.lru_cache(maxsize=None)
def ragged_mesh(V, step):
    """V seeded points within 0.09 m; the two vertices in the middle coincide (V > 2); the LAST min(8, Vs // 4) used vertices are
    the first used vertices moved by NN_SHIFT, so for the poses of ragged() their nearest neighbours lie at the very end of the
    target set -- in the last, partial tile"""
    rng = np.random.default_rng(1000 + 7 * V + step)
    p = rng.uniform(-1, 1, size=(V, 3))
    p = p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1.0) * 0.09
    if V > 2:
        p[V // 2] = p[V // 2 - 1]
    used = np.arange(0, V, step)
    for j in range(min(8, len(used) // 4)):
        p[used[-1 - j]] = p[used[j]] + NN_SHIFT
    return point_mesh(f"ragged{V}_{step}", p + np.array([0.01, 0.02, -0.03]))


def ragged_symmetries(mesh, S):
    """S mesh-frame transforms: rotations by multiples of 360 / (S + 1) degrees about an axis through the mesh centre (these clouds have
    no symmetry: the transforms only have to be handled)"""
    c = np.asarray(mesh.center, np.float64)
    return f32(np.stack([about(rigid(rot((0.3, -0.5, 1.0), 2 * np.pi * (k + 1) / (S + 1))), c) for k in range(S)])) if S else None


def ragged_poses(N, n_gt, seed):
    """N estimates at 0.4 .. 0.9 m; ground truth i = estimate i (n_gt == N) or estimate 0 (n_gt == 1) moved by NN_SHIFT and 0.02 rad"""
    rng = np.random.default_rng(seed)
    est = np.stack([rigid(syn.random_rotation(seed * 100 + i), (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 0.9))) for i in range(N)])
    move = rigid(rot((1.0, 0.5, -0.2), 0.02), NN_SHIFT)
    gt = np.stack([e @ move for e in est[:n_gt]])
    return f32(est), f32(gt)


# (V, N, S, n_gt is N, vertex_step): every V, N, S, n_gt kind and step of the list the test has to cover, V around the 1024-point target
# tile at step 1, and the small V with many poses, where the 64 items of a wave belong to many poses
RAGGED = [(1, 1, 0, True, 1), (1, 65, 1, False, 1), (2, 65, 0, True, 1), (2, 3, 7, False, 2), (63, 3, 1, True, 1), (64, 1, 7, True, 3),
          (65, 65, 0, False, 7), (65, 3, 0, True, 2), (1023, 3, 1, True, 1), (1024, 1, 0, True, 1), (1025, 3, 0, False, 1),
          (1025, 1, 7, True, 3), (1025, 65, 0, True, 7)]


@functools.lru_cache(maxsize=None)
def ragged(V, N, S, paired, step):
    """-> (mesh, est, gt, symmetries, reference records)"""
    mesh = ragged_mesh(V, step)
    est, gt = ragged_poses(N, N if paired else 1, V + N)
    sym = ragged_symmetries(mesh, S)
    return mesh, est, gt, sym, PR.pose_errors(centred(mesh), mesh.center, K, est, gt, sym, step)
