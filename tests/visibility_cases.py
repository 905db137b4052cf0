"""Meshes and poses for the visibility rules of tests/visibility_ref.py.  Every other mesh of the suite is
star-shaped: nothing on it hides anything but its own back side.  These are not:

    torus_plate   a 32 x 16 torus (R 0.06, r 0.025) and an OPEN 9 x 9-vertex plate through its hole, tilted (z = 0.35 x + 0.011) so that it cuts
                  the tube where no edge of either lies: concave, self-occluding, interpenetrating, with boundary edges and a surface seen
                  from behind.  Five poses, two of them across the near plane (t_z = 0.14, and t_z = 0.09 with vertices behind the camera)
    fine          a coarse 3 x 3-vertex back plate (+- 0.07 m) and, 1 cm in front of it, a 49 x 49-vertex patch of 0.5 mm cells (about 1/3 px: the
                  snap to 1/16 px collapses many), one triangle with a repeated index and one with collinear corners
    plates_a / b  two parallel quads 1 mm apart, the farther one listed first / last, seen from both sides

and the frame-resolution cases put torus_plate and fine on a 160 x 120 frame with fx != fy.  Faces wind so that (p1 - p0) x (p2 - p0) points
out of the torus."""
import dataclasses
import functools

import numpy as np

import test_shade_warp_ref_cpu as C
from foundationpose_cpp_amd import synthetic as syn

NEW_CASES = ["torus_plate", "fine", "plates_a", "plates_b"]
OLD_CASES = C.CPU_CASES + ["edge"]
CLOSED_CASES = [f"rnd{i}" for i in range(12)] + ["ellipsoid"]          # closed surfaces: a foreground pixel has a front and a back
NEAR_POSES = {"torus_plate": (3, 4), "edge": (1, 2)}                    # the poses that cross the near plane
GPU_CASES = ["torus_plate", "fine", "plates_a", "plates_b", "edge", "rnd1", "rnd5"]


def _grid_faces(nu, nv, wrap_u=False, wrap_v=False, base=0):
    """two triangles per cell of an nu x nv vertex grid (vertex (i, j) = base + i * nv + j), (00, 10, 11) and (00, 11, 01)"""
    f = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            i1, j1 = (i + 1) % nu, (j + 1) % nv
            a, b, c, d = base + i * nv + j, base + i1 * nv + j, base + i1 * nv + j1, base + i * nv + j1
            f += [(a, b, c), (a, c, d)]
    return f


def _plate(n, half, z):
    """n x n vertices on [-half, half]^2, z = z(x, y)"""
    g = np.linspace(-half, half, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x, y, z(x, y)], -1).reshape(-1, 3)


def _mesh(name, v, n, faces):
    uv = (v[:, :2] - v[:, :2].min(0)) / np.ptp(v[:, :2], axis=0)
    tex = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    return syn.Mesh(name, v.astype(np.float32), n.astype(np.float32), uv.astype(np.float32), np.array(faces, np.int32), tex).finalize()


@functools.lru_cache(maxsize=None)
def torus_plate_mesh():
    R, r, nu, nv = 0.06, 0.025, 32, 16
    th, ph = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    tv = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1).reshape(-1, 3)
    tn = np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], -1).reshape(-1, 3)
    pv = _plate(9, 0.08, lambda x, y: 0.35 * x + 0.011)
    pn = np.tile(np.array([-0.35, 0.0, 1.0]) / np.hypot(0.35, 1.0), (len(pv), 1))
    faces = _grid_faces(nu, nv, True, True) + _grid_faces(9, 9, base=len(tv))
    return _mesh("torus_plate", np.concatenate([tv, pv]), np.concatenate([tn, pn]), faces)


@functools.lru_cache(maxsize=None)
def fine_mesh():
    back = _plate(3, 0.07, lambda x, y: 0.01 + 0 * x)
    patch = _plate(49, 0.012, lambda x, y: 0 * x)                      # 48 cells of 0.5 mm
    v = np.concatenate([back, patch])
    faces = _grid_faces(3, 3) + _grid_faces(49, 49, base=9)
    p = lambda i, j: 9 + i * 49 + j
    faces.append((p(10, 10), p(10, 10), p(30, 40)))                    # a repeated index
    faces.append((p(20, 5), p(20, 6), p(20, 8)))                       # three vertices of one grid line: x equal, z equal -> collinear after centring
    return _mesh("fine", v, np.tile([0.0, 0.0, -1.0], (len(v), 1)), faces)


def plates_mesh(far_first):
    q = lambda z: np.array([[-0.05, -0.05, z], [0.05, -0.05, z], [0.05, 0.05, z], [-0.05, 0.05, z]])
    near, far = q(0.0), q(0.001)                                       # (near / far for a camera on the -z side)
    v = np.concatenate([far, near] if far_first else [near, far])
    faces = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
    return _mesh("plates_a" if far_first else "plates_b", v, np.tile([0.0, 0.0, -1.0], (8, 1)), faces)


def _poses(*rt):
    return np.stack([syn.pose_matrix(C._rot(*a), t) for a, t in rt]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """a C.Case; the names of tests/test_shade_warp_ref_cpu.py are passed on"""
    if name not in NEW_CASES:
        return C.case(name)
    K = syn.intrinsics()
    hw = (480, 640)
    rgb, depth = np.zeros(hw + (3,), np.uint8), np.zeros(hw, np.float32)
    if name == "torus_plate":
        mesh = torus_plate_mesh()
        poses = _poses(((55, 20, 10), (0.03, -0.02, 0.5)), ((-130, 35, 70), (-0.1, 0.05, 1.2)), ((20, -60, -40), (0.4, 0.3, 3.0)),
                       ((65, 25, 5), (0.01, 0.0, 0.14)), ((75, -50, 30), (0.0, 0.01, 0.09)))
        z = (np.asarray(mesh.vertices - mesh.center, np.float64) @ poses[4, :3, :3].astype(np.float64).T)[:, 2] + 0.09
        assert z.min() < 0 < 0.1 < z.max()                             # vertices behind the camera, others in front of the near plane
    elif name == "fine":
        mesh = fine_mesh()
        poses = _poses(((0, 0, 0), (0.003, -0.002, 0.4)), ((40, -30, 15), (0.02, 0.01, 0.6)), ((5, 8, 100), (-0.3, 0.2, 2.5)),
                       ((88, 0, 20), (0.0, 0.0, 0.5)))
    else:
        mesh = plates_mesh(name == "plates_a")
        poses = _poses(((0, 0, 0), (0.0, 0.0, 0.5)), ((25, -30, 10), (0.02, 0.0, 0.5)), ((180, 0, 0), (0.0, 0.0, 0.5)),
                       ((200, 25, -15), (0.0, 0.02, 0.6)))
    return C.Case(name, mesh, K, rgb, depth, poses, hw, ratios=(1.2, 1.1))


@dataclasses.dataclass
class FrameCase:
    name: str
    mesh: syn.Mesh
    K: np.ndarray
    poses: np.ndarray
    hw: tuple = (120, 160)


FRAME_CASES = ["torus_plate", "fine"]


@functools.lru_cache(maxsize=None)
def frame_case(name):
    K = np.array([[150.0, 0, 81.3], [0, 170.0, 58.7], [0, 0, 1]], np.float32)
    if name == "torus_plate":
        poses = _poses(((55, 20, 10), (0.0, 0.0, 0.35)), ((-130, 35, 70), (0.02, -0.01, 0.5)), ((20, -60, -40), (0.25, 0.1, 0.9)),
                       ((75, -50, 30), (-0.01, 0.01, 0.25)))
        return FrameCase(name, torus_plate_mesh(), K, poses)
    poses = _poses(((0, 0, 0), (0.003, -0.002, 0.3)), ((40, -30, 15), (0.01, 0.005, 0.25)), ((5, 8, 100), (-0.1, 0.05, 1.0)),
                   ((20, 10, -50), (0.0, 0.0, 0.15)))
    return FrameCase(name, fine_mesh(), K, poses)
