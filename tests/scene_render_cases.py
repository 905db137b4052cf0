"""The scenes tests/test_scene_render_gpu.py renders, built without a GPU so that tests/test_scene_render_ref_cpu.py can hold each to what
it is for (overlap, interpenetration, ties, coverage bits >= 32, triangles across many tiles) before a kernel sees it.  A case is
(meshes, names, poses, K, rgb, depth, (H, W)); the reference of a case is computed once and shared."""
import functools

import numpy as np

import frame_render_ref as FR
import scene_render_ref as SR
from foundationpose_cpp_amd import synthetic as syn


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _named(mesh, name):
    return syn.Mesh(name, mesh.vertices, mesh.normals, mesh.texcoords, mesh.faces, mesh.texture).finalize()


def box_mesh():
    """the 12-triangle box of tests/test_frame_render_gpu.py"""
    h = np.array([0.10, 0.075, 0.05])
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int32)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    return syn.Mesh("box", v.astype(np.float32), n.astype(np.float32), np.zeros((8, 2), np.float32), faces, np.full((2, 2, 3), 100, np.uint8)).finalize()


@functools.lru_cache(maxsize=None)
def meshes():
    return dict(a=_named(syn.make_mesh(1, textured=False), "a"), b=_named(syn.make_mesh(2, textured=False), "b"), box=box_mesh())


def objects_of(case):
    ms, names, poses = case[0], case[1], case[2]
    return [(FR.centred(ms[n]), ms[n].faces, p) for n, p in zip(names, poses)]


@functools.lru_cache(maxsize=None)
def single():
    """K = 1: syn.make_mesh(1) on a 160 x 120 frame"""
    W, H = 160, 120
    K = syn.intrinsics(W, H)
    depth = np.full((H, W), 1.0, np.float32)
    depth[:, :W // 2] = 0.20                         # an observed plane in front of the left half of the object
    depth[::7, ::5] = 0.0                            # missing depth counts as visible
    pose = syn.pose_matrix(syn.random_rotation(7), (0.01, 0.0, 0.25))
    return meshes(), ("a",), (pose,), K, _frame(H, W, 5), depth, (H, W)


# rotation seeds of the four objects of overlap(): the first set tried for which the reference shows every property the case is for
# (tests/test_scene_render_ref_cpu.py asserts them)
OVERLAP_SEEDS = (3, 11, 5, 8)


@functools.lru_cache(maxsize=None)
def overlap():
    """K = 4 on 208 x 150: meshes a, b, a, b; objects 0 and 1 interpenetrate (translations 2 cm apart: less than any radius), object 2
    lies behind them, object 3 behind an observed depth plane"""
    W, H = 208, 150
    K = syn.intrinsics(W, H)
    t = ((0.0, 0.0, 0.30), (0.016, 0.010, 0.305), (-0.03, 0.02, 0.42), (0.10, -0.04, 0.36))
    poses = tuple(syn.pose_matrix(syn.random_rotation(s), ti) for s, ti in zip(OVERLAP_SEEDS, t))
    depth = np.full((H, W), 2.0, np.float32)
    depth[:, 130:] = 0.25                            # the plane: in front of object 3 and of the right rim of the pair
    depth[::9, ::4] = 0.0
    return meshes(), ("a", "b", "a", "b"), poses, K, _frame(H, W, 6), depth, (H, W)


@functools.lru_cache(maxsize=None)
def tie():
    """the same target twice at the identical pose"""
    ms, _, (pose,), K, rgb, depth, hw = single()
    return ms, ("a", "a"), (pose, pose), K, rgb, depth, hw


@functools.lru_cache(maxsize=None)
def grid64():
    """K = 64: an 8 x 8 grid of make_mesh(1) in 320 x 240, neighbours overlapping"""
    W, H = 320, 240
    K = syn.intrinsics(W, H)
    poses = []
    for i in range(64):
        r, c = divmod(i, 8)
        z = 0.55 + 0.01 * ((i * 5) % 7)
        poses.append(syn.pose_matrix(syn.random_rotation(100 + i), ((c - 3.5) * 0.1 * z / 0.55, (r - 3.5) * 0.075 * z / 0.55, z)))
    depth = np.full((H, W), 2.0, np.float32)
    depth[100:140] = 0.5
    return meshes(), ("a",) * 64, tuple(poses), K, _frame(H, W, 7), depth, (H, W)


@functools.lru_cache(maxsize=None)
def binning(larger=False):
    """640 x 480: the box at 0.3 m (each triangle spans tens of tiles), a subdivision-2 mesh in front of a corner of it, one object partly
    outside the frame, one wholly outside.  larger: more objects and nearer ones, so the tile lists grow"""
    W, H = 640, 480
    K = syn.intrinsics(W, H)
    names = ["box", "b", "b", "a"]
    poses = [syn.pose_matrix(syn.random_rotation(3), (0.02, -0.01, 0.30)), syn.pose_matrix(syn.random_rotation(4), (0.05, 0.03, 0.22)),
             syn.pose_matrix(syn.random_rotation(5), (-0.28, 0.10, 0.30)),      # partly outside (left edge)
             syn.pose_matrix(syn.random_rotation(6), (0.0, -0.9, 0.40))]        # wholly outside (above)
    if larger:
        names += ["b", "box", "b", "a"]
        poses += [syn.pose_matrix(syn.random_rotation(7), (-0.05, -0.05, 0.15)), syn.pose_matrix(syn.random_rotation(8), (0.0, 0.02, 0.25)),
                  syn.pose_matrix(syn.random_rotation(9), (0.08, -0.06, 0.18)), syn.pose_matrix(syn.random_rotation(10), (-0.1, 0.08, 0.2))]
    depth = np.full((H, W), 2.0, np.float32)
    depth[200:260] = 0.2
    return meshes(), tuple(names), tuple(poses), K, _frame(H, W, 8), depth, (H, W)


@functools.lru_cache(maxsize=None)
def wide():
    """2112 x 1056: 66 x 33 = 2178 tiles, more than the 2048 the binning kernels hold in LDS at a time.  One object in the first tiles, a
    box and a mesh across tile 2048 (tile row 31) down to the frame's lower edge"""
    W, H = 2112, 1056
    K = syn.intrinsics(W, H)
    poses = (syn.pose_matrix(syn.random_rotation(12), (-0.42, -0.2, 0.5)), syn.pose_matrix(syn.random_rotation(13), (0.1, 0.17, 0.4)),
             syn.pose_matrix(syn.random_rotation(14), (0.03, 0.2, 0.33)))
    depth = np.full((H, W), 2.0, np.float32)
    depth[1000:1020] = 0.2
    return meshes(), ("a", "box", "b"), poses, K, _frame(H, W, 9), depth, (H, W)


@functools.lru_cache(maxsize=None)
def reference(name, *args):
    """(outputs, records) of scene_render_ref.render for the case `name`; computed once, callers must not modify it"""
    case = globals()[name](*args)
    return SR.render(objects_of(case), case[3], case[4], case[5])
