"""fp_render_pose's host-side screen bound (frame_tile_bound) is conservative: every pixel the reference covers
lies in a tile inside the bound, for objects inside, across and outside the frame, near and far, and for poses that are not rotations.
A pure host function of the test build: no GPU."""
import ctypes as C

import numpy as np
import pytest

import frame_render_ref as FR
import geometry_cases as GC
from foundationpose_cpp_amd import _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

TILE = 32


@pytest.fixture(scope="module")
def bound():
    L = _lib.test_lib()
    L.fpt_frame_tile_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]

    def call(pose, K, radius, H, W):
        out = np.zeros(4, np.int32)
        assert L.fpt_frame_tile_bound(_p(syn.to_colmajor(np.asarray(pose, np.float32))), _p(np.ascontiguousarray(K, np.float32)), radius, H, W, _p(out)) == 0
        return [int(v) for v in out]
    return call


def _covered_tiles(v, faces, pose, K, H, W):
    cam, snap, near, far = FR.project(v, pose, K)
    assert not near.any() and not far.any()
    model = FR.rasterize(cam, snap, faces, H, W) != FR.EMPTY
    return {(x // TILE, y // TILE) for y, x in zip(*np.nonzero(model))}


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5, 17, 32])
def test_bound_contains_every_covered_tile(bound, seed):
    mesh, K, _, _, poses, (H, W) = GC.random_case(seed)
    v = FR.centred(mesh)
    radius = float(np.sqrt((v.astype(np.float64) ** 2).sum(1).max()))
    ntx, nty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rng = np.random.default_rng(seed)
    checked = spared = 0
    for pose in list(poses) + [syn.pose_matrix(syn.random_rotation(seed) * rng.uniform(0.5, 1.5), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.4, 2.0)))
                               for _ in range(4)]:       # ... and four scaled "rotations": the bound follows the norm of the linear part
        if FR.refused(v, pose, K):
            continue
        tx0, ty0, tx1, ty1 = bound(pose, K, radius, H, W)
        assert 0 <= tx0 and 0 <= ty0 and tx1 < ntx and ty1 < nty
        tiles = _covered_tiles(v, mesh.faces, pose, K, H, W)
        assert all(tx0 <= x <= tx1 and ty0 <= y <= ty1 for x, y in tiles), (seed, pose)
        checked += 1
        spared += (max(tx1 - tx0 + 1, 0) * max(ty1 - ty0 + 1, 0)) < ntx * nty
    assert checked >= 6 and spared >= 1              # and it does spare work somewhere


def test_bound_edge_cases(bound):
    K = syn.intrinsics()
    whole = [0, 0, 19, 14]
    eye = np.eye(3)
    assert bound(syn.pose_matrix(eye, (0, 0, 0.7)), K, 0.1, 480, 640) == [8, 5, 11, 9]       # columns 320 -+ 0.1 / 0.6 * 320 = 266.7 .. 373.3, rows 186.7 .. 293.3, each grown by 2 px
    assert bound(syn.pose_matrix(eye, (0, 0, 0.105)), K, 0.1, 480, 640) == whole              # the sphere reaches the near constant
    assert bound(syn.pose_matrix(eye, (0, 0, -1.0)), K, 0.1, 480, 640) == whole
    assert bound(syn.pose_matrix(eye, (np.nan, 0, 1.0)), K, 0.1, 480, 640) == whole
    assert bound(syn.pose_matrix(eye, (0, 0, 1.0)), K, float("inf"), 480, 640) == whole
    tx0, ty0, tx1, ty1 = bound(syn.pose_matrix(eye, (5.0, 0, 1.0)), K, 0.1, 480, 640)         # far off to the right: an empty range
    assert tx0 > tx1
    tx0, ty0, tx1, ty1 = bound(syn.pose_matrix(eye, (0, -5.0, 1.0)), K, 0.1, 480, 640)        # far above
    assert ty0 > ty1
    tx0, ty0, tx1, ty1 = bound(syn.pose_matrix(eye, (1e30, 0, 1.0)), K, 0.1, 480, 640)        # no overflow on the way to int
    assert tx0 > tx1
