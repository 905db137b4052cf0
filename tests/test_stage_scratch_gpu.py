"""The stage operators of one model share one scratch family (fp_model's st_snap / st_cam / st_poses / st_items; DESIGN.md sections 4.8 -
4.13): every one of these calls holds the model's serial lock and leaves the stream synchronised, so a block one call filled is free
for the next.  Here seven calls of different sizes follow each other on ONE model -- so that every shared block both grows and is
reused below its cap, whole and in forced chunks -- and each result must equal, byte for byte, the same call on a fresh model.  What
the results ARE is the business of the operators' own tests; this one only asks that a neighbour leaves nothing behind."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

import icp_cases as IC
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

# A 96 x 80 window (3 x 3 tiles of 32 px, the last row ragged) of icp_cases' 200 x 150 frame around its principal point, seen through
# the same camera with the principal point moved along: the window of the "nan_and_zero" case's depth is that camera's own picture.
W, H = 96, 80
X0, Y0 = (IC.W - W) // 2, 35
K = np.array(IC.K, np.float32)
K[0, 2] -= X0
K[1, 2] -= Y0
DEPTH = np.ascontiguousarray(IC.record_case("nan_and_zero")[2][Y0:Y0 + H, X0:X0 + W], np.float32)
RGB = (np.arange(H * W * 3, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(H, W, 3)
SMALL, LARGE = "ico1", "ico3"          # 80 faces / 42 vertices and 1 280 faces / 642 vertices
G = np.asarray(IC.ICO_G, np.float32)
EST = np.stack([syn.perturb_pose(G, deg=3.0 + 2 * i, trans=0.003 * (i + 1), seed=70 + i) for i in range(3)]).astype(np.float32)
GTS = np.stack([syn.perturb_pose(G, deg=1.0 + i, trans=0.001 * (i + 1), seed=80 + i) for i in range(3)]).astype(np.float32)
TAUS = np.array([0.05, 0.2, 0.5], np.float32)


def _planes(out):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in sorted(out))


def _vsd(m, name, est, gt):
    e, g = syn.to_colmajor(est), syn.to_colmajor(gt)
    out = (_lib.FpPoseVsd * len(e))()
    m._must(m._L.fp_pose_vsd(m._h, name.encode(), _p(e), len(e), _p(g), len(g), 0.015, _p(TAUS), len(TAUS), 1, out))
    return bytes(out)


def _refine(m, name, poses, iterations):
    e = syn.to_colmajor(poses)
    out_p = np.zeros_like(e)
    out = (_lib.FpDepthRefine * len(e))()
    m._must(m._L.fp_refine_depth(m._h, name.encode(), _p(e), len(e), iterations, IC.GATE, 0, _p(out_p), out))
    return out_p.tobytes() + bytes(out)


def _search(m, name, poses):
    e = syn.to_colmajor(poses)
    out = (_lib.FpPoseSearch * len(e))()
    m._must(m._L.fp_pose_search(m._h, name.encode(), _p(e), len(e), 5, 0.004, 0.005, 1, out))
    return bytes(out)


def _scene(m):
    out, recs = m.render_scene([SMALL, LARGE], np.stack([EST[0], IC.moved(G, (0.02, 0.0, 0.03))]))
    return _planes(out) + recs.tobytes()


# (what it is, the forced chunks {hook: poses}, the call -> bytes), in the order the shared model makes them
STEPS = [
    ("render_pose, large mesh", {}, lambda m: _planes(m.render_pose(LARGE, G))),
    ("pose_vsd, small mesh, 3 paired poses in chunks of 1", {"fpt_vsd_set_chunk": 1}, lambda m: _vsd(m, SMALL, EST, GTS)),
    ("refine_depth, small mesh, 3 poses, 2 iterations in chunks of 2", {"fpt_icp_set_chunk": 2}, lambda m: _refine(m, SMALL, EST, 2)),
    ("pose_search, small mesh, 3 poses", {}, lambda m: _search(m, SMALL, EST)),
    ("render_scene, both meshes", {}, _scene),
    ("pose_vsd, small mesh, 3 poses against one truth", {}, lambda m: _vsd(m, SMALL, EST, GTS[:1])),
    ("refine_depth, large mesh", {}, lambda m: _refine(m, LARGE, EST[:2], 2)),
]


@pytest.fixture
def tl():
    """the test build (its chunk hooks) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    for hook in ("fpt_vsd_set_chunk", "fpt_icp_set_chunk"):
        getattr(L, hook).argtypes = [C.c_int]
        getattr(L, hook).restype = None
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_vsd_set_chunk(0)
    L.fpt_icp_set_chunk(0)


def _model():
    m = FoundationPose([IC.ico(1), IC.ico(3)], K)          # geometry-only
    m.upload_frame(RGB, DEPTH)
    return m


def _run(tl, m, step):
    _, chunks, call = step
    try:
        for hook, poses in chunks.items():
            getattr(tl, hook)(poses)
        return call(m)
    finally:
        for hook in chunks:
            getattr(tl, hook)(0)


def test_calls_that_follow_each_other_on_one_model_equal_the_same_calls_on_fresh_models(tl):
    assert (len(IC.ico(1).faces), len(IC.ico(3).faces)) == (80, 1280) and DEPTH.shape == (H, W)
    shared = _model()
    try:
        got = [_run(tl, shared, step) for step in STEPS]
    finally:
        shared.close()
    assert len(set(got)) == len(got) and all(len(b) > 0 for b in got)
    for step, mine in zip(STEPS, got):
        fresh = _model()
        try:
            ref = _run(tl, fresh, step)
        finally:
            fresh.close()
        print(f"{step[0]}: {len(ref)} bytes")
        assert mine == ref, step[0]
