"""fp_register_depth on a geometry-only model: byte for byte the composition of the public calls it is made of
(upload_frame -> get_hyp_poses -> pose_search -> refine_depth, with the candidate and winner rules of tests/search_ref.py in Python), within
twice the float64 reference's worst MSSD of the ground truth (tests/test_search_ref_cpu.py recorded it), the same bytes from call to call,
the sampler's errors, a frame without the object, and a serving path that does not notice the call."""
import ctypes as C
import functools
from unittest import mock

import numpy as np
import pytest

import icp_ref as IR
import search_cases as SC
import search_ref as SR
from foundationpose_cpp_amd import DepthRegister, FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

NAME = "ico3"
REFUSED = IR.REFUSED_NEAR | IR.REFUSED_RANGE | IR.TOO_FEW


def _register(m, name, rgb, depth, mask, top_k=0, tol_m=0.0, iterations=0, rec=None, out=None):
    """fp_register_depth through the raw ABI -> (return code, pose [4,4], record)"""
    rgb, depth, mask = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(mask, np.uint8)
    out = np.zeros(16, np.float32) if out is None else out
    rec = _lib.FpDepthRegister() if rec is None else rec
    rc = m._L.fp_register_depth(m._h, _p(rgb), _p(depth), _p(mask), 0, depth.shape[0], depth.shape[1], name.encode(), top_k, tol_m, iterations,
                                _p(out), C.byref(rec))
    return rc, syn.from_colmajor(out), rec


def _composed(m, mesh, name, rgb, depth, mask, top_k=SC.TOP_K, tol_m=SC.TOL, iterations=SC.ITERATIONS):
    """the five steps through the public calls -> (pose [4,4], record, hypothesis poses), or (None, None, poses) when no candidate is left"""
    m.upload_frame(rgb, depth)
    hyp = m.get_hyp_poses(mask)
    assert hyp is not None, m.last_error
    step = SC.step_of(mesh)
    found = (_lib.FpPoseSearch * len(hyp))()
    m._must(m._L.fp_pose_search(m._h, name.encode(), _p(syn.to_colmajor(hyp)), len(hyp), 9, float(step), tol_m, SR.smallest_step(len(mesh.vertices)), found))
    cands = SR.pick_candidates([dict(score=r.score, status=r.status) for r in found], top_k)
    starts = syn.to_colmajor(np.stack([SR.at_step(hyp[i], found[i].best_step, step) for i in cands]))
    refined = np.zeros_like(starts)
    recs = (_lib.FpDepthRefine * len(cands))()
    gate = float(min(np.float32(4) * np.float32(tol_m), np.float32(mesh.diameter)))
    m._must(m._L.fp_refine_depth(m._h, name.encode(), _p(starts), len(cands), iterations, gate, 0, _p(refined), recs))
    w = SR.pick_winner(cands, [dict(status=r.status, n_used=r.n_used, n_behind=r.n_behind, e2=r.sums_q32[27]) for r in recs])
    if w is None:
        return None, None, hyp
    rec = _lib.FpDepthRegister(hypothesis=cands[w], n_hypotheses=len(hyp), n_candidates=len(cands), rank_key=recs[w].n_used - recs[w].n_behind)
    C.memmove(C.byref(rec.search), C.byref(found[cands[w]]), C.sizeof(_lib.FpPoseSearch))
    C.memmove(C.byref(rec.refine), C.byref(recs[w]), C.sizeof(_lib.FpDepthRefine))
    return syn.from_colmajor(refined[w]), rec, hyp


@pytest.fixture
def tl():
    """the test build (its launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L


def _logged(tl, fn):
    tl.fpt_launch_log_clear()
    tl.fpt_launch_log_arm(2)                      # 2: the launches outside the networks too
    try:
        out = fn()
    finally:
        tl.fpt_launch_log_arm(0)
    n = tl.fpt_launch_log_count()
    f = (C.c_int * (7 * max(n, 1)))()
    names = C.create_string_buffer(96 * max(n, 1))
    assert tl.fpt_launch_log_get_all(f, names, 96, n) == n
    tl.fpt_launch_log_clear()
    return out, (list(f), names.raw)


@pytest.fixture(scope="module")
def model():
    m = FoundationPose(SC.mesh(), SC.K)          # geometry-only: NULL weights
    yield m
    m.close()


@pytest.mark.parametrize("seed", SC.GPU_SEEDS)
def test_equals_the_composition_and_reaches_the_truth(model, seed):
    mesh, sc = SC.mesh(), SC.scene(seed)
    rc, pose, rec = _register(model, NAME, sc.rgb, sc.depth, sc.mask)
    assert rc == 0, _lib.last_error()
    rc2, pose2, rec2 = _register(model, NAME, sc.rgb, sc.depth, sc.mask, SC.TOP_K, SC.TOL, SC.ITERATIONS)          # again, the defaults spelled out
    assert rc2 == 0 and pose2.tobytes() == pose.tobytes() and bytes(rec2) == bytes(rec)
    want_pose, want_rec, hyp = _composed(model, mesh, NAME, sc.rgb, sc.depth, sc.mask)
    assert pose.tobytes() == want_pose.tobytes() and bytes(rec) == bytes(want_rec)
    assert (rec.n_hypotheses, rec.n_candidates) == (252, SC.TOP_K) and rec.rank_key == rec.refine.n_used - rec.refine.n_behind > 0
    assert not rec.refine.status & REFUSED and rec.search.status == 0
    err = model.pose_errors(NAME, [pose], sc.gt_pose, symmetries=np.stack(SC.SYMMETRIES), adds=False)[0]
    print(f"seed {seed}: hypothesis {rec.hypothesis} (step {rec.search.best_step}, score {rec.search.score}), rank_key {rec.rank_key}, "
          f"MSSD {err.mssd_m * 1e3:.3f} mm (float64 reference {SC.REF_MSSD_MM[seed]:.3f} mm, bound {SC.BOUND_M * 1e3:.3f} mm)")
    assert err.mssd_m <= SC.BOUND_M
    # the f32 reference ICP from the winner's start ends within the bound too
    start = SR.at_step(hyp[rec.hypothesis], rec.search.best_step, SC.step_of(mesh))
    ref = IR.icp32(mesh, start, SC.K, sc.depth, float(min(np.float32(4) * np.float32(SC.TOL), np.float32(mesh.diameter))), SC.ITERATIONS)
    gap = SC.mssd_sym(mesh, ref["pose"], sc.gt_pose)
    print(f"  icp32 from the same start: MSSD {gap * 1e3:.3f} mm")
    assert gap <= SC.BOUND_M
    # the frame stays uploaded: a stage operator can follow
    _, (again,) = model.refine_depth(NAME, [pose], iterations=0, max_dist_m=0.02)
    assert again.n_used == rec.refine.n_used


def test_through_the_python_interface(model):
    sc = SC.scene(1)
    rc, pose, rec = _register(model, NAME, sc.rgb, sc.depth, sc.mask)
    ok, P, r = model.register_depth(sc.rgb, sc.depth, sc.mask, NAME)
    assert ok and rc == 0 and P.tobytes() == pose.tobytes() and isinstance(r, DepthRegister)
    assert (r.hypothesis, r.n_hypotheses, r.n_candidates, r.rank_key) == (rec.hypothesis, 252, SC.TOP_K, rec.rank_key)
    assert r.search.score == rec.search.score and r.refine.n_used == rec.refine.n_used and r.refine.sums_q32 == tuple(rec.refine.sums_q32)
    ok, P, r = model.register_depth(sc.rgb, sc.depth, np.zeros_like(sc.mask), NAME)
    assert not ok and P is None and "Mask is all zero" in model.last_error


def test_errors_leave_the_pose_untouched(model):
    sc = SC.scene(1)

    def refused(match, name=NAME, mask=sc.mask, **kw):
        out = np.full(16, 7.5, np.float32)
        rec = _lib.FpDepthRegister()
        C.memset(C.byref(rec), 0x5A, C.sizeof(rec))
        rc, _, _ = _register(model, name, sc.rgb, sc.depth, mask, out=out, rec=rec, **kw)
        assert rc != 0 and match in _lib.last_error(), (match, _lib.last_error())
        assert (out == 7.5).all() and bytes(rec) == b"\x5a" * C.sizeof(rec)

    refused("Mask is all zero", mask=np.zeros_like(sc.mask))                  # the sampler's message
    refused("Invalid `target_name`", name="nobody")
    refused("top_k", top_k=65)
    refused("top_k", top_k=-1)
    refused("tol_m", tol_m=-0.001)
    refused("tol_m", tol_m=float("nan"))
    refused("iterations", iterations=33)
    refused("iterations", iterations=-1)


@functools.lru_cache(maxsize=None)
def _wall():
    return np.full((SC.H, SC.W), np.float32(1.5))


def test_a_frame_without_the_object(model):
    """the wall alone under the scene's mask, top_k 4 and 5 iterations.  The rules give neither of the outcomes the design expected (a
    failure, or rank_key <= 0): where the ellipsoid's flank touches the wall a few dozen pixels are used and none is behind, so the call
    returns a pose with a small positive rank_key -- the f32 reference says the same (62 here, 63 with top_k 16 and 15 iterations, against
    473 to 1056 on the eight real scenes).  The test asserts what the reference gives: the same kind of outcome, and a rank_key below half the
    least one of a real scene."""
    mesh, sc = SC.mesh(), SC.scene(1)
    D = _wall()
    rc, pose, rec = _register(model, NAME, sc.rgb, D, sc.mask, 4, SC.TOL, 5)
    want_pose, want_rec, hyp = _composed(model, mesh, NAME, sc.rgb, D, sc.mask, 4, SC.TOL, 5)
    ref = SR.register_ref(mesh, hyp, SC.K, D, IR.icp32, 4, SC.TOL, 5)
    print("device:", "failed: " + _lib.last_error() if rc else f"rank_key {rec.rank_key}, n_used {rec.refine.n_used}", "| reference:",
          "no candidate" if ref is None else f"rank_key {ref['rank_key']}")
    assert (rc == 0) == (ref is not None) == (want_pose is not None)
    if rc:
        assert "no candidate" in _lib.last_error()
    else:
        assert pose.tobytes() == want_pose.tobytes() and bytes(rec) == bytes(want_rec)
        assert 0 < ref["rank_key"] < 473 // 2 and 0 < rec.rank_key < 473 // 2


def test_serving_path_is_untouched(tl, disc_nets, syn_mesh, syn_scene):
    """a Register followed by a Track after the calls equals one before them, bit for bit and launch for launch; a Track from a host frame
    leaves only its crop window, and a submitted Track is pending: both refuse fp_pose_search, the second fp_register_depth too"""
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        m.set_inplane_steps(1)
        hw = syn_scene.depth.shape
        name = syn_mesh.name

        def serve():
            ok, reg = m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, name)
            assert ok, m.last_error
            ok, trk = m.Track(syn_scene.rgb, syn_scene.depth, reg, name)
            assert ok, m.last_error
            return reg.tobytes() + trk.tobytes()

        before = [serve() for _ in range(3)]             # eager, capturing, replayed
        assert len(set(before)) == 1
        m.upload_frame(syn_scene.rgb, syn_scene.depth)   # (as before the calls below: both logged rounds follow an upload)
        _, log_before = _logged(tl, serve)
        found = (_lib.FpPoseSearch * 1)()
        C.memset(found, 0x5A, C.sizeof(found))
        g = syn.to_colmajor(syn_scene.gt_pose[None])
        rc = m._L.fp_pose_search(m._h, name.encode(), _p(g), 1, 9, 0.01, 0.005, 3, found)
        assert rc != 0 and "only its crop window" in _lib.last_error() and bytes(found) == b"\x5a" * C.sizeof(found)
        ok, pose, rec = m.register_depth(syn_scene.rgb, syn_scene.depth, syn_scene.mask, name)
        assert ok, m.last_error
        err = m.pose_errors(name, [pose], syn_scene.gt_pose, symmetries=np.stack(SC.SYMMETRIES), adds=False)[0]
        print(f"640 x 480, 42 hypotheses: hypothesis {rec.hypothesis}, rank_key {rec.rank_key}, MSSD {err.mssd_m * 1e3:.3f} mm")
        assert rec.n_hypotheses == 42 and rec.search.n_points == 854 and rec.rank_key > 0
        recs = m.pose_search(name, [pose, syn_scene.gt_pose], vertex_step=3)           # the frame stayed uploaded
        assert recs[1].n_inlier > recs[1].n_facing // 2
        after, log_after = _logged(tl, serve)
        assert after == before[0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), name.encode(), 1))
        rc = m._L.fp_pose_search(m._h, name.encode(), _p(g), 1, 9, 0.01, 0.005, 3, found)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and bytes(found) == b"\x5a" * C.sizeof(found)
        ok, _, _ = m.register_depth(syn_scene.rgb, syn_scene.depth, syn_scene.mask, name)
        assert not ok and "has not been waited for" in m.last_error
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        # the profiler's family
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        m.profile_reset(); m.profile(True)
        m.pose_search(name, [syn_scene.gt_pose], vertex_step=3)
        rep = m.profile_report()
        m.profile(False)
        assert rep["pose_search"]["calls"] == 1
    finally:
        m.close()
