"""fp_resolve_symmetry: byte for byte the composition of the public calls, and on the noisy scenes of
tests/search_cases.py the equivalent of fp_register_depth's answer that lies nearest the truth -- which the depth alone cannot tell."""
import ctypes as C

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import search_cases as SC
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, PoseColor, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

TEXTURED, PLAIN = "ico3t", "ico3"


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([CC.mesh3(), SC.mesh()], SC.K)          # geometry-only; the same 642 vertices with the 512^2 texture and with the grey default
    yield m
    m.close()


def _resolve(m, name, pose, syms, tol=CC.TOL, S=None, fill=0x5A):
    """the raw ABI -> (return code, out_pose bytes as left, best_sym as left, records)"""
    e = syn.to_colmajor(np.asarray(pose, np.float32).reshape(4, 4))
    s = None if syms is None or len(syms) == 0 else syn.to_colmajor(np.asarray(syms, np.float32).reshape(-1, 4, 4))
    n = (0 if s is None else len(s)) if S is None else S
    out = np.frombuffer(bytes([fill]) * 64, np.float32).copy()
    best = C.c_int(-7)
    recs = (_lib.FpPoseColor * (max(n, 0) + 1))()
    rc = m._L.fp_resolve_symmetry(m._h, name.encode(), _p(e), _p(s), n, tol, _p(out), C.byref(best), recs)
    return rc, out, best.value, recs


def _color(m, name, poses):
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    out = (_lib.FpPoseColor * len(e))()
    m._must(m._L.fp_pose_color(m._h, name.encode(), _p(e), len(e), CC.TOL, out))
    return out


def test_register_by_depth_then_the_colour_reaches_the_truth_itself(model):
    mesh = CC.mesh3()
    syms = CC.mesh_frame_symmetries(mesh)
    unresolved = []
    for seed in SC.GPU_SEEDS:
        sc = CC.scene(seed)
        ok, pose, _ = model.register_depth(sc.rgb, sc.depth, sc.mask, TEXTURED)
        assert ok, model.last_error
        rc, out, best, recs = _resolve(model, TEXTURED, pose, syms)
        assert rc == 0, _lib.last_error()
        # the composition through the public calls, byte for byte
        E = CR.equivalents(pose, syms, mesh.center)
        assert E[0].tobytes() == np.asarray(pose, np.float32).tobytes()
        composed = _color(model, TEXTURED, E)
        win = CR.resolve(list(composed))
        assert bytes(recs) == bytes(composed) and best == win and out.tobytes() == syn.to_colmajor(E[win]).tobytes()
        # against the truth: plain MSSD, no minimum over the symmetries
        errs = [e.mssd_m for e in model.pose_errors(TEXTURED, E, sc.gt_pose, adds=False)]
        z = sorted((float(r.zncc) for r in recs), reverse=True)
        print(f"seed {seed}: plain MSSD of the Register {errs[0] * 1e3:.2f} mm, resolved (symmetry {best}) {errs[best] * 1e3:.3f} mm "
              f"(bound {SC.BOUND_M * 1e3:.3f} mm); zncc winner {z[0]:.3f}, runner-up {z[1]:.3f}")
        assert all(r.status == 0 for r in recs)
        assert best == int(np.argmin(errs))
        assert errs[best] <= SC.BOUND_M
        unresolved.append(errs[0])
    assert max(unresolved) > 0.050          # without the resolution at least one answer is an equivalent 180 degrees away: the test bites


def test_an_untextured_model_has_no_usable_record(model):
    sc = CC.scene(1)
    model.upload_frame(sc.rgb, sc.depth)
    rc, out, best, _ = _resolve(model, PLAIN, sc.gt_pose, np.stack(SC.SYMMETRIES).astype(np.float32))
    assert rc != 0 and "no usable record" in _lib.last_error(), _lib.last_error()
    assert out.tobytes() == b"\x5a" * 64 and best == -7
    flat = _color(model, PLAIN, [sc.gt_pose])[0]
    assert flat.status == CR.FLAT and flat.n_compared > 500


def test_without_symmetries_the_pose_comes_back(model):
    sc = CC.scene(11)
    model.upload_frame(sc.rgb, sc.depth)
    P = syn.perturb_pose(sc.gt_pose, deg=3.0, trans=0.002, seed=12)
    rc, out, best, recs = _resolve(model, TEXTURED, P, None)
    assert rc == 0 and best == 0 and out.tobytes() == syn.to_colmajor(P).tobytes()
    assert bytes(recs) == bytes(_color(model, TEXTURED, [P]))


def test_refusals_leave_the_outputs_untouched(model):
    sc = CC.scene(1)
    syms = CC.mesh_frame_symmetries(CC.mesh3())
    model.upload_frame(sc.rgb, sc.depth)

    def refused(match, name=TEXTURED, pose=sc.gt_pose, s=syms, **kw):
        rc, out, best, _ = _resolve(model, name, pose, s, **kw)
        assert rc != 0 and match in _lib.last_error(), (match, _lib.last_error())
        assert out.tobytes() == b"\x5a" * 64 and best == -7

    refused("unknown target_name", name="nobody")
    refused("0..FP_MAX_SYMMETRIES", S=-1)
    refused("0..FP_MAX_SYMMETRIES", S=1025)
    refused("tol_m", tol=float("nan"))
    bad = syms.copy()
    bad[1, 0, 0] = np.inf
    refused("symmetries[1]", s=bad)
    far = syms.copy()
    far[2, 1, 3] = 2000.0
    refused("symmetries[2]", s=far)
    nan_pose = np.array(sc.gt_pose, np.float32)
    nan_pose[1, 3] = np.nan
    refused("non-finite entry in pose", pose=nan_pose)
    fresh = FoundationPose(CC.mesh3(), SC.K)
    try:
        rc, out, best, _ = _resolve(fresh, TEXTURED, sc.gt_pose, syms)
        assert rc != 0 and "no frame uploaded" in _lib.last_error() and out.tobytes() == b"\x5a" * 64
    finally:
        fresh.close()


def test_through_the_python_interface(model):
    sc = CC.scene(21)
    syms = CC.mesh_frame_symmetries(CC.mesh3())
    model.upload_frame(sc.rgb, sc.depth)
    E = CC.scene_equivalents(21)
    pose, best, recs = model.resolve_symmetry(TEXTURED, E[2], syms)
    rc, out, raw_best, raw = _resolve(model, TEXTURED, E[2], syms)
    assert rc == 0 and best == raw_best == 2 and pose.tobytes() == syn.from_colmajor(out).tobytes()          # symmetry 2 is its own inverse
    assert np.abs(pose - sc.gt_pose).max() < 1e-6
    assert len(recs) == 4 and all(isinstance(r, PoseColor) for r in recs) and [r.zncc for r in recs] == [float(r.zncc) for r in raw]
    alone, best0, one = model.resolve_symmetry(TEXTURED, E[0], None)
    assert best0 == 0 and alone.tobytes() == E[0].tobytes() and len(one) == 1
    with pytest.raises(FoundationPoseError, match="no usable record"):
        model.resolve_symmetry(PLAIN, sc.gt_pose, syms)
