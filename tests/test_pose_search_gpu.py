"""fp_pose_search against tests/search_ref.py: the device records EQUAL the f32 restatement in every integer on the
cases of tests/search_cases.py, which tests/test_search_ref_cpu.py holds to hand answers and to float64 before a kernel sees them.  Then
the promises of the interface: byte-identical records whatever the batch, refusals that leave `out` untouched (argument checks made on
the host: none of them launches anything), the raw depth whatever the depth filter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_cases as IC
import search_cases as SC
import search_ref as SR
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, PoseSearch, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

RGB = np.zeros((SC.H, SC.W, 3), np.uint8)
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundationpose_amd.h")).read()
MAX_BATCH = int(re.search(r"#define FP_MAX_BATCH (\d+)", HEADER).group(1))


def _raw(m, name, poses, n_steps=4, step_m=0.01, tol_m=SC.TOL, vertex_step=1, N=None, out=None):
    """fp_pose_search through the raw ABI -> (return code, records)"""
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out = (_lib.FpPoseSearch * max(N, 1))() if out is None else out
    return m._L.fp_pose_search(m._h, name.encode(), _p(e), N, n_steps, step_m, tol_m, vertex_step, out), out


def _search(m, name, poses, **kw):
    rc, out = _raw(m, name, poses, **kw)
    m._must(rc)
    return list(out)


def _fields(r):
    return {k: getattr(r, k) for k in SR.FIELDS}


def _bytes(recs):
    return b"".join(bytes(r) for r in recs)


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([IC.ico(2), IC.ico(3), SC.cloud(257), SC.cloud(4096), SC.cloud(4097)], SC.K)          # geometry-only
    yield m
    m.close()


@pytest.mark.parametrize("name", SC.RECORD_CASES)
def test_records_equal_the_restatement(model, name):
    mesh, poses, D, n_steps, step_m, vstep = SC.record_case(name)
    ref = SC.expected(name)
    model.upload_frame(RGB, D)
    got = _search(model, mesh, poses, n_steps=n_steps, step_m=float(step_m), vertex_step=vstep)
    for i, (g, r) in enumerate(zip(got, ref)):
        print(f"{name}[{i}]: " + " ".join(f"{k}={v}" for k, v in _fields(g).items()))
        assert _fields(g) == r, (name, i)


def test_a_pose_is_the_same_alone_in_any_batch_and_again(model):
    mesh, poses, D, n_steps, step_m, _ = SC.record_case("batch")
    kw = dict(n_steps=n_steps, step_m=float(step_m))
    model.upload_frame(RGB, D)
    whole = _search(model, mesh, poses, **kw)
    assert _bytes(_search(model, mesh, poses, **kw)) == _bytes(whole)                         # call to call
    for i in range(7):
        alone = _search(model, mesh, poses[i:i + 1], **kw)
        first = _search(model, mesh, np.roll(poses, -i, 0), **kw)                             # pose i at position 0
        last = _search(model, mesh, np.roll(poses, 6 - i, 0), **kw)                           # ... and at position 6
        assert bytes(alone[0]) == bytes(first[0]) == bytes(last[6]) == bytes(whole[i]), i


def test_refusals_leave_out_untouched():
    G = np.asarray(IC.ICO_G, np.float32)
    m = FoundationPose([IC.ico(2), SC.cloud(4097)], SC.K)
    try:
        def refused(match, name, poses, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(poses).reshape(-1, 4, 4)))
            out = (_lib.FpPoseSearch * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            rc, _ = _raw(m, name, poses, out=out, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert bytes(out) == b"\x5a" * C.sizeof(out)

        refused("no frame uploaded", "ico2", [G])
        m.upload_frame(RGB, IC.rendering(IC.ico(2), G))
        assert _raw(m, "ico2", [G])[0] == 0
        refused("unknown target_name", "nobody", [G])
        refused(r"1\.\.FP_MAX_BATCH", "ico2", [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", "ico2", [G] * (MAX_BATCH + 1))
        refused(r"1\.\.FP_SEARCH_MAX_STEPS", "ico2", [G], n_steps=0)
        refused(r"1\.\.FP_SEARCH_MAX_STEPS", "ico2", [G], n_steps=65)
        assert _raw(m, "ico2", [G], n_steps=64)[0] == 0
        for value in (float("nan"), float("inf"), -0.01):
            refused("step_m", "ico2", [G], step_m=value)
        for value in (float("nan"), float("inf"), -0.01, 0.0):
            refused("tol_m", "ico2", [G], tol_m=value)
        refused("vertex_step must be >= 1", "ico2", [G], vertex_step=0)
        refused("vertex_step must be >= 1", "ico2", [G], vertex_step=-3)
        refused(r"FP_SEARCH_MAX_POINTS.*smallest vertex_step that fits is 2", "cloud4097", [G])
        rc, out = _raw(m, "cloud4097", [G], vertex_step=2)
        assert rc == 0 and out[0].n_points == 2049
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(G)
                bad[where] = value
                refused(r"non-finite.*poses\[1\]", "ico2", [G, bad])
        for z in (0.009, 0.0, -0.35):
            bad = np.array(G)
            bad[2, 3] = z
            refused(r"poses\[2\].*FP_RENDER_NEAR_M", "ico2", [G, G, bad])
    finally:
        m.close()


def test_the_depth_filter_does_not_reach_the_call():
    mesh, poses, D, n_steps, step_m, _ = SC.record_case("nan_zero_inf")
    m = FoundationPose(IC.ico(2), SC.K)
    try:
        kw = dict(n_steps=n_steps, step_m=float(step_m))
        m.upload_frame(RGB, D)
        off = _search(m, mesh, poses, **kw)
        m.set_depth_filter(True)
        on = _search(m, mesh, poses, **kw)
        m.upload_frame(RGB, D)
        again = _search(m, mesh, poses, **kw)
        assert _bytes(off) == _bytes(on) == _bytes(again) and _fields(off[0]) == SC.expected("nan_zero_inf")[0]
    finally:
        m.close()


def test_through_the_python_interface(model):
    mesh, poses, D, n_steps, step_m, _ = SC.record_case("batch")
    model.upload_frame(RGB, D)
    recs = model.pose_search(mesh, poses, n_steps=n_steps)                     # step_m: the diameter / 16 by default
    assert all(isinstance(r, PoseSearch) for r in recs)
    assert [{k: getattr(r, k) for k in SR.FIELDS} for r in recs] == SC.expected("batch")
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.pose_search("nobody", poses)
