"""fp_pose_errors against tests/pose_error_ref.py, the float64 reference, within the bounds its docstring derives
(metric_bound: 3.7e-6 m at the scale of these cases).  The cases are those of tests/pose_error_cases.py, which
tests/test_pose_error_ref_cpu.py holds to what each is for.  Geometry-only models except where a Register / Track is part of the test."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pose_error_cases as PC
import pose_error_ref as PR
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

K = PC.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
ADDS = 1
FIELDS = [f for f, _ in _lib.FpPoseError._fields_]


def _const(name):
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def _raw(m, name, est, gt, sym=None, step=1, flags=ADDS, N=None, n_gt=None, S=None, out=None):
    """fp_pose_errors through the raw ABI -> (return code, records)"""
    e = syn.to_colmajor(np.asarray(est, np.float32).reshape(-1, 4, 4))
    g = syn.to_colmajor(np.asarray(gt, np.float32).reshape(-1, 4, 4))
    s = None if sym is None else syn.to_colmajor(np.asarray(sym, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out = (_lib.FpPoseError * max(N, 1))() if out is None else out
    rc = m._L.fp_pose_errors(m._h, name.encode(), _p(e), N, _p(g), len(g) if n_gt is None else n_gt, _p(s),
                             (0 if s is None else len(s)) if S is None else S, step, flags, out)
    return rc, out


def _errors(m, name, est, gt, sym=None, step=1, flags=ADDS):
    rc, out = _raw(m, name, est, gt, sym, step, flags)
    m._must(rc)
    return list(out)


def _bytes(rec):
    return b"".join(bytes(r) for r in rec) if isinstance(rec, (list, tuple)) else bytes(rec)


def _check(what, got, ref, adds=True):
    """one record against the reference, every figure printed before it is asserted"""
    lines = []
    for f in ("add_m", "adds_m", "mssd_m"):
        if f == "adds_m" and not adds:
            continue
        bound = PR.metric_bound(ref, ref[f])
        lines.append(f"{f}: device {getattr(got, f):.9g} reference {ref[f]:.9g} diff {abs(getattr(got, f) - ref[f]):.3g} bound {bound:.3g}")
    print(f"{what}: " + "; ".join(lines))
    for f in ("add_m", "adds_m", "mssd_m"):
        if f == "adds_m" and not adds:
            assert math.isnan(got.adds_m) and got.adds_sum_q20 == -1
            continue
        assert abs(getattr(got, f) - ref[f]) <= PR.metric_bound(ref, ref[f]), (what, f, getattr(got, f), ref[f])
    assert got.n_vertices == ref["n_vertices"] and got.reserved == 0
    assert got.add_m == np.float32(got.add_sum_q20 / 2.0 ** 20 / got.n_vertices)
    if adds:
        assert got.adds_m == np.float32(got.adds_sum_q20 / 2.0 ** 20 / got.n_vertices)
    # the arg-min: equal to the reference's where the runner-up is clearly worse; always a symmetry that attains the minimum
    surf = ref["per_sym_mssd"]
    assert surf[got.best_sym] - ref["mssd_m"] <= 2 * PR.metric_bound(ref, ref["mssd_m"])
    if len(surf) == 1 or np.sort(surf)[1] - ref["mssd_m"] > 1e-3:
        assert got.best_sym == ref["best_sym"], (what, got.best_sym, ref["best_sym"])
        print(f"{what}: rot_deg device {got.rot_deg:.9g} reference {ref['rot_deg']:.9g}; trans_m device {got.trans_m:.9g} reference {ref['trans_m']:.9g}")
        assert abs(got.rot_deg - ref["rot_deg"]) <= PR.angle_bound(ref["rot_deg"]) and abs(got.trans_m - ref["trans_m"]) <= PR.length_bound(ref["trans_m"])
    if ref["best_sym_mspd"] < 0:
        assert got.mspd_px == float("inf") and got.best_sym_mspd == -1
    else:
        bound = PR.pixel_bound(ref, K, ref["mspd_px"])
        print(f"{what}: mspd_px device {got.mspd_px:.9g} reference {ref['mspd_px']:.9g} bound {bound:.3g}")
        assert abs(got.mspd_px - ref["mspd_px"]) <= bound, (what, got.mspd_px, ref["mspd_px"], bound)
        proj = ref["per_sym_mspd"]
        assert proj[got.best_sym_mspd] - ref["mspd_px"] <= 2 * bound
        if len(proj) == 1 or np.sort(proj)[1] - ref["mspd_px"] > 1.0:
            assert got.best_sym_mspd == ref["best_sym_mspd"]


@pytest.fixture(scope="module")
def box_model():
    m = FoundationPose(PC.box(), K)
    yield m
    m.close()


def test_box_lattice_finds_the_symmetry(box_model):
    mesh = PC.box()
    E, Gs = PC.box_poses()
    sym = PC.box_symmetries()
    ref = PR.pose_errors(PC.centred(mesh), mesh.center, K, [E] * 4, Gs, sym)
    got = _errors(box_model, "box", [E] * 4, Gs, sym)
    for k in range(4):
        _check(f"box k = {k}", got[k], ref[k])
        assert got[k].best_sym == k and got[k].best_sym_mspd == k          # (the runner-up is 0.18 m / 134 px away)
    assert max(g.adds_m for g in got) - min(g.adds_m for g in got) < 2e-6 and got[0].mssd_m == pytest.approx(got[3].mssd_m, abs=2e-6)
    assert got[1].add_m > 0.13 and got[0].add_m < 3e-3
    # without the symmetries MSSD is as blind as ADD
    plain = _errors(box_model, "box", [E] * 4, Gs)
    assert all(p.best_sym == 0 for p in plain) and plain[1].mssd_m > 0.17 and plain[0].mssd_m == got[0].mssd_m


def test_anisotropic_cloud_searches_from_the_ground_truth():
    mesh = PC.cloud257()
    E, G = PC.cloud257_poses()
    ref = PR.pose_error(PC.centred(mesh), mesh.center, K, E, G)
    m = FoundationPose(mesh, K)
    try:
        got = _errors(m, "cloud", [E], [G])[0]
        _check("cloud257", got, ref)
        v = PC.centred(mesh).astype(np.float64)
        wrong = PR.nearest_mean(v @ E[:3, :3].T + E[:3, 3], v @ G[:3, :3].T + G[:3, 3])
        assert abs(got.adds_m - wrong) > 1e-3
    finally:
        m.close()


@pytest.mark.parametrize("V,N,S,paired,step", PC.RAGGED)
def test_ragged_shapes(V, N, S, paired, step):
    mesh, est, gt, sym, ref = PC.ragged(V, N, S, paired, step)
    m = FoundationPose(mesh, K)
    try:
        got = _errors(m, mesh.name, est, gt, sym, step)
        assert len(got) == N
        for i in range(N):
            _check(f"V {V} N {N} S {S} n_gt {'N' if paired else 1} step {step} pose {i}", got[i], ref[i])
    finally:
        m.close()


def test_equal_poses_give_exactly_zero(box_model):
    E, Gs = PC.box_poses()
    for sym in (None, PC.box_symmetries()):
        for r in _errors(box_model, "box", [E, Gs[1]], [E, Gs[1]], sym):
            assert (r.add_m, r.adds_m, r.mssd_m, r.mspd_px, r.rot_deg, r.trans_m) == (0, 0, 0, 0, 0, 0)
            assert (r.best_sym, r.best_sym_mspd, r.add_sum_q20, r.adds_sum_q20, r.n_vertices) == (0, 0, 0, 0, 150)


def test_a_record_is_the_same_alone_in_a_batch_and_again():
    mesh, est, gt, sym, ref = PC.ragged(1025, 3, 0, False, 1)
    est65, gt65 = PC.ragged_poses(65, 65, 77)
    m = FoundationPose(mesh, K)
    try:
        batch = _errors(m, mesh.name, est65, gt65, sym)
        again = _errors(m, mesh.name, est65, gt65, sym)
        assert _bytes(batch) == _bytes(again)
        for i in (0, 31, 64):
            alone = _errors(m, mesh.name, est65[i:i + 1], gt65[i:i + 1], sym)
            assert _bytes(alone[0]) == _bytes(batch[i]), i
        # without the flag: the ADD-S fields say so, everything else is unchanged
        plain = _errors(m, mesh.name, est65, gt65, sym, flags=0)
        for p, b in zip(plain, batch):
            assert math.isnan(p.adds_m) and p.adds_sum_q20 == -1
            assert [getattr(p, f) for f in FIELDS if not f.startswith("adds")] == [getattr(b, f) for f in FIELDS if not f.startswith("adds")]
        # every hypothesis against one truth = the same estimates against copies of it
        one = _errors(m, mesh.name, est65, gt65[:1], sym)
        assert _bytes(one) == _bytes(_errors(m, mesh.name, est65, np.repeat(gt65[:1], 65, 0), sym))
    finally:
        m.close()


def test_equal_symmetries_tie_to_the_lower_index(box_model):
    E, Gs = PC.box_poses()
    sym = PC.box_symmetries()
    twice = np.stack([sym[1], sym[2], sym[2], sym[0], sym[2]])      # the z rotation at 2, 3 and 5 of the combined list
    got = _errors(box_model, "box", [E], [Gs[3]], twice)[0]
    assert got.best_sym == 2 and got.best_sym_mspd == 2
    single = _errors(box_model, "box", [E], [Gs[3]], sym)[0]
    assert (got.mssd_m, got.mspd_px, got.rot_deg, got.trans_m) == (single.mssd_m, single.mspd_px, single.rot_deg, single.trans_m)
    same = _errors(box_model, "box", [E], [Gs[0]], np.stack([np.eye(4)] * 3))[0]      # the identity again: 0 wins
    assert same.best_sym == 0 and same.best_sym_mspd == 0


def test_a_vertex_behind_the_near_plane():
    """one vertex pushed to z = 0.004 under the ground truth only: MSPD says so, the other fields are still within the bound"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.05, 0.05, size=(70, 3))
    pts[-1] = (0.0, 0.0, -0.296)
    pts[0] = (0.0, 0.0, 0.296)                          # (keeps the box centre where it is)
    mesh = PC.point_mesh("near", pts)
    E = PC.f32(PC.rigid(PC.rot((0, 0, 1), 0.3), (0.01, 0.0, 0.35)))
    G = PC.f32(PC.rigid(np.eye(3), (0.0, 0.01, 0.30)))
    ref = PR.pose_error(PC.centred(mesh), mesh.center, K, E, G)
    assert ref["best_sym_mspd"] == -1
    m = FoundationPose(mesh, K)
    try:
        got = _errors(m, "near", [E, E], [G, E])
        _check("near plane", got[0], ref)
        assert got[0].mspd_px == float("inf") and got[0].best_sym_mspd == -1
        assert got[1].mspd_px == 0 and got[1].best_sym_mspd == 0          # the other pair of the call is not affected
    finally:
        m.close()


def _smallest_step(N, V, cap):
    return next(s for s in range(1, V + 1) if N * (-(-V // s)) ** 2 <= cap)


def test_refusals_leave_out_untouched():
    cap, max_batch, max_sym = _const("FP_POSE_ERROR_MAX_PAIRS"), _const("FP_MAX_BATCH"), _const("FP_MAX_SYMMETRIES")
    V = max(math.isqrt(cap // max_batch) + 2, cap // 64 // (max_batch * (max_sym + 1)) + 2)
    rng = np.random.default_rng(9)
    big = PC.point_mesh("big", rng.uniform(-0.1, 0.1, size=(V, 3)), diameter=0.35)   # (given: the O(V^2) search is not what this is about)
    E, Gs = PC.box_poses()
    m = FoundationPose([PC.box(), big], K)
    try:
        def refused(match, *a, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(a[1]).reshape(-1, 4, 4)))
            out = (_lib.FpPoseError * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            before = _bytes(out)
            rc, _ = _raw(m, *a, out=out, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert _bytes(out) == before

        refused("unknown target_name", "nobody", [E], [Gs[0]])
        refused(r"1\.\.FP_MAX_BATCH", "box", [E], [Gs[0]], N=0)
        refused(r"1\.\.FP_MAX_BATCH", "box", [E] * (max_batch + 1), [Gs[0]])
        refused("n_gt must be 1 or N", "box", [E] * 3, [Gs[0]] * 2)
        refused("n_gt must be 1 or N", "box", [E] * 3, [Gs[0]], n_gt=0)
        refused(r"0\.\.FP_MAX_SYMMETRIES", "box", [E], [Gs[0]], S=-1)
        refused(r"0\.\.FP_MAX_SYMMETRIES", "box", [E], [Gs[0]], [np.eye(4)] * (max_sym + 1))
        refused("vertex_step", "box", [E], [Gs[0]], step=0)
        refused("vertex_step", "box", [E], [Gs[0]], step=-3)
        refused("unknown flag bits", "box", [E], [Gs[0]], flags=2)
        refused("unknown flag bits", "box", [E], [Gs[0]], flags=-1)
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(E)
                bad[where] = value
                refused(r"non-finite.*est_poses\[1\]", "box", [E, bad], [Gs[0]])
                refused(r"non-finite.*gt_poses\[0\]", "box", [E, E], [bad])
                refused(r"non-finite.*symmetries\[2\]", "box", [E], [Gs[0]], [np.eye(4), np.eye(4), bad])
        far = np.array(E)
        far[1, 3] = -1000.5
        refused(r"1000 m.*est_poses\[0\]", "box", [far], [Gs[0]])
        refused(r"1000 m.*gt_poses\[1\]", "box", [E, E], [E, far])
        refused(r"1000 m.*symmetries\[0\]", "box", [E], [Gs[0]], [far])
        far[1, 3] = 1000.0                              # the limit itself is a translation
        assert _raw(m, "box", [far], [Gs[0]])[0] == 0
        # ADD-S above the cap: the message names the smallest vertex_step that fits, and that step is accepted while the one below is not
        step = _smallest_step(max_batch, V, cap)
        assert max_batch * V * V > cap and step >= 2
        refused(rf"FP_POSE_ERROR_MAX_PAIRS.*smallest vertex_step that fits is {step}\b", "big", [E] * max_batch, [Gs[0]])
        if step > 2:
            refused(rf"smallest vertex_step that fits is {step}\b", "big", [E] * max_batch, [Gs[0]], step=step - 1)
        # ... and the paired part alone: N (S + 1) Vs transformed vertex pairs
        refused("transformed vertex pairs", "big", [E] * max_batch, [Gs[0]], [np.eye(4)] * max_sym, flags=0)
        assert _raw(m, "big", [E], [Gs[0]], step=1, flags=0)[0] == 0
    finally:
        m.close()


def test_serving_path_is_untouched(disc_nets, syn_mesh, syn_scene):
    """a Register followed by a Track after the call equals one before it, bit for bit; a submitted Track refuses the call"""
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        m.set_inplane_steps(1)
        hw = syn_scene.depth.shape

        def serve():
            ok, reg = m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
            assert ok, m.last_error
            ok, trk = m.Track(syn_scene.rgb, syn_scene.depth, reg, syn_mesh.name)
            assert ok, m.last_error
            return reg.tobytes() + trk.tobytes(), trk

        before = [serve() for _ in range(3)]             # eager, capturing, replayed
        assert len({b[0] for b in before}) == 1
        pose = before[0][1]
        errs = m.pose_errors(syn_mesh.name, [pose, syn_scene.gt_pose], syn_scene.gt_pose, vertex_step=3)
        ref = PR.pose_errors(PC.centred(syn_mesh), syn_mesh.center, syn_scene.K, [pose, syn_scene.gt_pose], [syn_scene.gt_pose], None, 3)
        assert abs(errs[0].adds_m - ref[0]["adds_m"]) <= PR.metric_bound(ref[0], ref[0]["adds_m"]) and errs[1].add_m == 0 and errs[0].n_vertices == 854
        assert serve()[0] == before[0][0]
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        out = (_lib.FpPoseError * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(m, syn_mesh.name, [pose], [pose], out=out)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        assert m.pose_errors(syn_mesh.name, [pose], [pose])[0].mssd_m == 0
    finally:
        m.close()


def test_through_the_python_interface(box_model):
    from foundationpose_cpp_amd import PoseError, auc, recall
    mesh = PC.box()
    E, Gs = PC.box_poses()
    ref = PR.pose_errors(PC.centred(mesh), mesh.center, K, [E] * 4, Gs, PC.box_symmetries(), 2)
    errs = box_model.pose_errors("box", [E] * 4, Gs, symmetries=PC.box_symmetries(), vertex_step=2)
    assert len(errs) == 4 and all(isinstance(e, PoseError) for e in errs)
    for k, (e, r) in enumerate(zip(errs, ref)):
        assert e.best_sym == k and e.n_vertices == 75 and abs(e.adds_m - r["adds_m"]) <= PR.metric_bound(r, r["adds_m"])
        assert abs(e.mssd_m - r["mssd_m"]) <= PR.metric_bound(r, r["mssd_m"]) and abs(e.add_m - r["add_m"]) <= PR.metric_bound(r, r["add_m"])
    one = box_model.pose_errors("box", Gs, E, adds=False)                         # one [4,4] ground truth for all; no ADD-S
    assert len(one) == 4 and all(math.isnan(e.adds_m) and e.adds_sum_q20 == -1 for e in one)
    full = box_model.pose_errors("box", [E] * 4, Gs)
    assert recall([e.add_m for e in full], 0.01) == 0.25 and recall([e.adds_m for e in full], 0.01) == 1.0
    assert auc([e.adds_m for e in full]) > 0.96 > 0.3 > auc([e.add_m for e in full])
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        box_model.pose_errors("nobody", [E], [E])
