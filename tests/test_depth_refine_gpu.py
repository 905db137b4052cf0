"""fp_refine_depth against tests/icp_ref.py: the records of one evaluation EQUAL the f32 restatement (a) in every
count and every one of the 28 integer sums; the refined poses end where the float64 ICP (b) ends, within the bound measured on the CPU
between (a) and (b), and within (b)'s bound of the ground truth.  Then the promises of the interface: the fixed point, byte-identical
records whatever the batch, the stopping rules, refusals that leave the outputs untouched, the untouched serving path.  The cases are
those of tests/icp_cases.py, which tests/test_icp_ref_cpu.py holds to a hand answer and to (b) before a kernel sees them."""
import ctypes as C
import os
import re
from unittest import mock

import numpy as np
import pytest

import frame_render_ref as FR
import icp_cases as IC
import icp_ref as IR
from foundationpose_cpp_amd import DepthRefine, FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
RGB = np.zeros((IC.H, IC.W, 3), np.uint8)
TRANSLATION_ONLY = 1


def _const(name):
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def _raw(m, name, poses, iterations=0, gate=IC.GATE, flags=0, N=None, out_p=None, out=None):
    """fp_refine_depth through the raw ABI -> (return code, poses [N,4,4], records)"""
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out_p = np.zeros((max(N, 1), 16), np.float32) if out_p is None else out_p
    out = (_lib.FpDepthRefine * max(N, 1))() if out is None else out
    rc = m._L.fp_refine_depth(m._h, name.encode(), _p(e), N, iterations, gate, flags, _p(out_p), out)
    return rc, syn.from_colmajor(out_p), out


def _refine(m, name, poses, **kw):
    rc, P, out = _raw(m, name, poses, **kw)
    m._must(rc)
    return P, list(out)


def _bytes(rec):
    return b"".join(bytes(r) for r in rec) if isinstance(rec, (list, tuple)) else bytes(rec)


def _show(what, r):
    print(f"{what}: " + " ".join(f"{k}={getattr(r, k)}" for k in IR.COUNTS + ("iterations", "rank", "status")) +
          f" rms_m={r.rms_m:.3e} cond={r.cond:.3e} last={r.last_rot_rad:.2e} rad {r.last_trans_m:.2e} m")


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([IC.ico(2), IC.ico(3), IC.ico(4), IC.plate()], IC.K)          # geometry-only
    yield m
    m.close()


@pytest.mark.parametrize("name", IC.RECORD_CASES)
def test_one_evaluation_equals_the_restatement(model, name):
    """iterations = 0: six counts and 28 integers equal (a), rms_m is the host formula, the pose comes back bit for bit"""
    mesh, P, D = IC.record_case(name)
    ref = IC.expected(name)
    model.upload_frame(RGB, D)
    out_p, (r,) = _refine(model, mesh, [P])
    _show(name, r)
    for k in IR.COUNTS:
        assert getattr(r, k) == ref[k], (name, k, getattr(r, k), ref[k])
    assert list(r.sums_q32) == ref["sums"], name
    assert r.n_valid == r.n_used + r.n_front + r.n_behind + r.n_grazing
    assert (r.iterations, r.rank, r.status, r.reserved, r.cond, r.last_rot_rad, r.last_trans_m) == (0, 0, 0, 0, 0.0, 0.0, 0.0)
    assert np.float32(r.rms_m) == IR.rms_m(ref["sums"], ref["n_used"], IC.mesh_of(mesh).diameter)
    assert out_p[0].tobytes() == np.asarray(P, np.float32).tobytes()
    if name == "outside":
        assert ref["n_model"] == 0 and not any(ref["sums"])
    if name == "plate_in_front":
        assert ref["n_front"] > 100 and ref["n_used"] > 100            # the pixels under the plate are front, never used: (a) says which
    if name == "nan_and_zero":
        assert ref["n_model"] - ref["n_valid"] >= 60
    if name == "edge":
        assert 0 < ref["n_model"] < IC.expected("inside")["n_model"]


def test_fixed_point(model):
    """the depth is fp_render_pose's own model_depth of G over a wall at 1.5 m: G comes back bit for bit, sum J e and sum e^2 are exactly 0,
    CONVERGED after one evaluation (a zero update leaves the f32 pose as it is, so no second pass is needed)"""
    G = np.asarray(IC.ICO_G, np.float32)
    model.upload_frame(RGB, np.zeros((IC.H, IC.W), np.float32))
    z = model.render_pose("ico3", G, want=("model_depth",))["model_depth"]
    assert (z != 0).sum() > 500
    model.upload_frame(RGB, np.where(z != 0, z, IC.WALL).astype(np.float32))
    out_p, (r,) = _refine(model, "ico3", [G], iterations=5)
    _show("fixed point", r)
    assert out_p[0].tobytes() == G.tobytes()
    assert list(r.sums_q32[21:]) == [0] * 7 and r.rms_m == 0.0
    assert r.status == IR.CONVERGED and r.iterations == 1 and r.rank == 6 and r.n_used > 400
    assert r.last_rot_rad == 0.0 and r.last_trans_m == 0.0


@pytest.mark.parametrize("seed", IC.SCENE_SEEDS)
def test_converges_where_float64_converges(model, seed):
    """the four noisy scenes, both starts, gate 0.02 m, 10 iterations: the device's final pose against (b)'s and against the ground truth"""
    sc = IC.scene(seed)
    model.upload_frame(RGB, sc.depth)
    starts = [IC.start(seed, 0), IC.start(seed, 1)]
    out_p, recs = _refine(model, "ico4", starts, iterations=10)
    for k in (0, 1):
        _show(f"seed {seed} start {k}", recs[k])
        deg, dist = IR.pose_gap(out_p[k], IC.refined64(seed, k)["pose"])
        gdeg, gdist = IR.pose_gap(out_p[k], sc.gt_pose)
        print(f"  against (b): {deg:.4f} deg {dist * 1e3:.4f} mm; against the truth: {gdeg:.3f} deg {gdist * 1e3:.3f} mm")
        assert deg <= IC.AB_BOUND_DEG and dist <= IC.AB_BOUND_M
        assert gdeg <= IC.GT_BOUND_DEG and gdist <= IC.GT_BOUND_M
        assert recs[k].rank == 6 and 1e-4 < recs[k].cond < 1e-1 and recs[k].n_used > 300
        # the record describes the returned pose
        ref = IR.sums(FR.centred(IC.ico(4)), IC.ico(4).faces, out_p[k], IC.K, sc.depth, IC.GATE, IC.ico(4).diameter)
        assert [getattr(recs[k], c) for c in IR.COUNTS] == [ref[c] for c in IR.COUNTS] and list(recs[k].sums_q32) == ref["sums"]


@pytest.fixture
def tl():
    """the test build (its chunk hook and launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    L.fpt_icp_set_chunk.argtypes = [C.c_int]
    L.fpt_icp_set_chunk.restype = None
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_icp_set_chunk(0)


def _noisy_depth():
    rng = np.random.default_rng(7)
    D = IC.rendering(IC.ico(2), IC.ICO_G) + rng.normal(0, 0.0005, (IC.H, IC.W)).astype(np.float32)
    return np.ascontiguousarray(D, np.float32)


def test_a_pose_is_the_same_alone_in_any_batch_and_again(model, tl):
    est = IC.batch_poses(7)
    D = _noisy_depth()
    model.upload_frame(RGB, D)
    P, recs = _refine(model, "ico2", est, iterations=6)
    for i, r in enumerate(recs):
        _show(f"batch pose {i}", r)
    assert recs[5].n_model == 0 and recs[5].status == IR.TOO_FEW and sum(r.iterations >= 2 for r in recs) >= 5
    assert len({r.iterations for r in recs}) > 1 or len({r.status for r in recs}) > 1          # (the poses do stop at different passes)
    P2, recs2 = _refine(model, "ico2", est, iterations=6)                                      # call to call
    assert P.tobytes() == P2.tobytes() and _bytes(recs) == _bytes(recs2)
    for i in range(7):
        Pi, ri = _refine(model, "ico2", est[i:i + 1], iterations=6)
        assert Pi[0].tobytes() == P[i].tobytes() and _bytes(ri[0]) == _bytes(recs[i]), i
    m = FoundationPose(IC.ico(2), IC.K)                                                        # chunks of 2 poses, through the test build
    try:
        m.upload_frame(RGB, D)
        tl.fpt_icp_set_chunk(2)
        Pc, rc = _refine(m, "ico2", est, iterations=6)
        tl.fpt_icp_set_chunk(0)
        assert Pc.tobytes() == P.tobytes() and _bytes(rc) == _bytes(recs)
    finally:
        m.close()


def test_plate_rank(model):
    """the hand answer of tests/test_icp_ref_cpu.py on the device: rank 3 (z, rotations about x and y), rank 1 with the translation-only
    flag; 3 mm along z, the other components untouched"""
    G = np.asarray(IC.PLATE_G, np.float32)
    model.upload_frame(RGB, IC.PLATE_D)
    P, (r,) = _refine(model, "plate", [G], iterations=1)
    _show("plate", r)
    assert r.rank == 3 and r.iterations == 1 and r.n_used == r.n_model > 500
    assert abs(float(P[0, 2, 3]) - (IC.PLATE_Z0 + 0.003)) < 1e-6
    assert P[0, :2, 3].tobytes() == G[:2, 3].tobytes()                               # x, y
    assert abs(float(P[0, 1, 0]) - float(P[0, 0, 1])) < 1e-12 and r.last_rot_rad < 1e-4   # no rotation about z; none to speak of about x, y
    assert abs(r.last_trans_m - 0.003) < 1e-6
    assert r.rms_m < 1e-6                                                            # the record is that of the moved plate
    P1, (r1,) = _refine(model, "plate", [G], iterations=1, flags=TRANSLATION_ONLY)
    _show("plate, translation only", r1)
    assert r1.rank == 1 and r1.last_rot_rad == 0.0
    assert P1[0, :3, :3].tobytes() == G[:3, :3].tobytes() and P1[0, :2, 3].tobytes() == G[:2, 3].tobytes() and P1[0, 3].tobytes() == G[3].tobytes()
    assert abs(float(P1[0, 2, 3]) - (IC.PLATE_Z0 + 0.003)) < 1e-6


def test_stopping(model):
    est = IC.batch_poses(7)
    D = _noisy_depth()
    behind = IC.moved(IC.ICO_G, (0, 0, -0.5))
    beyond = IC.pose(t=(5000.0, 0.0, 0.12))
    model.upload_frame(RGB, D)
    P, recs = _refine(model, "ico2", [est[0], behind, est[1], beyond, est[2]], iterations=4)
    assert recs[1].status == IR.REFUSED_NEAR and recs[3].status == IR.REFUSED_RANGE
    for i, bad in ((1, behind), (3, beyond)):
        assert P[i].tobytes() == np.asarray(bad, np.float32).tobytes()
        assert _bytes(recs[i]) == bytes(_lib.FpDepthRefine(status=recs[i].status))      # every other field 0
    Pc, clean = _refine(model, "ico2", est[:3], iterations=4)
    assert P[[0, 2, 4]].tobytes() == Pc.tobytes() and _bytes([recs[0], recs[2], recs[4]]) == _bytes(clean)      # the neighbours do not notice
    # fewer than 32 used pixels: a depth with 20 valid pixels on the object
    few = np.zeros_like(D)
    rows, cols = np.nonzero(IC.rendering(IC.ico(2), IC.ICO_G) != IC.WALL)
    few[rows[100:120], cols[100:120]] = D[rows[100:120], cols[100:120]]
    model.upload_frame(RGB, few)
    P, (r,) = _refine(model, "ico2", [est[0]], iterations=4)
    _show("too few", r)
    assert r.status == IR.TOO_FEW and r.iterations == 0 and 0 < r.n_valid <= 20 and r.n_used < _const("FP_ICP_MIN_PIXELS") == IR.MIN_PIXELS
    assert P[0].tobytes() == est[0].tobytes()
    # one update allowed: it is applied, the record is that of the updated pose
    model.upload_frame(RGB, D)
    P, (r,) = _refine(model, "ico2", [est[0]], iterations=1)
    ref = IR.sums(FR.centred(IC.ico(2)), IC.ico(2).faces, P[0], IC.K, D, IC.GATE, IC.ico(2).diameter)
    assert r.iterations == 1 and P[0].tobytes() != est[0].tobytes() and list(r.sums_q32) == ref["sums"]


def test_refusals_leave_the_outputs_untouched():
    G = np.asarray(IC.ICO_G, np.float32)
    max_batch, cap = _const("FP_MAX_BATCH"), int(re.search(r"#define FP_ICP_MAX_WORK (\d+)LL", HEADER).group(1))
    # the work cap: every pose so near that its bound is the whole 1920 x 1080 frame (2040 tiles), a mesh of F degenerate faces
    tiles, passes = 60 * 34, 33
    F = cap // (max_batch * tiles * passes) + 1
    base = IC.plate()
    many = syn.Mesh("many", base.vertices, base.normals, base.texcoords, np.zeros((F, 3), np.int32), base.texture).finalize()
    near = IC.pose(t=(0.0, 0.0, 0.03))
    m = FoundationPose([IC.ico(2), many], IC.K)
    try:
        def refused(match, name, poses, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(poses).reshape(-1, 4, 4)))
            out = (_lib.FpDepthRefine * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            out_p = np.full((n, 16), 7.5, np.float32)
            rc, _, _ = _raw(m, name, poses, out=out, out_p=out_p, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert _bytes(out) == b"\x5a" * C.sizeof(out) and (out_p == 7.5).all()

        refused("no frame uploaded", "ico2", [G])
        m.upload_frame(RGB, IC.rendering(IC.ico(2), G))
        assert _raw(m, "ico2", [G])[0] == 0
        refused("unknown target_name", "nobody", [G])
        refused(r"1\.\.FP_MAX_BATCH", "ico2", [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", "ico2", [G] * (max_batch + 1))
        refused(r"0\.\.FP_ICP_MAX_ITERATIONS", "ico2", [G], iterations=-1)
        refused(r"0\.\.FP_ICP_MAX_ITERATIONS", "ico2", [G], iterations=33)
        assert _raw(m, "ico2", [G], iterations=32)[0] == 0
        for value in (float("nan"), float("inf"), 0.0, -0.01, float(np.float32(IC.ico(2).diameter)) * 1.001):
            refused("max_dist_m", "ico2", [G], gate=value)
        assert _raw(m, "ico2", [G], gate=float(np.float32(IC.ico(2).diameter)))[0] == 0
        refused("unknown flag bits", "ico2", [G], flags=2)
        refused("unknown flag bits", "ico2", [G], flags=-1)
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(G)
                bad[where] = value
                refused(r"non-finite.*poses\[1\]", "ico2", [G, bad])
        # the cap: FP_MAX_BATCH poses over the whole of a large frame for 33 evaluations are one face too many; nothing is launched
        m.upload_frame(np.zeros((1080, 1920, 3), np.uint8), np.zeros((1080, 1920), np.float32))
        assert max_batch * tiles * passes * F > cap >= max_batch * tiles * passes * (F - 1)
        refused("FP_ICP_MAX_WORK", "many", [near] * max_batch, iterations=32)
        rc, _, out = _raw(m, "many", [near], iterations=32)
        assert rc == 0 and out[0].n_model == 0 and out[0].status == IR.TOO_FEW
    finally:
        m.close()


def test_the_depth_filter_does_not_reach_the_call():
    mesh, P, D = IC.record_case("nan_and_zero")
    m = FoundationPose(IC.ico(2), IC.K)
    try:
        m.upload_frame(RGB, D)
        off = _refine(m, mesh, [P], iterations=3)
        m.set_depth_filter(True)
        on = _refine(m, mesh, [P], iterations=3)
        m.upload_frame(RGB, D)
        again = _refine(m, mesh, [P], iterations=3)
        assert off[0].tobytes() == on[0].tobytes() == again[0].tobytes() and _bytes(off[1]) == _bytes(on[1]) == _bytes(again[1])
    finally:
        m.close()


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


def test_serving_path_is_untouched(tl, disc_nets, syn_mesh, syn_scene):
    """a Register followed by a Track after the call equals one before it, bit for bit and launch for launch; a Track from a host frame
    leaves only its crop window, and a submitted Track is pending: both refuse the call"""
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
        m.upload_frame(syn_scene.rgb, syn_scene.depth)   # (as before the call below: both logged rounds follow an upload)
        (_, pose), log_before = _logged(tl, serve)
        out = (_lib.FpDepthRefine * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        out_p = np.full((1, 16), 7.5, np.float32)
        start = syn.perturb_pose(syn_scene.gt_pose, deg=4.0, trans=0.008)
        rc, _, _ = _raw(m, syn_mesh.name, [start], iterations=3, out=out, out_p=out_p)
        assert rc != 0 and "only its crop window" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out) and (out_p == 7.5).all()
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        P, recs = m.refine_depth(syn_mesh.name, [start, syn_scene.gt_pose], iterations=8)
        for k in (0, 1):
            deg, dist = IR.pose_gap(P[k], syn_scene.gt_pose)
            print(f"640 x 480, pose {k}: {deg:.3f} deg {dist * 1e3:.3f} mm from the truth, n_used {recs[k].n_used}, rms {recs[k].rms_m * 1e3:.3f} mm")
            assert recs[k].n_used > 600 and recs[k].rank == 6 and recs[k].rms_m < 2e-3
        assert IR.pose_gap(P[0], syn_scene.gt_pose)[1] < IR.pose_gap(start, syn_scene.gt_pose)[1]
        after, log_after = _logged(tl, serve)
        assert after[0] == before[0][0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        rc, _, _ = _raw(m, syn_mesh.name, [start], out=out, out_p=out_p)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out) and (out_p == 7.5).all()
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        # the profiler's families: one vertex and one tile scope per evaluation
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        m.profile_reset(); m.profile(True)
        m.refine_depth(syn_mesh.name, [start], iterations=0)
        rep = m.profile_report()
        m.profile(False)
        assert rep["icp_vertex"]["calls"] == 1 and rep["icp_tile"]["calls"] == 1
    finally:
        m.close()


def test_through_the_python_interface(model):
    est = IC.batch_poses(3)
    D = _noisy_depth()
    model.upload_frame(RGB, D)
    P, recs = model.refine_depth("ico2", est, iterations=6)
    Pr, raw = _refine(model, "ico2", est, iterations=6)
    assert P.shape == (3, 4, 4) and P.dtype == np.float32 and P.tobytes() == Pr.tobytes()
    assert all(isinstance(r, DepthRefine) for r in recs)
    for r, w in zip(recs, raw):
        assert [getattr(r, k) for k in IR.COUNTS + ("iterations", "rank", "status")] == [getattr(w, k) for k in IR.COUNTS + ("iterations", "rank", "status")]
        assert r.sums_q32 == tuple(w.sums_q32) and len(r.sums_q32) == 28 and r.rms_m == float(w.rms_m)
    Pt, rt = model.refine_depth("ico2", est[:1], iterations=6, translation_only=True)
    assert Pt[0, :3, :3].tobytes() == est[0, :3, :3].tobytes() and rt[0].rank == 3 and Pt[0, :3, 3].tobytes() != est[0, :3, 3].tobytes()
    P0, r0 = model.refine_depth("ico2", est[:1], iterations=0)
    assert P0[0].tobytes() == est[0].tobytes() and r0[0].iterations == 0
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.refine_depth("nobody", est)
