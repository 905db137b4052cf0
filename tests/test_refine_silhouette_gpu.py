"""fp_refine_silhouette against tests/silref_ref.py.  One evaluation is held to the f32 restatement (a) EXACTLY:
every count, every one of the 28 sums, the status, and the bits of rms_px and scale_px.  After updates the device's host solve (Jacobi, in
C++) and the reference's (numpy.linalg.eigh) round differently, so the returned record is held to (a) evaluated AT THE RETURNED POSE,
again exactly, and the returned pose to silref32's within a bound measured once (silref_cases.AB_BOUND_*).  Then the promises of the
interface: byte-identical records and poses whatever the batch, the chunking or the memory space of the mask, refusals per record and
per call, the untouched serving path, and neighbours on one model that leave nothing behind."""
import ctypes as C
import os
import re
from unittest import mock

import numpy as np
import pytest

import camera_cases as CC
import icp_cases as IC
import icp_ref as IR
import silhouette_cases as SIC
import silref_cases as SC
import silref_ref as RR
import test_stage_scratch_gpu as SS
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, SilhouetteRefine, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
FP_HOST, FP_DEVICE = 0, 1
f32 = np.float32


def _raw(m, name, mask, poses, iterations=0, gate=0, tol=SC.TOL, flags=0, N=None, out=None, out_p=None, memspace=FP_HOST):
    """fp_refine_silhouette through the raw ABI -> (return code, poses [N,4,4], records)"""
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out = (_lib.FpSilhouetteRefine * max(N, 1))() if out is None else out
    out_p = np.zeros((max(N, 1), 16), np.float32) if out_p is None else out_p
    if isinstance(mask, np.ndarray):
        mask = np.ascontiguousarray(mask, np.uint8)
        ptr = _p(mask)
    else:
        ptr = mask
    rc = m._L.fp_refine_silhouette(m._h, None if name is None else name.encode(), ptr, memspace, _p(e), N, iterations, gate, tol, flags, _p(out_p), out)
    return rc, out_p, out


def _ref(m, name, mask, poses, **kw):
    rc, out_p, out = _raw(m, name, mask, poses, **kw)
    m._must(rc)
    return syn.from_colmajor(out_p), list(out)


def _bytes(result):
    poses, recs = result
    return np.ascontiguousarray(poses).tobytes() + b"".join(bytes(r) for r in recs)


def _run_case(m, name, iterations=None, **kw):
    c = SC.case(name)
    m.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    return _ref(m, c["mesh"].name, c["mask"], c["poses"], iterations=c["iterations"] if iterations is None else iterations, gate=c["gate_px"], tol=c["tol"],
                flags=c["flags"], **kw)


def _equal(what, got, ev):
    """one device record against (a)'s evaluation at the pose the record describes: every integer, the bits of rms_px and scale_px"""
    print(f"{what}: device " + " ".join(f"{k}={getattr(got, k)}" for k in RR.INTS) + f" rms_px={float(got.rms_px):.5f}")
    if isinstance(ev, int):
        assert got.status & 12 == ev and all(getattr(got, k) == 0 for k in RR.COUNTS), (what, got.status, ev)
        return
    for k in RR.COUNTS:
        assert getattr(got, k) == ev[k], (what, k, getattr(got, k), ev[k])
    assert list(got.sums_q24) == ev["sums"], (what, list(got.sums_q24), ev["sums"])
    assert got.status & 12 == 0
    assert f32(got.scale_px).tobytes() == f32(ev["scale_px"]).tobytes()
    assert f32(got.rms_px).tobytes() == RR.rms_px(ev["sums"], ev["n_used"], ev["scale_px"]).tobytes()
    assert got.reserved_f == 0.0


@pytest.fixture(scope="module")
def model():
    import search_cases as SE
    m = FoundationPose([IC.ico(1), IC.ico(2), SE.mesh(), SIC.hand_quad(), SC.wedge()], SC.K)          # geometry-only
    yield m
    m.close()


# ---- one evaluation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.RECORD_CASES)
def test_one_evaluation_equals_the_reference(model, name):
    c = SC.case(name)
    poses, recs = _run_case(model, name, iterations=0)
    assert np.array_equal(poses, np.asarray(c["poses"], f32))                        # I = 0 measures only
    for i, (g, ev) in enumerate(zip(recs, SC.expected0(name))):
        _equal(f"{name}[{i}]", g, ev)
        assert g.iterations == 0 and g.rank == 0 and g.cond == 0.0 and g.status & 3 == 0


def test_the_hand_case(model):
    _, recs = _run_case(model, "hand", iterations=0)
    assert {k: getattr(recs[0], k) for k in RR.COUNTS} == SC.HAND
    assert abs(float(recs[0].rms_px) - SC.HAND_RMS_PX) < 1e-5
    poses, recs = _run_case(model, "hand", iterations=1)
    assert SC.HAND_STEP_X_M[0] <= float(poses[0][0, 3]) <= SC.HAND_STEP_X_M[1] and recs[0].rank == 3 and recs[0].iterations == 1
    poses, recs = _run_case(model, "hand", iterations=2)                              # three evaluations
    assert recs[0].n_used == 44 and recs[0].rms_px == 0.0 and list(recs[0].sums_q24)[21:] == [0] * 7
    poses, recs = _run_case(model, "hand", iterations=8)                              # the exact fixed point: the update is exactly 0
    assert recs[0].status == RR.CONVERGED and recs[0].iterations == 3 and recs[0].last_rot_rad == 0.0 and recs[0].last_trans_m == 0.0


# ---- after updates -------------------------------------------------------------------------------------------------------------------------
def _gap_report(name, poses, refs):
    worst = (0.0, 0.0)
    for i, (P, r) in enumerate(zip(poses, refs)):
        deg, met = IR.pose_gap(P, r["pose"])
        print(f"{name}[{i}]: device against silref32 {deg:.5f} deg {met * 1e3:.8f} mm")
        worst = (max(worst[0], deg), max(worst[1], met))
    return worst


@pytest.mark.parametrize("name", SC.ITERATED_CASES)
def test_the_returned_record_describes_the_returned_pose(model, name):
    c = SC.case(name)
    poses, recs = _run_case(model, name)
    refs = SC.iterated(name)
    for i, (P, g, r) in enumerate(zip(poses, recs, refs)):
        _equal(f"{name}[{i}] at the returned pose", g, SC.evaluate(c, P))
        assert g.status == r["status"] and g.iterations == r["iterations"], (name, i, g.status, r["status"], g.iterations, r["iterations"])
        if g.status & 12:
            assert np.array_equal(P, np.asarray(c["poses"][i], f32))                 # refused at the input: returned as it came
    deg, met = _gap_report(name, poses, refs)
    assert deg <= SC.AB_BOUND_DEG and met <= SC.AB_BOUND_M


@pytest.mark.parametrize("seed", SC.WEDGE_SEEDS)
def test_the_wedge_ends_at_the_truth(model, seed):
    name = f"wedge_{seed}"
    c = SC.case(name)
    poses, recs = _run_case(model, name)
    for k in (0, 1):
        end = SC.mssd(SC.wedge(), poses[k], SC.wedge_truth(seed))
        ref = SC.wedge_refined(seed, k)
        deg, met = IR.pose_gap(poses[k], ref["pose"])
        print(f"wedge {seed} start {k}: device {end * 1e3:.3f} mm from the truth (reference {SC.REF_MSSD_MM[(seed, k)]} mm), {recs[k].iterations} updates, "
              f"rms {float(recs[k].rms_px):.4f} px; against silref32 {deg:.5f} deg {met * 1e3:.8f} mm")
        assert end <= SC.BOUND_M
        _equal(f"{name}[{k}] at the returned pose", recs[k], SC.evaluate(c, poses[k]))
        assert deg <= SC.AB_BOUND_DEG and met <= SC.AB_BOUND_M


def test_a_general_camera(model):
    """fx != fy and a principal point off centre (tests/camera_cases.py): one evaluation and three updates, each record exact"""
    cc = CC.camera_case(2)
    mask = np.where(CC.model_depth(cc.mesh, cc.G[0], cc.K, cc.H, cc.W) != 0, 255, 0).astype(np.uint8)
    sd = RR.signed_map(mask)
    assert cc.K[0, 0] != cc.K[1, 1]
    m = FoundationPose(cc.mesh, cc.K)
    try:
        m.upload_frame(cc.rgb, cc.depth)
        for iterations in (0, 3):
            poses, recs = _ref(m, cc.mesh.name, mask, cc.E, iterations=iterations)
            for i, (P, g) in enumerate(zip(poses, recs)):
                _equal(f"camera 2 pose {i}, {iterations} iterations", g, RR.sums(RR.FR.centred(cc.mesh), cc.mesh.faces, P, cc.K, sd, cc.mesh.diameter))
            assert any(g.n_used > 50 for g in recs)
    finally:
        m.close()


# ---- byte identity -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tl():
    """the test build (its chunk hooks and launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    for hook in ("fpt_silref_set_chunk", "fpt_silhouette_set_chunk", "fpt_color_set_chunk", "fpt_vsd_set_chunk", "fpt_icp_set_chunk"):
        getattr(L, hook).argtypes = [C.c_int]
        getattr(L, hook).restype = None
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_silref_set_chunk(0)


def test_batches_across_chunk_boundaries(tl):
    """47 poses at 2 iterations whole and in chunks of 1, 2 and 7; 512 poses whole and in chunks of 100: the same bytes"""
    c = SC.case("batch_47")
    m = FoundationPose(c["mesh"], SC.K)
    try:
        m.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
        whole = _ref(m, c["mesh"].name, c["mask"], c["poses"], iterations=2)
        assert len({bytes(r) for r in whole[1]}) > 40                                # (the poses do differ)
        for chunk in (1, 2, 7):
            tl.fpt_silref_set_chunk(chunk)
            assert _bytes(_ref(m, c["mesh"].name, c["mask"], c["poses"], iterations=2)) == _bytes(whole), chunk
        tl.fpt_silref_set_chunk(0)
        big = SC.case("batch_512")
        many = _ref(m, big["mesh"].name, big["mask"], big["poses"], iterations=2)
        tl.fpt_silref_set_chunk(100)
        assert _bytes(_ref(m, big["mesh"].name, big["mask"], big["poses"], iterations=2)) == _bytes(many)
        tl.fpt_silref_set_chunk(0)
        assert np.array_equal(big["poses"][:47], c["poses"])                          # pose i alone, among 47 and among 512
        assert many[0][:47].tobytes() == whole[0].tobytes() and b"".join(bytes(r) for r in many[1][:47]) == b"".join(bytes(r) for r in whole[1])
        for i in range(47, 512, 31):
            _equal(f"batch_512[{i}] at the returned pose", many[1][i], SC.evaluate(big, many[0][i]))
    finally:
        m.close()


def test_a_pose_is_the_same_alone_in_any_batch_and_again(model):
    c = SC.case("ragged")
    name, poses, mask = c["mesh"].name, c["poses"], c["mask"]
    model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    batch = _ref(model, name, mask, poses, iterations=3, gate=5)
    assert _bytes(batch) == _bytes(_ref(model, name, mask, poses, iterations=3, gate=5))          # call to call
    three = _ref(model, name, mask, poses[[0, 3, 6]], iterations=3, gate=5)
    for k, i in enumerate((0, 3, 6)):
        alone = _ref(model, name, mask, poses[i:i + 1], iterations=3, gate=5)
        assert _bytes(alone) == _bytes((batch[0][i:i + 1], batch[1][i:i + 1])) == _bytes((three[0][k:k + 1], three[1][k:k + 1])), i


def test_a_device_mask_gives_the_same(model):
    import torch
    c = SC.case("ragged")
    model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    dev = torch.from_numpy(np.ascontiguousarray(c["mask"])).cuda()
    torch.cuda.synchronize()
    host = _ref(model, c["mesh"].name, c["mask"], c["poses"], iterations=2)
    there = _ref(model, c["mesh"].name, C.c_void_p(dev.data_ptr()), c["poses"], iterations=2, memspace=FP_DEVICE)
    assert _bytes(host) == _bytes(there)
    assert np.array_equal(dev.cpu().numpy(), c["mask"])                              # the caller's mask is not modified


def test_refused_poses_do_not_disturb_their_neighbours(model):
    c = SC.case("refused")
    poses, recs = _run_case(model, "refused")
    assert [g.status & 12 for g in recs] == [0, RR.REFUSED_NEAR, 0, RR.REFUSED_RANGE, 0]
    for i in (1, 3):
        assert np.array_equal(poses[i], np.asarray(c["poses"][i], f32))
        assert bytes(recs[i])[:36] == b"\0" * 36 and bytes(recs[i])[40:] == b"\0" * 248
    clean = _ref(model, c["mesh"].name, c["mask"], c["poses"][[0, 2, 4]], iterations=c["iterations"])
    assert _bytes((poses[[0, 2, 4]], [recs[0], recs[2], recs[4]])) == _bytes(clean)
    # a pose whose ORIGIN is nearer than the near constant has no scale: refused like one with such a vertex
    origin_near = IC.pose(t=(0.0, 0.0, 0.005))
    p2, r2 = _ref(model, c["mesh"].name, c["mask"], [origin_near], iterations=2)
    assert r2[0].status == RR.REFUSED_NEAR and np.array_equal(p2[0], np.asarray(origin_near, f32))


def test_an_outline_that_leaves_stops_the_pose(model):
    """wholly outside the frame: no contour, TOO_FEW, the pose comes back as it went in"""
    c = SC.case("outside")
    poses, recs = _run_case(model, "outside", iterations=4)
    assert recs[0].status == RR.TOO_FEW and recs[0].iterations == 0 and all(getattr(recs[0], k) == 0 for k in RR.COUNTS)
    assert np.array_equal(poses[0], np.asarray(c["poses"][0], f32))


# ---- refusals of the call --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    c = SC.case("ragged")
    G, mask = c["poses"][0], c["mask"]
    max_batch, cap = int(re.search(r"#define FP_MAX_BATCH (\d+)", HEADER).group(1)), int(re.search(r"#define FP_SILREF_MAX_WORK (\d+)LL", HEADER).group(1))
    tiles = 60 * 34                                                                   # a bound that is the whole 1920 x 1080 frame
    F = cap // (max_batch * tiles * 33) + 1
    base = c["mesh"]
    many = syn.Mesh("many", base.vertices, base.normals, base.texcoords, np.zeros((F, 3), np.int32), base.texture).finalize()
    near = IC.pose(np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), (0.0, 0.0, 0.09))   # the bounding sphere reaches the camera plane, no vertex does
    m = FoundationPose([base, many], SC.K)
    skew = np.array(SC.K, np.float32)
    skew[0, 1] = 0.5
    ms = FoundationPose(base, skew)
    try:
        def refused(match, *a, model=m, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(a[2]).reshape(-1, 4, 4)))
            out = (_lib.FpSilhouetteRefine * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            out_p = np.full((n, 16), 7.5, np.float32)
            rc, _, _ = _raw(model, *a, out=out, out_p=out_p, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert bytes(out) == b"\x5a" * C.sizeof(out) and (out_p == 7.5).all()

        refused("fp_refine_silhouette: no frame uploaded", base.name, mask, [G])
        rgb = np.zeros(c["D"].shape + (3,), np.uint8)
        m.upload_frame(rgb, c["D"])
        ms.upload_frame(rgb, c["D"])
        assert _raw(m, base.name, mask, [G])[0] == 0
        refused(r"fp_refine_silhouette: the model's K is not a plain pinhole matrix: K\[1\]", base.name, mask, [G], model=ms)
        refused("unknown target_name", "nobody", mask, [G])
        refused("fp_refine_silhouette: invalid arguments", base.name, None, [G])
        refused("fp_refine_silhouette: memspace", base.name, mask, [G], memspace=7)
        refused(r"fp_refine_silhouette: 0 poses \(1\.\.FP_MAX_BATCH", base.name, mask, [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", base.name, mask, [G] * (max_batch + 1))
        for value in (-1, 33):
            refused("fp_refine_silhouette: -?\\d+ iterations", base.name, mask, [G], iterations=value)
        assert _raw(m, base.name, mask, [G], iterations=32)[0] == 0
        for value in (float("nan"), float("inf"), -0.01):
            refused("fp_refine_silhouette: tol_m", base.name, mask, [G], tol=value)           # checked where it is not used ...
            refused("fp_refine_silhouette: tol_m", base.name, mask, [G], tol=value, flags=RR.OCCLUSION)   # ... and where it is
        assert _raw(m, base.name, mask, [G], tol=0.0)[0] == 0
        for value in (-1, 32768):
            refused("fp_refine_silhouette: gate_px", base.name, mask, [G], gate=value)
        assert _raw(m, base.name, mask, [G], gate=32767)[0] == 0
        for value in (4, 7, -1, 1 << 20):
            refused("fp_refine_silhouette: unknown flag bits", base.name, mask, [G], flags=value)
        for value in (float("nan"), float("inf")):
            bad = np.array(G)
            bad[2, 3] = value
            refused(r"fp_refine_silhouette: a non-finite entry in poses\[1\]", base.name, mask, [G, bad])
        # a mask without an outline: the call fails after the transform, before anything is written
        refused("fp_refine_silhouette: the mask is empty", base.name, np.zeros_like(mask), [G], iterations=2)
        refused("fp_refine_silhouette: the mask covers the whole frame", base.name, np.full_like(mask, 3), [G], iterations=2)
        # the cap counts every evaluation: FP_MAX_BATCH poses over the whole of a large frame, 33 evaluations, one face too many
        big = np.zeros((1080, 1920), np.uint8)
        big[500:600, 900:1000] = 1
        m.upload_frame(np.zeros((1080, 1920, 3), np.uint8), np.zeros((1080, 1920), np.float32))
        assert max_batch * tiles * F * 33 > cap >= max_batch * tiles * (F - 1) * 33
        refused("FP_SILREF_MAX_WORK", "many", big, [near] * max_batch, iterations=32)
        rc, _, out = _raw(m, "many", big, [near], iterations=1)
        assert rc == 0 and out[0].n_model == 0 and out[0].status == RR.TOO_FEW
    finally:
        m.close()
        ms.close()


# ---- the rest of the library ----------------------------------------------------------------------------------------------------------------
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
    leaves only its crop window, and a submitted Track is pending: both refuse fp_refine_silhouette"""
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
        out = (_lib.FpSilhouetteRefine * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _, _ = _raw(m, syn_mesh.name, syn_scene.mask, [pose], out=out)
        assert rc != 0 and "only its crop window" in _lib.last_error() and bytes(out) == b"\x5a" * C.sizeof(out)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        start = syn.perturb_pose(syn_scene.gt_pose, deg=2.0, trans=0.004)
        m.profile_reset(); m.profile(True)
        poses, recs = m.refine_silhouette(syn_mesh.name, syn_scene.mask, [start], iterations=3, translation_only=True)
        rep = m.profile_report()
        m.profile(False)
        for fam in ("mask_edt_cols", "mask_edt_rows", "mask_signed_d2"):
            assert rep[fam]["calls"] == 1, fam
        for fam in ("silref_vertex", "silref_tile"):
            assert rep[fam]["calls"] == 4, fam             # one per evaluation
        first = m.refine_silhouette(syn_mesh.name, syn_scene.mask, [start], iterations=0)[1][0]
        assert isinstance(recs[0], SilhouetteRefine) and recs[0].iterations == 3 and recs[0].rank == 3 and recs[0].n_used > 100
        print(f"640 x 480 scene: rms {first.rms_px:.3f} px -> {recs[0].rms_px:.3f} px in three translation-only updates")
        assert recs[0].rms_px < first.rms_px
        after, log_after = _logged(tl, serve)
        assert after[0] == before[0][0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        rc, _, _ = _raw(m, syn_mesh.name, syn_scene.mask, [pose], out=out)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and bytes(out) == b"\x5a" * C.sizeof(out)
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
    finally:
        m.close()


def _sil(m, name, mask, poses):
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    out = (_lib.FpPoseSilhouette * len(e))()
    m._must(m._L.fp_pose_silhouette(m._h, name.encode(), _p(mask), FP_HOST, _p(e), len(e), SC.TOL, 0, 0, out))
    return bytes(out)


def test_neighbours_on_one_model_leave_nothing_behind(tl):
    """in the spirit of tests/test_stage_scratch_gpu.py (its window, its poses): fp_refine_silhouette between fp_pose_silhouette,
    fp_refine_depth and fp_mask_distance on ONE model, each equal to the same call on a fresh model"""
    small, large = syn.make_mesh(1, textured=True, name="ico1t"), syn.make_mesh(3, textured=True, name="ico3t")
    mask = np.zeros((SS.H, SS.W), np.uint8)
    mask[20:60, 30:75] = 255
    other = np.zeros((SS.H, SS.W), np.uint8)
    other[10:50, 20:70] = 1

    def fresh():
        m = FoundationPose([small, large], SS.K)
        m.upload_frame(SS.RGB, SS.DEPTH)
        return m

    steps = [("refine_silhouette, large mesh, chunks of 2", {"fpt_silref_set_chunk": 2}, lambda m: _bytes(_ref(m, large.name, mask, SS.EST, iterations=2))),
             ("pose_silhouette, large mesh, another mask", {"fpt_silhouette_set_chunk": 2}, lambda m: _sil(m, large.name, other, SS.EST)),
             ("refine_silhouette, small mesh, occlusion", {}, lambda m: _bytes(_ref(m, small.name, mask, SS.EST[:2], iterations=1, flags=RR.OCCLUSION))),
             ("refine_depth, small mesh, chunks of 2", {"fpt_icp_set_chunk": 2}, lambda m: SS._refine(m, small.name, SS.EST, 2)),
             ("mask_distance", {}, lambda m: b"".join(a.tobytes() for a in m.mask_distance(other))),
             ("refine_silhouette, small mesh, gate", {}, lambda m: _bytes(_ref(m, small.name, mask, SS.EST, iterations=2, gate=4))),
             ("pose_silhouette, small mesh", {}, lambda m: _sil(m, small.name, mask, SS.EST[:2]))]
    shared = fresh()
    try:
        got = [SS._run(tl, shared, s) for s in steps]
    finally:
        shared.close()
    assert len(set(got)) == len(got)
    for s, mine in zip(steps, got):
        m = fresh()
        try:
            ref = SS._run(tl, m, s)
        finally:
            m.close()
        assert mine == ref, s[0]
    sd = RR.signed_map(mask)
    P = np.frombuffer(got[0][:64], np.float32).reshape(4, 4)                    # (_bytes holds the poses as numpy has them)
    first = _lib.FpSilhouetteRefine.from_buffer_copy(got[0][3 * 64:3 * 64 + 288])
    _equal("refine_silhouette on the shared model", first, RR.sums(RR.FR.centred(large), large.faces, P, SS.K, sd, large.diameter))


def test_through_the_python_interface(model):
    c = SC.case("ragged")
    model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    poses, recs = model.refine_silhouette(c["mesh"].name, c["mask"], c["poses"], iterations=2, gate_px=6, translation_only=True, occlusion=True)
    raw = _ref(model, c["mesh"].name, c["mask"], c["poses"], iterations=2, gate=6, flags=3)
    assert poses.shape == (7, 4, 4) and poses.dtype == np.float32 and np.array_equal(poses, raw[0])
    assert len(recs) == 7 and all(isinstance(r, SilhouetteRefine) for r in recs)
    for r, w in zip(recs, raw[1]):
        assert [getattr(r, k) for k in RR.INTS] == [getattr(w, k) for k in RR.INTS] and r.sums_q24 == tuple(w.sums_q24)
        assert r.rank in (0, 3)
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.refine_silhouette("nobody", c["mask"], c["poses"])
    with pytest.raises(FoundationPoseError, match="a mask of shape"):
        model.refine_silhouette(c["mesh"].name, c["mask"][:-1], c["poses"])
