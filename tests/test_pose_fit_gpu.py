"""The pose fit (fp_set_pose_fit / fp_last_track_fit / fp_last_register_fit / fp_pose_fit_eval) on the device.

  exact     every field of every record equals tests/pose_fit_ref.py of the networks' input tensor of the SAME call (the test build's
            TAP_NN_IN tap; fp_pose_fit_eval runs no network, its tensor is read back from the model's buffer), over an eager, a capturing
            and a replayed call, whose tensors and records are equal bit for bit
  oracle    no device tensor involved: the counts lie in [certain, certain + uncertain] of pose_fit_ref.certain_counts over the oracle's
            render / crop (tests/test_pose_fit_ref_cpu.py holds the uncertain share of these scenes under 2 %)
  meaning   ground truth, poses pushed along the camera ray, an occluder, missing depth
  off       with the option never enabled nothing changes, bit for bit
  errors    every refusal returns non-zero with a message"""
import ctypes as C
import dataclasses
import gc
from unittest import mock

import numpy as np
import pytest
import torch

import nn_in_ref as R
import pose_fit_ref as PF
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, FP_HOST, FP_PREC_BF16, FP_PREC_F16, _p
from oracle import fp_oracle as fo
from pose_fit_ref import TOL_M, gpu_scenes

pytestmark = pytest.mark.gpu

TAP_NN_IN = 0
DEV = "cuda"
PREC = {R.F16: FP_PREC_F16, R.BF16: FP_PREC_BF16}
NAME = {R.F16: "f16", R.BF16: "bf16"}
DTS = [R.F16, R.BF16]
FP_MAX_BATCH = 2377
PHASES = ("eager", "capturing", "replayed")


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_tap_arm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.fpt_tap_bytes.restype = C.c_longlong
    L.fpt_tap_bytes.argtypes = [C.c_int, C.c_int]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    L.fpt_model_graph_state.argtypes = [C.c_void_p]
    L.fpt_read_buffer.restype = C.c_longlong
    L.fpt_read_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
    L.fpt_digests.argtypes = [C.c_void_p, C.c_void_p]
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    yield L
    L.fpt_tap_clear()


@pytest.fixture(scope="module", autouse=True)
def _test_build_is_the_library(tl):
    """every model here lives on the TEST build, and fp_last_error is thread-local PER LIBRARY: the messages the refusals are matched
    against have to be read from the build that refused (api._ok asks _lib.lib())"""
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield


def _new_model(tl, meshes, K, nets, **kw):
    """a model on the TEST build (its taps act on this instance); graph replay stays ON"""
    return FoundationPose(meshes, K, nets[0], nets[1], **kw)


@pytest.fixture(scope="module")
def model(tl, disc_nets, syn_mesh):
    m = _new_model(tl, syn_mesh, syn.intrinsics(), disc_nets)
    yield m
    m.close()


@pytest.fixture(scope="module")
def om(syn_mesh):
    return fo.OracleMesh(syn_mesh)


@pytest.fixture(autouse=True)
def _free_cached_blocks():
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _same(case, got, ref):
    """every field of a device record against the reference's, bit for bit"""
    g = (got.n_model, got.n_observed, got.n_inlier, got.n_front, got.n_behind, got.sum_dz_q20, np.float32(got.mean_dz_m).tobytes(), np.float32(got.tol_n).tobytes())
    r = ref.ints() + (np.float32(ref.mean_dz_m).tobytes(), np.float32(ref.tol_n).tobytes())
    assert g == r, (case, got, ref)
    assert got.n_observed == got.n_inlier + got.n_front + got.n_behind, (case, got)


def _three_phases(tl, model, dt, case, call, fetch, kind, nb2, n, tol, diam, graph_bit):
    """call() three times from dropped graphs -- eager, capturing, replayed -- with TAP_NN_IN of the refiner's (kind 0) or the scorer's (1)
    pass armed on ONE buffer (the captured graph keeps the copy into it): the three tensors are equal bit for bit, so are the records, and
    the records equal pose_fit_ref of the tensor; -> the records"""
    assert tl.fpt_model_use_graphs(model._h, 1) == 0        # drops the graphs: the next call is the eager one
    tl.fpt_tap_clear()
    t = torch.empty((nb2, R.P, R.P, 32), dtype=R.TORCH_DT[dt], device=DEV)
    nbytes = t.numel() * t.element_size()
    assert tl.fpt_tap_arm(kind, TAP_NN_IN, C.c_void_p(t.data_ptr()), nbytes) == 0
    first_t = first_r = None
    try:
        for phase in PHASES:
            t.fill_(float("nan"))
            torch.cuda.synchronize()
            call()
            torch.cuda.synchronize()
            assert tl.fpt_tap_bytes(kind, TAP_NN_IN) == nbytes, (case, phase)      # the tap was reached, with the size expected
            got = t.cpu()
            recs = fetch()
            assert len(recs) == n
            if first_t is None:
                first_t, first_r = got, recs
                refs = PF.pose_fit_batch(got, n, tol, diam)
                for i in range(n):
                    _same(f"{case} {phase} record {i}", recs[i], refs[i])
                assert sum(r.n_model for r in recs) > 0, case
            else:
                assert torch.equal(got.view(torch.int16), first_t.view(torch.int16)), (case, phase)
                assert recs == first_r, (case, phase)
            del got
        if graph_bit:
            assert tl.fpt_model_graph_state(model._h) & graph_bit, f"{case}: the third call did not replay a graph"
    finally:
        tl.fpt_tap_clear()
        tl.fpt_model_use_graphs(model._h, 1)                # (the captured graph holds a copy into this test's buffer)
    return first_r


def _track_call(model, mesh, rgb, depth, pose, itr, how):
    hw = depth.shape
    p16 = syn.to_colmajor(np.asarray(pose, np.float32)[None])[0]
    out = np.zeros(16, np.float32)
    if how == "device":
        r_d, d_d = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
        model._must(model._L.fp_track_ex(model._h, C.c_void_p(r_d.data_ptr()), C.c_void_p(d_d.data_ptr()), FP_DEVICE, hw[0], hw[1], _p(p16),
                                         mesh.name.encode(), itr, _p(out)))
        torch.cuda.synchronize()
    elif how == "submit":
        assert model.track_submit(rgb, depth, pose, mesh.name, itr), model.last_error
        with pytest.raises(FoundationPoseError, match="not been waited for"):
            model.last_track_fit()
        ok, _ = model.track_wait()
        assert ok, model.last_error
    else:
        ok, _ = model.Track(rgb, depth, pose, mesh.name, itr)
        assert ok, model.last_error


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("how,itr", [("host", 1), ("host", 2), ("device", 1), ("device", 2), ("submit", 1)])
def test_track_records_equal_the_reference_of_the_tapped_tensor(tl, model, syn_mesh, syn_scene, dt, how, itr):
    """refine_itr 2: the tap holds the LAST iteration's input, and so does the record"""
    model.set_precision(PREC[dt])
    model.set_pose_fit(True, TOL_M)
    try:
        pose = syn.perturb_pose(syn_scene.gt_pose)
        recs = _three_phases(tl, model, dt, f"Track {NAME[dt]} {how} itr {itr}",
                             lambda: _track_call(model, syn_mesh, syn_scene.rgb, syn_scene.depth, pose, itr, how), model.last_track_fit,
                             0, 2, 1, PF.tol_n(TOL_M, syn_mesh.diameter), syn_mesh.diameter, 2)
        assert recs[0].n_model > 2000
    finally:
        model.set_pose_fit(False, TOL_M)
        model.set_precision(FP_PREC_F16)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_windowed_upload_at_the_image_border(tl, disc_nets, syn_mesh, dt):
    """a model that has never seen a whole frame; the window crosses the last row"""
    scene = syn.make_scene(syn_mesh)
    pose = syn.perturb_pose(scene.gt_pose)
    pose[1, 3] = 0.45
    m = _new_model(tl, syn_mesh, scene.K, disc_nets)
    try:
        m.set_precision(PREC[dt])
        m.set_pose_fit(True, TOL_M)
        _three_phases(tl, m, dt, f"Track {NAME[dt]} window at the border", lambda: _track_call(m, syn_mesh, scene.rgb, scene.depth, pose, 1, "host"),
                      m.last_track_fit, 0, 2, 1, PF.tol_n(TOL_M, syn_mesh.diameter), syn_mesh.diameter, 2)
    finally:
        m.close()


def _scaled(mesh, s, name):
    return dataclasses.replace(mesh, name=name, vertices=(mesh.vertices * s).astype(np.float32), diameter=0.0, center=None).finalize()


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_multi_two_meshes_of_different_diameter(tl, disc_nets, syn_mesh, syn_scene, dt):
    """K = 4: every object against its own crop (image K + o) with its own mesh's threshold"""
    big = _scaled(syn_mesh, 1.5, "big")
    assert big.diameter > 1.4 * syn_mesh.diameter
    m = _new_model(tl, [syn_mesh, big], syn.intrinsics(), disc_nets)
    try:
        m.set_precision(PREC[dt])
        m.set_pose_fit(True, TOL_M)
        names = [syn_mesh.name, syn_mesh.name, "big", syn_mesh.name]
        hyps = np.stack([syn.perturb_pose(syn_scene.gt_pose, seed=5 + k) for k in range(4)])
        diam = [syn_mesh.diameter, syn_mesh.diameter, big.diameter, syn_mesh.diameter]

        def call():
            ok, _ = m.track_multi(syn_scene.rgb, syn_scene.depth, hyps, names)
            assert ok, m.last_error
        recs = _three_phases(tl, m, dt, f"track_multi {NAME[dt]}", call, lambda: m.last_track_fit(4), 0, 8, 4,
                             [PF.tol_n(TOL_M, d) for d in diam], diam, 0)
        assert recs[2].tol_n < recs[0].tol_n and len({r.n_model for r in recs}) > 1
        with pytest.raises(FoundationPoseError, match="4 records"):
            m.last_track_fit(3)
    finally:
        m.close()


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("steps", [6, 24], ids=["252", "1008"])
def test_register_records_equal_the_reference_of_the_tapped_tensor(tl, model, syn_mesh, syn_scene, dt, steps):
    """fp_register_shard_begin over the whole grid + fp_register_shard_finish: all N records, and winner == all[best_index]"""
    model.set_inplane_steps(steps)
    model.set_precision(PREC[dt])
    model.set_pose_fit(True, TOL_M)
    try:
        n = model.num_hypotheses
        idx = []

        def call():
            ok, _, i, *_ = model.register_detailed(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
            assert ok, model.last_error
            idx.append(i)

        def fetch():
            win, every = model.last_register_fit(True)
            assert win == every[idx[-1]]
            return every
        recs = _three_phases(tl, model, dt, f"Register {NAME[dt]} N={n}", call, fetch, 1, 2 * n, n, PF.tol_n(TOL_M, syn_mesh.diameter),
                             syn_mesh.diameter, 4)
        assert len(set(idx)) == 1 and len({r.n_inlier for r in recs}) > 10
        with pytest.raises(FoundationPoseError, match="records"):
            out = (_lib.FpPoseFit * (n - 1))()
            model._must(model._L.fp_last_register_fit(model._h, None, out, n - 1))
    finally:
        model.set_pose_fit(False, TOL_M)
        model.set_precision(FP_PREC_F16)
        model.set_inplane_steps(6)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_plain_register_publishes_the_winner(tl, model, syn_mesh, syn_scene, dt):
    """fp_register: the winner's record rides in the pinned result block and equals the reference of the winner's images"""
    model.set_precision(PREC[dt])
    model.set_pose_fit(True, TOL_M)
    try:
        def call():
            ok, _ = model.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
            assert ok, model.last_error
        wins = []

        def fetch():
            win, every = model.last_register_fit(True)
            assert win in every
            wins.append(win)
            return every
        _three_phases(tl, model, dt, f"fp_register {NAME[dt]}", call, fetch, 1, 504, 252, PF.tol_n(TOL_M, syn_mesh.diameter), syn_mesh.diameter, 4)
        assert wins[0] == wins[1] == wins[2] == model.last_register_fit()
    finally:
        model.set_pose_fit(False, TOL_M)
        model.set_precision(FP_PREC_F16)


def _read_nn_in(tl, model, dt, nb2):
    t = torch.zeros((nb2, R.P, R.P, 32), dtype=R.TORCH_DT[dt])
    nbytes = t.numel() * t.element_size()
    assert tl.fpt_read_buffer(model._h, 3, C.c_void_p(t.data_ptr()), nbytes) == nbytes
    return t


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("n,ratio", [(1, 1.2), (5, 1.1), (64, 1.2), (252, 1.1), (300, 1.2)])
def test_eval_records_equal_the_reference_of_the_tensor_it_wrote(tl, model, syn_mesh, syn_scene, dt, n, ratio):
    model.set_precision(PREC[dt])
    try:
        model.upload_frame(syn_scene.rgb, syn_scene.depth)
        poses = np.stack([syn.perturb_pose(syn_scene.gt_pose, deg=1 + k % 7, trans=0.002 * (k % 5), seed=k) for k in range(n)])
        tol_m = 0.004 if ratio == 1.1 else TOL_M
        first = None
        for _ in PHASES:
            recs = model.pose_fit(syn_mesh.name, poses, ratio, tol_m)
            t = _read_nn_in(tl, model, dt, 2 * n)
            if first is None:
                first = (recs, t)
                refs = PF.pose_fit_batch(t, n, PF.tol_n(tol_m, syn_mesh.diameter), syn_mesh.diameter)
                for i in range(n):
                    _same(f"eval {NAME[dt]} N={n} @{ratio} record {i}", recs[i], refs[i])
            else:
                assert recs == first[0] and torch.equal(t.view(torch.int16), first[1].view(torch.int16))
        assert all(r.n_model > 1000 for r in first[0])
    finally:
        model.set_precision(FP_PREC_F16)


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_counts_lie_in_the_oracle_band(tl, model, syn_mesh, om, dt):
    model.set_precision(PREC[dt])
    model.set_pose_fit(True, TOL_M)
    tol = PF.tol_n(TOL_M, syn_mesh.diameter)
    try:
        for name, scene in gpu_scenes(syn_mesh):
            p16 = syn.to_colmajor(scene.gt_pose[None])
            hw = scene.depth.shape
            got = {}
            ok, _ = model.Track(scene.rgb, scene.depth, scene.gt_pose, syn_mesh.name)
            assert ok, model.last_error
            got["Track", 1.2] = model.last_track_fit()[0]
            model.upload_frame(scene.rgb, scene.depth)
            for ratio in (1.2, 1.1):
                got["eval", ratio] = model.pose_fit(syn_mesh.name, scene.gt_pose[None], ratio, TOL_M)[0]
            for (what, ratio), g in got.items():
                ra = fo.render(om, p16, scene.K, hw, ratio)
                rb = fo.crop(scene.rgb, scene.depth, scene.K, p16, ratio, syn_mesh.diameter)
                c, unc = PF.certain_counts(ra[0], rb[0], dt, tol)
                print(f"{name} {what} @{ratio} {NAME[dt]}: {g}; certain {c}, uncertain {unc}")
                assert unc <= 0.02 * g.n_model
                for k in PF.FIELDS:
                    assert c[k] <= getattr(g, k) <= c[k] + unc, (name, what, ratio, k, c[k], getattr(g, k), unc)
                assert g.n_inlier >= 0.9 * g.n_model
    finally:
        model.set_pose_fit(False, TOL_M)
        model.set_precision(FP_PREC_F16)


# ---- 3. meaning -----------------------------------------------------------------------------------------------------------------------------

def test_meaning_of_the_counts(tl, model, syn_mesh, om, syn_scene):
    scene, gt = syn_scene, syn_scene.gt_pose
    model.upload_frame(scene.rgb, scene.depth)
    ray = gt[:3, 3] / np.linalg.norm(gt[:3, 3])
    away, towards = gt.copy(), gt.copy()
    away[:3, 3] += 3 * TOL_M * ray
    towards[:3, 3] -= 3 * TOL_M * ray
    f_gt, f_away, f_tow = model.pose_fit(syn_mesh.name, np.stack([gt, away, towards]), 1.2, TOL_M)
    print(f_gt, f_away, f_tow)
    assert f_gt.n_inlier >= 0.9 * f_gt.n_model
    assert f_away.n_front >= 0.9 * f_away.n_observed > 0          # the model lies behind the surface: the depth is nearer
    assert f_tow.n_behind >= 0.9 * f_tow.n_observed > 0
    # an occluder: a plane 5 cm nearer than the object's nearest point over the left half of its bounding box
    ys, xs = np.nonzero(scene.mask)
    y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
    xc = (x0 + x1) // 2
    occ = scene.depth.copy()
    inside = scene.depth[y0:y1, x0:x1][scene.mask[y0:y1, x0:x1] > 0]
    occ[y0 - 4:y1 + 4, x0 - 4:xc] = inside[inside > 0].min() - 0.05
    model.upload_frame(scene.rgb, occ)
    f_occ = model.pose_fit(syn_mesh.name, gt[None], 1.2, TOL_M)[0]
    p16 = syn.to_colmajor(gt[None])
    ra = fo.render(om, p16, scene.K, occ.shape, 1.2)
    c, unc = PF.certain_counts(ra[0], fo.crop(scene.rgb, occ, scene.K, p16, 1.2, syn_mesh.diameter)[0], R.F16, PF.tol_n(TOL_M, syn_mesh.diameter))
    print(f_occ, c, unc)
    assert unc <= 0.02 * f_occ.n_model
    for k in PF.FIELDS:
        assert c[k] <= getattr(f_occ, k) <= c[k] + unc, (k, c[k], getattr(f_occ, k), unc)
    assert f_occ.n_front >= 0.35 * f_occ.n_model and f_occ.n_front > 20 * f_gt.n_front
    # the uncovered half keeps its inliers: the oracle's count of them on the unoccluded frame, right of the cut
    assert 0.35 * f_gt.n_inlier <= f_occ.n_inlier <= 0.65 * f_gt.n_inlier
    # no depth under the object
    gone = scene.depth.copy()
    gone[y0 - 8:y1 + 8, x0 - 8:x1 + 8] = 0
    model.upload_frame(scene.rgb, gone)
    f_gone = model.pose_fit(syn_mesh.name, gt[None], 1.2, TOL_M)[0]
    assert f_gone.n_model == f_gt.n_model and f_gone.n_observed == 0 and f_gone.mean_dz_m == 0 and f_gone.sum_dz_q20 == 0


# ---- 4. off means untouched ---------------------------------------------------------------------------------------------------------------

def _log(tl, fn):
    tl.fpt_launch_log_arm(1)
    try:
        out = fn()
    finally:
        tl.fpt_launch_log_arm(0)
    n = tl.fpt_launch_log_count()
    f = (C.c_int * (7 * max(n, 1)))()
    names = C.create_string_buffer(96 * max(n, 1))
    assert tl.fpt_launch_log_get_all(f, names, 96, n) == n and n > 0
    tl.fpt_launch_log_clear()
    return out, (list(f), names.raw)


def _digested(tl, m, fn):
    d = (C.c_ulonglong * 16)()
    assert tl.fpt_digests(m._h, d) == 0          # the first call enables them, later ones read and clear
    assert tl.fpt_digests(m._h, d) == 0
    out = fn()
    assert tl.fpt_digests(m._h, d) == 0
    return out, list(d)


def test_off_means_untouched(tl, disc_nets, syn_mesh, syn_scene):
    pose = syn.perturb_pose(syn_scene.gt_pose)

    def track(m):
        return m.Track(syn_scene.rgb, syn_scene.depth, pose, syn_mesh.name)

    def register(m):
        return m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)

    def poses(m):
        """eager, capturing, replayed Track and Register -> the six poses; both graphs exist afterwards"""
        out = []
        for fn in (track, register):
            for _ in PHASES:
                ok, p = fn(m)
                assert ok, m.last_error
                out.append(p.tobytes())
        assert tl.fpt_model_graph_state(m._h) & 7 == 7
        return out

    def diagnostics(m):
        """stage digests and launch log of a Track and a Register (eager from here on: digests keep a model off its graphs)"""
        out = []
        for fn in (track, register):
            (_, dig), log = _log(tl, lambda: _digested(tl, m, lambda: fn(m)))
            out += [dig, log]
        return out

    def profile(m):
        m.profile(True)
        assert track(m)[0] and register(m)[0]
        rep = m.profile_report()
        m.profile(False)
        m.profile_reset()
        return rep
    a = _new_model(tl, syn_mesh, syn.intrinsics(), disc_nets)
    b = _new_model(tl, syn_mesh, syn.intrinsics(), disc_nets)
    try:
        never = poses(a)
        b.set_pose_fit(True, TOL_M)
        assert b.pose_fit_config == (True, pytest.approx(TOL_M))
        on = poses(b)
        assert on == never                                     # the kernel only reads: the poses do not change either
        assert b.last_track_fit()[0].n_model > 0 and b.last_register_fit().n_model > 0
        b.set_pose_fit(False, TOL_M)
        assert tl.fpt_model_graph_state(b._h) & 6 == 0, "toggling the option keeps captured graphs"
        assert poses(b) == never
        for getter in (b.last_track_fit, b.last_register_fit):
            with pytest.raises(FoundationPoseError, match="pose fit off"):
                getter()
        b.set_pose_fit(False, TOL_M)                           # no change: the graphs stay
        assert tl.fpt_model_graph_state(b._h) & 6 == 6
        b.set_pose_fit(True, TOL_M)
        assert tl.fpt_model_graph_state(b._h) & 6 == 0
        poses(b)
        b.set_pose_fit(True, 2 * TOL_M)                        # a new threshold drops them too
        assert tl.fpt_model_graph_state(b._h) & 6 == 0
        rep_on = profile(b)
        assert [k for k in rep_on if "pose_fit" in k] == ["pose_fit"] and rep_on["pose_fit"]["calls"] == 2
        b.set_pose_fit(False, TOL_M)
        assert not [k for k in profile(b) if "pose_fit" in k] and not [k for k in profile(a) if "pose_fit" in k]
        assert diagnostics(b) == diagnostics(a)
    finally:
        a.close()
        b.close()


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------------

def test_errors_are_refusals_with_a_message(tl, disc_nets, syn_mesh, syn_scene):
    m = _new_model(tl, syn_mesh, syn.intrinsics(), disc_nets)
    pose = syn.perturb_pose(syn_scene.gt_pose)
    try:
        for bad in (0.0, -0.001, float("nan"), float("inf")):
            with pytest.raises(FoundationPoseError, match="finite and > 0"):
                m.set_pose_fit(True, bad)
        assert m.pose_fit_config == (False, pytest.approx(0.005))
        for getter, what in ((m.last_track_fit, "no Track has run"), (m.last_register_fit, "no Register has run")):
            with pytest.raises(FoundationPoseError, match=what):
                getter()
        with pytest.raises(FoundationPoseError, match="no frame uploaded"):
            m.pose_fit(syn_mesh.name, pose[None])
        m.set_pose_fit(True, TOL_M)
        ok, p = m.Track(syn_scene.rgb, syn_scene.depth, pose, syn_mesh.name, 0)
        assert ok and np.array_equal(p, pose)
        with pytest.raises(FoundationPoseError, match="refine_itr <= 0"):
            m.last_track_fit()
        # a windowed Track leaves a partial frame: the stage operator refuses it
        assert m.Track(syn_scene.rgb, syn_scene.depth, pose, syn_mesh.name)[0]
        assert m.last_track_fit()[0].n_model > 0
        with pytest.raises(FoundationPoseError, match="only its crop window"):
            m.pose_fit(syn_mesh.name, pose[None])
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        for bad in (0.0, float("nan"), float("inf")):
            with pytest.raises(FoundationPoseError, match="finite and > 0"):
                m.pose_fit(syn_mesh.name, pose[None], 1.2, bad)
        with pytest.raises(FoundationPoseError, match="batch limit"):
            m.pose_fit(syn_mesh.name, np.stack([pose] * (FP_MAX_BATCH + 1)))
        with pytest.raises(FoundationPoseError, match="unknown target_name"):
            m.pose_fit("nobody", pose[None])
        out = (_lib.FpPoseFit * 1)()
        with pytest.raises(FoundationPoseError, match="room for 0"):
            m._must(m._L.fp_last_track_fit(m._h, out, 0))
        # a sharded Register: two halves, finished over the gathered rows -> no fit
        rgb, depth, mask = m._frame(syn_scene.rgb, syn_scene.depth, syn_scene.mask)
        feat, poses = C.c_void_p(), C.c_void_p()
        m._must(m._L.fp_register_shard_begin(m._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1], syn_mesh.name.encode(),
                                             1, 0, 126, C.byref(feat), C.byref(poses)))
        o16, idx = np.zeros(16, np.float32), C.c_int(-1)
        m._must(m._L.fp_register_shard_finish(m._h, feat, poses, 126, _p(o16), C.byref(idx), None))
        with pytest.raises(FoundationPoseError, match="sharded"):
            m.last_register_fit()
        assert m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)[0]
        assert m.last_register_fit().n_model > 0
    finally:
        m.close()
