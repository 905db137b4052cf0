"""fp_render_scene against tests/scene_render_ref.py: EQUAL on every output (model_depth by bit pattern) and on
the per-object records -- the rules are integer coverage, separately rounded f32, min and OR, so there is no tolerance to choose.  The
scenes are those of tests/scene_render_cases.py, which tests/test_scene_render_ref_cpu.py holds to what each is for.  Outputs are
pre-filled with 77 so that every pixel must be WRITTEN."""
import ctypes as C
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import frame_render_ref as FR
import scene_render_cases as SC
import scene_render_ref as SR
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, FP_HOST, _p

pytestmark = pytest.mark.gpu

TILE = 32
SPEC = FoundationPose.SCENE_OUTPUTS if hasattr(FoundationPose, "SCENE_OUTPUTS") else {}


def _names(names):
    return (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])


def _scene(m, names, poses, hw, tol_m=0.005, want=SR.OUTPUTS, records=True, K=None):
    """fp_render_scene with host outputs through the raw ABI -> (dict of arrays, records [K, 5] int64 or None)"""
    out = {n: np.full(tuple(hw) + SPEC[n][1], 77, SPEC[n][0]) for n in want}
    rec = _lib.FpSceneRender(**{n: _p(a) for n, a in out.items()})
    K = len(names) if K is None else K
    recs = (_lib.FpSceneObject * max(K, 1))()
    p16 = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    m._must(m._L.fp_render_scene(m._h, K, _names(names), _p(p16), tol_m, C.byref(rec), recs if records else None, FP_HOST))
    table = np.array([[getattr(r, f) for f in SR.RECORD] for r in recs[:K]], np.int64) if records else None
    if records:
        assert all(tuple(r.reserved) == (0, 0, 0) for r in recs[:K])
    return out, table


def _same(what, got, ref):
    for n in got:
        g, r = got[n], ref[n]
        if n == "model_depth":
            g, r = g.view(np.uint32), r.view(np.uint32)
        bad = g != r
        assert not bad.any(), f"{what}: {n} differs at {int(bad.sum())} of {bad.size} entries, first at {tuple(int(i) for i in np.argwhere(bad)[0])}"


def _same_records(what, got, ref):
    assert np.array_equal(got, ref), f"{what}: records\n{got}\nreference\n{ref}"


def _model(case, **kw):
    ms, names = case[0], case[1]
    m = FoundationPose([ms[n] for n in dict.fromkeys(names)], case[3], **kw)
    m.upload_frame(case[4], case[5])
    return m


def _identities(out, rec):
    c = {n: i for i, n in enumerate(SR.RECORD)}
    assert (rec[:, c["n_covered"]] == rec[:, c["n_front"]] + rec[:, c["n_hidden"]]).all()
    assert (rec[:, c["n_front"]] == rec[:, c["n_visible"]] + rec[:, c["n_occluded"]]).all()
    assert rec[:, c["n_front"]].sum() == (out["instance_id"] > 0).sum()


def _check_case(name, **kw):
    case = getattr(SC, name)()
    ref, ref_rec = SC.reference(name)
    m = _model(case, **kw)
    try:
        got, rec = _scene(m, case[1], case[2], case[6])
        _same(name, got, ref)
        _same_records(name, rec, ref_rec)
        _identities(got, rec)
    finally:
        m.close()
    return got, rec


def test_one_object_equals_fp_render_pose():
    """K = 1: bit-equal to fp_render_pose on the same model, through the raw ABI and through render_scene"""
    case = SC.single()
    ms, names, poses, K, rgb, depth, hw = case
    m = _model(case)
    try:
        one = m.render_pose("a", poses[0])
        assert (one["model_mask"] > 0).sum() > 500 and 0 < (one["visible_mask"] > 0).sum() < (one["model_mask"] > 0).sum()
        got, rec = _scene(m, names, poses, hw)
        api, api_rec = m.render_scene(names, poses)
        for what, g in (("raw", got), ("render_scene", api)):
            _same(f"K = 1, {what}", {n: g[n] for n in ("model_depth", "visible_mask", "tri_id", "overlay")}, one)
            assert np.array_equal(g["instance_id"] * 255, one["model_mask"])
            assert np.array_equal(g["cover_bits"], (one["model_mask"] > 0).astype(np.uint64))
        n_model, n_vis = int((one["model_mask"] > 0).sum()), int((one["visible_mask"] > 0).sum())
        assert tuple(rec[0]) == (n_model, n_model, 0, n_vis, n_model - n_vis)
        assert tuple(int(api_rec[0][f]) for f in SR.RECORD) == tuple(rec[0]) and api_rec.shape == (1,)
        _same("K = 1, reference", got, SC.reference("single")[0])
    finally:
        m.close()


def test_overlapping_and_interpenetrating_objects():
    got, rec = _check_case("overlap")
    assert (rec[:, 2] > 0).any() and (rec[:, 4] > 0).any()


def test_tie_goes_to_the_lower_object():
    got, rec = _check_case("tie")
    model = got["model_depth"] > 0
    assert (got["instance_id"][model] == 1).all() and (got["cover_bits"][model] == 3).all()
    assert rec[1, 1] == 0 and rec[1, 2] == rec[1, 0] > 0


def test_64_objects():
    got, rec = _check_case("grid64")
    assert (rec[:, 0] > 0).all() and (got["instance_id"] > 32).any()


def test_more_tiles_than_one_binning_chunk():
    """2178 tiles: the binning kernels walk their LDS histogram of 2048 tiles twice"""
    H, W = SC.wide()[6]
    _check_case("wide", max_input_image_height=H, max_input_image_width=W)


def test_binning_and_a_list_buffer_that_grows():
    case, big = SC.binning(), SC.binning(True)
    ref, ref_rec = SC.reference("binning")
    H, W = case[6]
    m = _model(big)                                   # (the same meshes; the frame is the same)
    try:
        got, rec = _scene(m, case[1], case[2], (H, W))
        border_r = [r for r in range(H) if r % TILE in (0, TILE - 1)]
        border_c = [c for c in range(W) if c % TILE in (0, TILE - 1)]
        _same("binning, tile-border rows", {n: a[border_r] for n, a in got.items()}, {n: a[border_r] for n, a in ref.items()})
        _same("binning, tile-border columns", {n: a[:, border_c] for n, a in got.items()}, {n: a[:, border_c] for n, a in ref.items()})
        _same("binning", got, ref)
        _same_records("binning", rec, ref_rec)
        assert (rec[3] == 0).all()                    # wholly outside the frame: zero counts, no error
        # a larger scene (the list buffer grows), then the first one again
        got_big, rec_big = _scene(m, big[1], big[2], (H, W))
        _same("binning, larger", got_big, SC.reference("binning", True)[0])
        _same_records("binning, larger", rec_big, SC.reference("binning", True)[1])
        again, rec_again = _scene(m, case[1], case[2], (H, W))
        _same("binning, again", again, got)
        _same_records("binning, again", rec_again, rec)
    finally:
        m.close()


def test_subsets_records_only_device_outputs_and_repeats():
    case = SC.overlap()
    ms, names, poses, K, rgb, depth, hw = case
    ref, ref_rec = SC.reference("overlap")
    m = _model(case)
    try:
        full, rec = _scene(m, names, poses, hw)
        second, rec2 = _scene(m, names, poses, hw)
        _same("two consecutive calls", second, full)
        _same_records("two consecutive calls", rec2, rec)
        for want in [(n,) for n in SR.OUTPUTS] + [("model_depth", "overlay"), ("instance_id", "cover_bits", "visible_mask")]:
            for records in (True, False):
                got, r = _scene(m, names, poses, hw, want=want, records=records)
                assert set(got) == set(want)
                _same(f"subset {want}", got, ref)
                if records:
                    _same_records(f"subset {want}", r, ref_rec)
        _, only = _scene(m, names, poses, hw, want=())                 # records only: all image pointers NULL
        _same_records("records only", only, ref_rec)
        recs = (_lib.FpSceneObject * 4)()
        p16 = syn.to_colmajor(np.asarray(poses, np.float32))
        m._must(m._L.fp_render_scene(m._h, 4, _names(names), _p(p16), 0.005, None, recs, FP_HOST))     # ... or no struct at all
        assert [r.n_covered for r in recs] == list(ref_rec[:, 0])
        with pytest.raises(FoundationPoseError, match="no output requested"):
            _scene(m, names, poses, hw, want=(), records=False)
        with pytest.raises(FoundationPoseError, match="no output requested"):
            m.render_scene(names, poses, want=(), records=False)
        # FP_DEVICE outputs, read back with fp_download
        dev = {n: torch.full(tuple(hw) + SPEC[n][1], 77, dtype=torch.uint8, device="cuda") if SPEC[n][0] == np.uint8 else
               torch.full(tuple(hw) + (np.dtype(SPEC[n][0]).itemsize,), 77, dtype=torch.uint8, device="cuda") for n in SR.OUTPUTS}
        torch.cuda.synchronize()
        rec_d = _lib.FpSceneRender(**{n: C.c_void_p(t.data_ptr()) for n, t in dev.items()})
        recs = (_lib.FpSceneObject * 4)()
        m._must(m._L.fp_render_scene(m._h, 4, _names(names), _p(p16), 0.005, C.byref(rec_d), recs, FP_DEVICE))
        back = {}
        for n, t in dev.items():
            host = np.zeros(tuple(hw) + SPEC[n][1], SPEC[n][0])
            m._must(m._L.fp_download(m._h, _p(host), C.c_void_p(t.data_ptr()), host.nbytes))
            back[n] = host
        _same("device outputs", back, ref)
        assert [[getattr(r, f) for f in SR.RECORD] for r in recs] == ref_rec.tolist()
        torch.cuda.synchronize()
    finally:
        m.close()


def _pose(m, name, pose, hw):
    """fp_render_pose with host outputs through the raw ABI, pre-filled like _scene's"""
    spec = FoundationPose.RENDER_OUTPUTS
    out = {n: np.full(tuple(hw) + spec[n][1], 77, spec[n][0]) for n in FR.OUTPUTS}
    rec = _lib.FpFrameRender(**{n: _p(a) for n, a in out.items()})
    m._must(m._L.fp_render_pose(m._h, name.encode(), _p(syn.to_colmajor(np.asarray(pose, np.float32))), 0.005, C.byref(rec), FP_HOST))
    return out


def _on_device(m, spec, record, hw, call):
    """call(record of FP_DEVICE outputs pre-filled with 77) -> the planes, read back with fp_download"""
    dev = {n: torch.full(tuple(hw) + spec[n][1] + (np.dtype(spec[n][0]).itemsize,), 77, dtype=torch.uint8, device="cuda") for n in spec}
    torch.cuda.synchronize()
    call(record(**{n: C.c_void_p(t.data_ptr()) for n, t in dev.items()}))
    back = {n: np.zeros(tuple(hw) + spec[n][1], spec[n][0]) for n in spec}
    for n, t in dev.items():
        m._must(m._L.fp_download(m._h, _p(back[n]), C.c_void_p(t.data_ptr()), back[n].nbytes))
    torch.cuda.synchronize()
    return back


@functools.lru_cache(maxsize=None)
def _shared_scratch_references():
    """what test_pose_and_scene_calls_share_their_scratch compares with, in the order of its calls; a model has ONE camera, so the
    frame of single() is rendered with overlap()'s intrinsics here.  Computed once, not to be modified."""
    big, small = SC.overlap(), SC.single()
    ms, poses, K = big[0], big[2], big[3]
    pose_a = FR.render(FR.centred(ms["a"]), ms["a"].faces, poses[0], K, big[4], big[5])
    pose_b = FR.render(FR.centred(ms["b"]), ms["b"].faces, poses[1], K, small[4], small[5])
    return pose_a, SC.reference("overlap"), pose_b, SR.render(SC.objects_of(small), K, small[4], small[5])


def test_pose_and_scene_calls_share_their_scratch():
    """fp_render_pose and fp_render_scene render into the same vertex scratch and the same FP_HOST staging block.  On ONE model: a pose,
    a scene with more vertices and more bytes per pixel (both blocks grow), then a pose and a scene on a SMALLER frame (each uses the
    front of a block sized for the larger one), then the first two again with FP_DEVICE outputs.  Every result is the reference's."""
    big, small = SC.overlap(), SC.single()
    ms, names, poses, K, rgb, depth, hw = big
    ref_a, (ref_big, rec_big), ref_b, (ref_small, rec_small) = _shared_scratch_references()
    assert small[6][0] * small[6][1] < hw[0] * hw[1] and (ref_b["model_mask"] > 0).sum() > 500 and rec_small[0, 0] > 500
    m = _model(big)
    try:
        _same("1: pose of object 0", _pose(m, names[0], poses[0], hw), ref_a)
        got, rec = _scene(m, names, poses, hw)
        _same("2: scene overlap", got, ref_big)
        _same_records("2: scene overlap", rec, rec_big)
        m.upload_frame(small[4], small[5])
        _same("3: pose of object 1, smaller frame", _pose(m, names[1], poses[1], small[6]), ref_b)
        got, rec = _scene(m, small[1], small[2], small[6])
        _same("4: scene single, smaller frame", got, ref_small)
        _same_records("4: scene single, smaller frame", rec, rec_small)
        m.upload_frame(rgb, depth)
        p16 = syn.to_colmajor(np.asarray(poses, np.float32))
        back = _on_device(m, FoundationPose.RENDER_OUTPUTS, _lib.FpFrameRender, hw, lambda r: m._must(
            m._L.fp_render_pose(m._h, names[0].encode(), _p(p16[0]), 0.005, C.byref(r), FP_DEVICE)))
        _same("1 again, device outputs", back, ref_a)
        recs = (_lib.FpSceneObject * 4)()
        back = _on_device(m, SPEC, _lib.FpSceneRender, hw, lambda r: m._must(
            m._L.fp_render_scene(m._h, 4, _names(names), _p(p16), 0.005, C.byref(r), recs, FP_DEVICE)))
        _same("2 again, device outputs", back, ref_big)
        assert [[getattr(r, f) for f in SR.RECORD] for r in recs] == rec_big.tolist()
    finally:
        m.close()


@pytest.fixture
def tl():
    """the test build (its launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    L.fpt_model_graph_state.argtypes = [C.c_void_p]
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


def test_serving_path_is_untouched(tl, disc_nets, syn_mesh, syn_scene):
    """a Track before and after fp_render_scene on the same model: bit-equal poses, the same launches, the captured graph still there --
    replayed (graphs on) and eager (graphs off)"""
    H, W = syn_scene.depth.shape
    gt = syn_scene.gt_pose
    hyp = syn.to_colmajor(syn.perturb_pose(gt))
    second = gt.copy()
    second[:3, 3] += (0.03, 0.0, 0.02)
    names, poses = (syn_mesh.name, syn_mesh.name), (gt, second)
    objects = [(FR.centred(syn_mesh), syn_mesh.faces, p) for p in poses]
    ref, ref_rec = SR.render(objects, syn_scene.K, syn_scene.rgb, syn_scene.depth)
    assert (ref_rec[:, 2] > 0).any()
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        rgb_d, depth_d = torch.from_numpy(syn_scene.rgb).cuda(), torch.from_numpy(syn_scene.depth).cuda()
        torch.cuda.synchronize()

        def track():
            out = np.zeros(16, np.float32)
            m._must(m._L.fp_track_ex(m._h, C.c_void_p(rgb_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), FP_DEVICE, H, W, _p(hyp),
                                     syn_mesh.name.encode(), 1, _p(out)))
            return out.tobytes()

        for graphs in (1, 0):
            tl.fpt_model_use_graphs(m._h, graphs)
            first = [track() for _ in range(3)]                  # eager, capturing, replayed
            assert len(set(first)) == 1
            state = tl.fpt_model_graph_state(m._h)
            assert (state & 3) == (3 if graphs else 0)             # bit 0: replay enabled, bit 1: the Track graph exists
            before, log_before = _logged(tl, track)
            # (a device-frame Track leaves the whole frame: the render needs no upload of its own)
            got, rec = _scene(m, names, poses, (H, W))
            _same(f"scene between Tracks, graphs {graphs}", got, ref)
            _same_records(f"scene between Tracks, graphs {graphs}", rec, ref_rec)
            assert tl.fpt_model_graph_state(m._h) == state, "fp_render_scene dropped a captured graph"
            after, log_after = _logged(tl, track)
            assert before == after == first[0]
            assert log_before == log_after
            assert tl.fpt_model_graph_state(m._h) == state
        m.profile(True)
        _scene(m, names, poses, (H, W))
        rep = m.profile_report()
        m.profile(False)
        assert rep["scene_vertex"]["calls"] == 1 and rep["scene_bin"]["calls"] == 2 and rep["scene_raster"]["calls"] == 1
    finally:
        m.close()


def test_errors_are_refusals_with_a_message(disc_nets, syn_mesh, syn_scene):
    hw = syn_scene.depth.shape
    pose = syn_scene.gt_pose
    name = syn_mesh.name
    verts = FR.centred(syn_mesh)
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        with pytest.raises(FoundationPoseError, match="no frame uploaded"):
            _scene(m, [name], [pose], hw)
        with pytest.raises(FoundationPoseError, match="no frame uploaded"):
            m.render_scene([name], [pose])
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        for K in (0, 65, -1):
            with pytest.raises(FoundationPoseError, match=r"1\.\.FP_SCENE_MAX_OBJECTS"):
                _scene(m, [name] * max(K, 1), [pose] * max(K, 1), hw, K=K)
        with pytest.raises(FoundationPoseError, match="unknown target_name of object 2"):
            _scene(m, [name, name, "nobody", "nobody"], [pose] * 4, hw)
        for bad in (-0.001, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(FoundationPoseError, match="finite and >= 0"):
                _scene(m, [name], [pose], hw, tol_m=bad)
        assert _scene(m, [name], [pose], hw, tol_m=0.0)[0]["instance_id"].any()             # zero is a tolerance
        near = syn.pose_matrix(pose[:3, :3], (0.0, 0.0, 0.05))
        far = syn.pose_matrix(pose[:3, :3], (4000.0, 0.0, 0.2))
        assert FR.refused(verts, near, syn_scene.K) == "near" and FR.refused(verts, far, syn_scene.K) == "range"
        # one refused object among valid ones: the message names it; with two, the lowest
        for poses, why in (([pose, pose, near], "object 2.*FP_RENDER_NEAR_M"), ([pose, far, pose, near], "object 1.*FP_RENDER_SNAP_MAX"),
                           ([syn.pose_matrix(pose[:3, :3], (0, 0, -0.7)), pose], "object 0.*FP_RENDER_NEAR_M")):
            out = np.full(hw, 77, np.uint8)
            rec = _lib.FpSceneRender(instance_id=_p(out))
            recs = (_lib.FpSceneObject * len(poses))()
            for r in recs:
                r.n_covered = -5
            p16 = syn.to_colmajor(np.asarray(poses, np.float32))
            with pytest.raises(FoundationPoseError, match=f"pose refused.*{why}"):
                m._must(m._L.fp_render_scene(m._h, len(poses), _names([name] * len(poses)), _p(p16), 0.005, C.byref(rec), recs, FP_HOST))
            assert (out == 77).all() and all(r.n_covered == -5 for r in recs)               # an error, not a picture
        with pytest.raises(FoundationPoseError, match="memspace"):
            rec = _lib.FpSceneRender(instance_id=_p(np.zeros(hw, np.uint8)))
            m._must(m._L.fp_render_scene(m._h, 1, _names([name]), _p(syn.to_colmajor(pose)), 0.005, C.byref(rec), None, 2))
        # a submitted Track that has not been waited for
        hyp = syn.to_colmajor(syn.perturb_pose(pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), FP_HOST, hw[0], hw[1], _p(hyp), name.encode(), 1))
        with pytest.raises(FoundationPoseError, match="has not been waited for"):
            _scene(m, [name], [pose], hw)
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        # a Track from a host frame uploads only its crop window: refused like the other stage operators, until the next upload
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        ok, _ = m.Track(syn_scene.rgb, syn_scene.depth, syn.perturb_pose(pose), name)
        assert ok, m.last_error
        with pytest.raises(FoundationPoseError, match="only its crop window"):
            _scene(m, [name], [pose], hw)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        assert _scene(m, [name], [pose], hw, want=("instance_id",))[0]["instance_id"].any()
    finally:
        m.close()
