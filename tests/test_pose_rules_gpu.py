"""The device's depth filters, back-projection, sampler, crop window, pose update and arg-max against the float64 rules of
tests/pose_rules_ref.py: the comparisons of tests/test_pose_rules_ref_cpu.py with the outputs of the stage
operators, of `PoseRec` read back through `fpt_read_buffer` and of the raw sampler hook `fpt_sampler_raw` in the oracle's place.

Cases, checks, bounds, exemptions and caps are that module's, imported; nothing is tuned here.  The module prints one table: per case
the peaks as fractions of their bounds and the exempted shares."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

import pose_rules_cases as PC
import pose_rules_ref as R
import test_pose_rules_ref_cpu as T
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn, weights as W

pytestmark = pytest.mark.gpu

_TABLE = []
RESET = [0x7fffffff, -1, 0x7fffffff, -1, 0]      # the scan state every sampler launch leaves for the next frame
REC_FLOATS = 53                                  # PoseRec: M 16 | pose 16 | a00 a11 a30 a31 | m0 m2 m4 m5 | tf 9 | bbox 4


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\n  device against the float64 rules (peaks as fractions of their bounds; *_share: exempted share against its cap):")
    for row in _TABLE:
        T.print_row(*row)


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_sampler_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fpt_sampler_raw.restype = C.c_int
    L.fpt_read_buffer.restype = C.c_longlong
    L.fpt_read_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    L.fpt_set_vertex_crop.argtypes = [C.c_int]
    return L


def _test_model(tl, mesh, K, *weights):
    """a model on the TEST build: the hooks take its handle"""
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        return FoundationPose(mesh, K, *weights)


# ---- filters, xyz and the sampler chain through the stage operators -----------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.GPU_FRAMES)
def test_filters_xyz_and_translation(name):
    f = PC.frame(name)
    m = FoundationPose(PC.hand_mesh(), f.K)
    try:
        m.upload_frame(f.rgb, f.depth)
        xyz = m.xyz_map()
        e, b = m.filter_depth()
        hyp = m.get_hyp_poses(f.mask)
    finally:
        m.close()
    s = {}
    s.update(T.check_xyz(xyz, f.depth, f.K))
    s.update(T.check_erode(e, f.depth))
    s.update(T.check_bilateral(b, e))             # (fed the erosion under test)
    assert hyp is not None and (hyp[:, :3, 3] == hyp[0, :3, 3]).all()
    s.update(T.check_translation(hyp[0, :3, 3], b, f.mask, f.K))     # (fed the filter under test: the median is exact)
    _TABLE.append(("frame", name, s))


# ---- the sampler on chosen patterns through the raw hook ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_model(tl):
    m = _test_model(tl, PC.hand_mesh(), syn.intrinsics())
    d = np.full((48, 64), 0.5, np.float32)
    m.upload_frame(np.zeros((48, 64, 3), np.uint8), d)
    assert m.get_hyp_poses(np.ones((48, 64), np.uint8)) is not None       # allocates the scan state
    yield m
    m.close()


def _sampler_raw(tl, m, p):
    """-> (translation [3] f32 or None, status, state words [5])"""
    vals, mask = np.ascontiguousarray(p.vals, np.float32), np.ascontiguousarray(p.mask, np.uint8)
    Kid = np.eye(3, dtype=np.float32)
    c, st, state = np.zeros(3, np.float32), C.c_int(-1), np.zeros(5, np.int32)
    rc = tl.fpt_sampler_raw(m._h, vals.ctypes.data, mask.ctypes.data, vals.shape[0], vals.shape[1], Kid.ctypes.data, C.c_float(p.min_depth),
                            c.ctypes.data, C.byref(st), state.ctypes.data)
    assert rc == 0, (p.name, rc, tl.fp_last_error())
    if st.value != 0:
        assert np.isnan(c).all(), (p.name, c)       # no centre is written on failure
        return None, st.value, state.tolist()
    return c, st.value, state.tolist()


def test_sampler_raw_patterns_bit_for_bit(tl, raw_model):
    """K = identity: the centre's z is the median's bits -- the radix select on bucket boundaries, split middle pairs, low-byte keys, n
    around the 1024-thread stride, min_depth, inf / NaN, single-pixel and corner masks; the status word and the reset of the state"""
    failures = []
    for p in PC.sampler_patterns():
        got, status, state = _sampler_raw(tl, raw_model, p)
        try:
            st = T.check_translation_bits(got, p.vals, p.mask, p.min_depth)
            assert status == st, f"status {status}, reference {st}"
            assert state == RESET, f"state words {state} after the call"
        except AssertionError as e:
            failures.append(f"{p.name}: {e}")
    assert not failures, "\n".join(failures)
    assert len(PC.sampler_patterns()) >= 50


def test_sampler_sequence_leaves_no_state_behind(tl, raw_model):
    """valid -> empty mask -> valid -> no valid depth -> valid on one model: every answer is that of a fresh call"""
    want = [R.ST_OK, R.ST_EMPTY_MASK, R.ST_OK, R.ST_NO_DEPTH, R.ST_OK]
    for p, w in zip(PC.sampler_sequence(), want):
        got, status, state = _sampler_raw(tl, raw_model, p)
        assert status == w, (p.name, status)
        assert T.check_translation_bits(got, p.vals, p.mask, p.min_depth) == w, p.name
        assert state == RESET, (p.name, state)
    # and through the product's entry point: an error frame, then a good one
    f = PC.frame("f160x120")
    m = FoundationPose(PC.hand_mesh(), f.K)
    try:
        m.upload_frame(f.rgb, f.depth)
        first = m.get_hyp_poses(f.mask)
        assert m.get_hyp_poses(np.zeros_like(f.mask)) is None and "Mask is all zero" in m.last_error
        again = m.get_hyp_poses(f.mask)
        m.upload_frame(f.rgb, np.zeros_like(f.depth))
        assert m.get_hyp_poses(f.mask) is None and "No valid value" in m.last_error
        m.upload_frame(f.rgb, f.depth)
        third = m.get_hyp_poses(f.mask)
    finally:
        m.close()
    assert np.array_equal(first, again) and np.array_equal(first, third)


# ---- the crop window: PoseRec read back ---------------------------------------------------------------------------------------------------
def _records(tl, m, n):
    buf = np.zeros((n, REC_FLOATS), np.float32)
    assert tl.fpt_read_buffer(m._h, 0, buf.ctypes.data, buf.nbytes) == buf.nbytes
    return buf


def _check_records(rec, poses, K, ratio, diameter, exempt_ties):
    assert np.array_equal(rec[:, 16:32], syn.to_colmajor(poses)), "PoseRec.pose is not the pose"
    return T.check_window(rec[:, 40:49], rec[:, 49:53], poses, K, ratio, diameter, exempt_ties=exempt_ties, coeffs=rec[:, 36:40])


@pytest.mark.parametrize("n", [1, 5, 64, 65])
def test_crop_window_records(tl, n):
    """N = 1, 5: the hand-made ties (no exemption); N = 64, 65: sweep poses of one random case.  Both float models: the record must not
    depend on it."""
    if n <= 5:
        mesh, K, poses, hw, ratios, exempt = PC.hand_mesh(), PC.HAND_K, PC.hand_poses()[:n], PC.HAND_HW, (PC.HAND_RATIO,), False
    else:
        mesh, K, poses, hw = PC.sweep_poses(2)
        poses, ratios, exempt = poses[:n], PC.RATIOS, True
    m = _test_model(tl, mesh, K)
    try:
        m.upload_frame(np.zeros(hw + (3,), np.uint8), np.full(hw, 0.7, np.float32))
        for ratio in ratios:
            recs = []
            for fmad in (1, 0):
                m.set_float_model(fmad)
                m.render_and_transform(mesh.name, poses, ratio)
                recs.append(_records(tl, m, n))
                s = _check_records(recs[-1], poses, K, ratio, mesh.diameter, exempt)
                _TABLE.append(("window", f"N={n}", s, f"ratio {ratio} fmad={fmad}"))
            assert np.array_equal(recs[0].view(np.uint32), recs[1].view(np.uint32)), "the record depends on the float model"
            if n <= 5:
                assert T.edges_of_tf(recs[0][:, 40:49]).tolist() == [list(map(float, e)) for _, e in PC.HAND_WINDOWS[:n]]
    finally:
        m.close()


def test_track_leaves_the_stage_calls_record(tl, tmp_path, syn_mesh, syn_scene):
    """the three launches that compute PoseRec: after a Track in each fpt_set_vertex_crop form the record equals, bit for bit, that of
    render_and_transform at the same pose.  Before every Track a stage call at ANOTHER pose overwrites the record, and the stage call
    at Track's pose runs last: a Track that did not write the record would leave the other pose's behind."""
    rp, sp = str(tmp_path / "r.fpw"), str(tmp_path / "s.fpw")
    W.pack_synthetic("refiner", rp)
    W.pack_synthetic("scorer", sp)
    m = _test_model(tl, syn_mesh, syn_scene.K, rp, sp)
    pose = syn.perturb_pose(syn_scene.gt_pose).astype(np.float32)
    other = pose.copy()
    other[:3, 3] += np.float32([0.03, -0.02, 0.1])
    try:
        tl.fpt_model_use_graphs(m._h, 0)          # (a replayed graph would keep the launches it was captured with)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        tracked = {}
        for form in (1, 2, 0):
            m.upload_frame(syn_scene.rgb, syn_scene.depth)
            m.render_and_transform(syn_mesh.name, other[None], 1.2)
            stale = _records(tl, m, 1)
            tl.fpt_set_vertex_crop(form)
            ok, _ = m.Track(syn_scene.rgb, syn_scene.depth, pose, syn_mesh.name)
            assert ok
            tracked[form] = _records(tl, m, 1)
            assert not np.array_equal(tracked[form][:, 40:49], stale[:, 40:49]), "the two poses have the same window: the test shows nothing"
        tl.fpt_set_vertex_crop(1)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        m.render_and_transform(syn_mesh.name, pose[None], 1.2)
        stage = _records(tl, m, 1)
        _TABLE.append(("window", "stage", _check_records(stage, pose[None], syn_scene.K, 1.2, syn_mesh.diameter, True)))
        for form, rec in tracked.items():
            assert np.array_equal(rec.view(np.uint32), stage.view(np.uint32)), f"fpt_set_vertex_crop({form}): the record differs from the stage call's"
    finally:
        tl.fpt_set_vertex_crop(1)
        m.close()


# ---- pose update and arg-max ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    m = FoundationPose(PC.hand_mesh(), syn.intrinsics())
    yield m
    m.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_pose_update(small_model, n):
    poses, trans, rot = (a[:n] for a in PC.pose_updates())
    out = small_model.refine_post_process("hand", poses, trans, rot)
    s = T.check_pose_update(out, poses, trans, rot, PC.HAND_DIAMETER)
    assert np.array_equal(out[0].view(np.uint32), poses[0].view(np.uint32))       # row 0: a zero update returns its input
    _TABLE.append(("pose update", f"N={n}", s))


def _device_argmax(m, s):
    """the device's outcome: its index, or T.ARGMAX_ERROR when the call fails -- with a message"""
    out = T.argmax_outcome(m.argmax, s, error=FoundationPoseError)
    if out == T.ARGMAX_ERROR:
        assert "not finite" in m.last_error, m.last_error
    return out


def test_argmax(small_model):
    failures = []
    for name, s in PC.argmax_cases() + PC.argmax_nan_cases():
        try:
            T.check_argmax(_device_argmax(small_model, s), s)
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    assert not failures, "\n".join(failures)
    for name, s in PC.argmax_nan_cases():              # the wrong rule "NaN ignored" fails on every one of them
        assert _device_argmax(small_model, s) == T.ARGMAX_ERROR
        with pytest.raises(AssertionError, match="arg-max"):
            T.check_argmax(_device_argmax(small_model, s), s, ref_fn=T._nan_ignored)
    assert small_model.argmax(np.array([1.0, 3.0, 3.0], np.float32)) == 1       # and the model answers again after the errors


# ---- the comparisons keep their teeth with the device's outputs ---------------------------------------------------------------------------
def test_wrong_rules_fail_on_the_device_outputs_too(tl, small_model, raw_model):
    f = PC.frame("f333x257")
    m = FoundationPose(PC.hand_mesh(), f.K)
    try:
        m.upload_frame(f.rgb, f.depth)
        e, b = m.filter_depth()
    finally:
        m.close()
    for rule, fn in T.WRONG_ERODE.items():
        with pytest.raises(AssertionError, match="erode differs"):
            T.check_erode(e, f.depth, ref_fn=fn)
    for rule, fn in T.WRONG_BILATERAL.items():
        with pytest.raises(AssertionError, match="bilateral"):
            T.check_bilateral(b, e, ref_fn=fn)
    # the window: the hand-made ties against the two wrong roundings, a sweep against the two wrong sizes
    for mesh, K, poses, hw, ratio, rules, exempt in (
            (PC.hand_mesh(), PC.HAND_K, PC.hand_poses(), PC.HAND_HW, PC.HAND_RATIO, ("half-even rounding", "floor(x + 1/2)"), False),
            PC.sweep_poses(2)[:2] + (PC.sweep_poses(2)[2][:64], PC.sweep_poses(2)[3], 1.2, ("radius from the u column", "160 / (right - left + 1)"), True)):
        m = _test_model(tl, mesh, K)
        try:
            m.upload_frame(np.zeros(hw + (3,), np.uint8), np.full(hw, 0.7, np.float32))
            m.render_and_transform(mesh.name, poses, ratio)
            rec = _records(tl, m, len(poses))
        finally:
            m.close()
        for rule in rules:
            with pytest.raises(AssertionError, match="window edges off|tf / bbox off"):
                T.check_window(rec[:, 40:49], rec[:, 49:53], poses, K, ratio, mesh.diameter, exempt_ties=exempt, ref_fn=T.WRONG_WINDOWS[rule])
    # the sampler: the lower median and > at min_depth on the raw patterns they can differ on
    pats = {p.name: p for p in PC.sampler_patterns()}
    for rule, name in (("lower median", "clusters 0.4 / 0.6, even"), ("> at min_depth", "at min_depth and just below"), ("mask == 255", "n=1025")):
        got, _, _ = _sampler_raw(tl, raw_model, pats[name])
        with pytest.raises(AssertionError, match="translation"):
            T.check_translation_bits(got, pats[name].vals, pats[name].mask, pats[name].min_depth, ref_fn=T.WRONG_SAMPLER[rule])
    # the pose update
    poses, trans, rot = (a[:300] for a in PC.pose_updates())
    out = small_model.refine_post_process("hand", poses, trans, rot)
    for rule, fn in T.WRONG_POSE_UPDATE.items():
        with pytest.raises(AssertionError, match="pose update off"):
            T.check_pose_update(out, poses, trans, rot, PC.HAND_DIAMETER, ref_fn=fn)
