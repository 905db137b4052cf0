"""fp_pose_vsd against tests/vsd_ref.py: EQUAL in every integer field, vsd[t] equal to the host formula bit for
bit -- the rules are integer coverage, separately rounded f32 and integer counts, so there is no tolerance to choose.  The cases are
those of tests/vsd_cases.py, which tests/test_vsd_ref_cpu.py holds to a float64 ray-cast and to hand answers.  Then the promises of the
interface: the counts of fp_render_pose's own planes, byte-identical records whatever the batch, refusals per record and per call, the
untouched serving path."""
import ctypes as C
import os
import re
from unittest import mock

import numpy as np
import pytest

import frame_render_ref as FR
import vsd_cases as VC
import vsd_ref as VR
from foundationpose_cpp_amd import BOP19_TAUS, FoundationPose, FoundationPoseError, PoseVsd, _lib, synthetic as syn, vsd_recall
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
NORMALIZED = 1
INT_FIELDS = VR.COUNTS + ("status",)
RGB = np.zeros((VC.H, VC.W, 3), np.uint8)


def _const(name):
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def _raw(m, name, est, gt, delta=0.015, taus=(0.2,), flags=NORMALIZED, N=None, n_gt=None, T=None, out=None):
    """fp_pose_vsd through the raw ABI -> (return code, records)"""
    e = syn.to_colmajor(np.asarray(est, np.float32).reshape(-1, 4, 4))
    g = syn.to_colmajor(np.asarray(gt, np.float32).reshape(-1, 4, 4))
    t = np.ascontiguousarray(np.asarray(taus, np.float32).ravel())
    N = len(e) if N is None else N
    out = (_lib.FpPoseVsd * max(N, 1))() if out is None else out
    rc = m._L.fp_pose_vsd(m._h, name.encode(), _p(e), N, _p(g), len(g) if n_gt is None else n_gt, delta, _p(t), len(t) if T is None else T, flags, out)
    return rc, out


def _vsd(m, name, est, gt, **kw):
    rc, out = _raw(m, name, est, gt, **kw)
    m._must(rc)
    return list(out)


def _bytes(rec):
    return b"".join(bytes(r) for r in rec) if isinstance(rec, (list, tuple)) else bytes(rec)


def _equal(what, got, ref):
    """one device record against the reference's dict: every integer field, and the bits of every vsd entry"""
    print(f"{what}: device " + " ".join(f"{k}={getattr(got, k)}" for k in INT_FIELDS) + f" n_fail={list(got.n_fail)} vsd={[float(v) for v in got.vsd]}")
    for k in INT_FIELDS:
        assert getattr(got, k) == ref[k], (what, k, getattr(got, k), ref[k])
    assert list(got.n_fail) == ref["n_fail"], (what, list(got.n_fail), ref["n_fail"])
    assert np.array(list(got.vsd), np.float32).tobytes() == np.array(ref["vsd"], np.float32).tobytes(), (what, list(got.vsd), ref["vsd"])
    assert got.reserved == 0
    for t in range(VR.MAX_TAUS):                                                   # the host formula, from the record's own counts
        if not np.isnan(ref["vsd"][t]):
            assert np.float32(got.vsd[t]) == VR.host_vsd(got.n_fail[t], got.n_union, got.n_inter)


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([VC.box(), VC.ico()], VC.K)          # geometry-only
    yield m
    m.close()


def _run_case(m, name, **kw):
    c = VC.case(name)
    m.upload_frame(RGB, c["D"])
    return _vsd(m, c["mesh"], c["est"], c["gt"], delta=c["delta"], taus=c["taus"], flags=NORMALIZED if c["normalized"] else 0, **kw)


@pytest.mark.parametrize("name", VC.CASES)
def test_cases_equal_the_reference(model, name):
    got, ref = _run_case(model, name), VC.expected(name)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        _equal(f"{name}[{i}]", g, r)


@pytest.mark.parametrize("name", ["box_half_outside", "box_corner", "ico_behind", "ico_batch"])
def test_counts_of_the_planes_of_render_pose(model, name):
    """section 4.11's promise: z_e and z_g ARE fp_render_pose's model_depth, so the rules applied to its two planes give the record"""
    c = VC.case(name)
    mesh = VC.mesh_of(c["mesh"])
    got = _run_case(model, name)
    z_g = model.render_pose(c["mesh"], c["gt"][0], want=("model_depth",))["model_depth"]
    for i, E in enumerate(c["est"]):
        z_e = model.render_pose(c["mesh"], E, want=("model_depth",))["model_depth"]
        ref = VR.record(VR.counts(z_e, z_g, c["D"], VC.K, c["delta"], VR.thresholds(c["taus"], mesh.diameter, c["normalized"])))
        _equal(f"{name}[{i}] from render_pose", got[i], ref)


@pytest.fixture
def tl():
    """the test build (its chunk hook and launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    L.fpt_vsd_set_chunk.argtypes = [C.c_int]
    L.fpt_vsd_set_chunk.restype = None
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_vsd_set_chunk(0)


def test_a_record_is_the_same_alone_in_any_batch_and_again(model, tl):
    c = VC.case("ico_batch")
    G = c["gt"]
    est = VC.batch_poses(70)
    model.upload_frame(RGB, c["D"])
    kw = dict(taus=BOP19_TAUS)
    batch = _vsd(model, "ico", est, G, **kw)
    assert len({_bytes(r) for r in batch}) > 60 and sum(0 < r.n_inter < r.n_union for r in batch) > 50          # (the poses do differ)
    assert _bytes(batch) == _bytes(_vsd(model, "ico", est, G, **kw))                                           # call to call
    assert _bytes(batch) == _bytes(_vsd(model, "ico", est, np.repeat(G, 70, 0), **kw))                         # one truth = N copies of it
    three = _vsd(model, "ico", est[[0, 35, 69]], G, **kw)
    paired3 = _vsd(model, "ico", est[[0, 35, 69]], np.repeat(G, 3, 0), **kw)
    for k, i in enumerate((0, 35, 69)):
        alone = _vsd(model, "ico", est[i:i + 1], G, **kw)
        assert _bytes(alone[0]) == _bytes(batch[i]) == _bytes(three[k]) == _bytes(paired3[k]), i
    # chunks of 2 poses at N = 5, through the test build: the seams change nothing, with one truth and with five
    m = FoundationPose(VC.ico(), VC.K)
    try:
        m.upload_frame(RGB, c["D"])
        whole = _vsd(m, "ico", est[:5], G, **kw)
        assert _bytes(whole) == _bytes(batch[:5])
        tl.fpt_vsd_set_chunk(2)
        assert _bytes(_vsd(m, "ico", est[:5], G, **kw)) == _bytes(whole)
        assert _bytes(_vsd(m, "ico", est[:5], np.repeat(G, 5, 0), **kw)) == _bytes(whole)
        tl.fpt_vsd_set_chunk(0)
    finally:
        m.close()


def test_refused_poses_are_flagged_per_record(model):
    c = VC.case("box_half_outside")
    G, E = c["gt"][0], c["est"][0]
    behind = VC.moved(G, (0, 0, -0.5))
    beyond = VC.pose(t=(5000.0, 0.0, 0.07))                          # in front of the near constant, 1e7 px to the right
    model.upload_frame(RGB, c["D"])
    kw = dict(delta=c["delta"], taus=(0.2, 0.4))
    est = [E, behind, G, beyond, E]
    got = _vsd(model, "box", est, [G], **kw)
    ref = VR.vsd(VC.box(), est, [G], c["D"], VC.K, c["delta"], (0.2, 0.4))
    assert [r["status"] for r in ref] == [0, VR.EST_NEAR, 0, VR.EST_RANGE, 0]
    for i in range(5):
        _equal(f"refused estimate, pose {i}", got[i], ref[i])
    assert list(got[1].vsd[:2]) == [1.0, 1.0] and got[1].n_union == 0 and got[0].n_union > 0
    clean = _vsd(model, "box", [E, G, E], [G], **kw)
    assert _bytes([got[0], got[2], got[4]]) == _bytes(clean)         # the neighbours do not notice
    # a refused truth: per record with n_gt == N ...
    gts = [G, behind, beyond, G, G]
    got = _vsd(model, "box", [E] * 5, gts, **kw)
    ref = VR.vsd(VC.box(), [E] * 5, gts, c["D"], VC.K, c["delta"], (0.2, 0.4))
    assert [r["status"] for r in ref] == [0, VR.GT_NEAR, VR.GT_RANGE, 0, 0]
    for i in range(5):
        _equal(f"refused truth, pose {i}", got[i], ref[i])
    assert _bytes(got[0]) == _bytes(got[3]) == _bytes(clean[0])
    # ... and the whole call with n_gt == 1, before out is written
    for bad, why in ((behind, "nearer than FP_RENDER_NEAR_M"), (beyond, "FP_RENDER_SNAP_MAX")):
        out = (_lib.FpPoseVsd * 2)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(model, "box", [E, G], [bad], out=out, **kw)
        assert rc != 0 and "ground truth refused" in _lib.last_error() and why in _lib.last_error(), _lib.last_error()
        assert _bytes(out) == b"\x5a" * C.sizeof(out)


def test_the_depth_filter_does_not_reach_the_call():
    c = VC.case("ico_behind")
    m = FoundationPose(VC.ico(), VC.K)
    try:
        m.upload_frame(RGB, c["D"])
        off = _vsd(m, "ico", c["est"], c["gt"], taus=c["taus"])
        m.set_depth_filter(True)
        on = _vsd(m, "ico", c["est"], c["gt"], taus=c["taus"])
        m.upload_frame(RGB, c["D"])
        again = _vsd(m, "ico", c["est"], c["gt"], taus=c["taus"])
        assert _bytes(off) == _bytes(on) == _bytes(again)
        _equal("depth filter on", on[0], VC.expected("ico_behind")[0])
    finally:
        m.close()


def test_refusals_leave_out_untouched():
    c = VC.case("box_same")
    E, G = c["est"][0], c["gt"][0]
    max_batch, cap = _const("FP_MAX_BATCH"), int(re.search(r"#define FP_VSD_MAX_WORK (\d+)LL", HEADER).group(1))
    # the work cap: every pose so near that its bound is the whole 1920 x 1080 frame (2040 tiles), a mesh of F degenerate faces
    tiles = 60 * 34
    F = cap // (max_batch * tiles) + 1
    base = VC.box()
    many = syn.Mesh("many", base.vertices, base.normals, base.texcoords, np.zeros((F, 3), np.int32), base.texture).finalize()
    near = VC.pose(t=(0.0, 0.0, 0.1))
    m = FoundationPose([VC.box(), many], VC.K)
    try:
        def refused(match, *a, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(a[1]).reshape(-1, 4, 4)))
            out = (_lib.FpPoseVsd * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            before = _bytes(out)
            rc, _ = _raw(m, *a, out=out, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert _bytes(out) == before

        refused("no frame uploaded", "box", [E], [G])
        m.upload_frame(RGB, c["D"])
        assert _raw(m, "box", [E], [G])[0] == 0
        refused("unknown target_name", "nobody", [E], [G])
        refused(r"1\.\.FP_MAX_BATCH", "box", [E], [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", "box", [E] * (max_batch + 1), [G])
        refused("n_gt must be 1 or N", "box", [E] * 3, [G] * 2)
        refused("n_gt must be 1 or N", "box", [E] * 3, [G], n_gt=0)
        refused(r"1\.\.FP_VSD_MAX_TAUS", "box", [E], [G], T=0)
        refused(r"1\.\.FP_VSD_MAX_TAUS", "box", [E], [G], taus=[0.1] * 17)
        assert _raw(m, "box", [E], [G], taus=[0.1] * 16)[0] == 0
        for value in (float("nan"), float("inf"), -0.01):
            refused(r"taus\[1\]", "box", [E], [G], taus=(0.1, value))
            refused("delta_m", "box", [E], [G], delta=value)
        assert _raw(m, "box", [E], [G], delta=0.0, taus=(0.0,))[0] == 0
        refused("unknown flag bits", "box", [E], [G], flags=2)
        refused("unknown flag bits", "box", [E], [G], flags=-1)
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(E)
                bad[where] = value
                refused(r"non-finite.*est_poses\[1\]", "box", [E, bad], [G])
                refused(r"non-finite.*gt_poses\[0\]", "box", [E, E], [bad])
                refused(r"non-finite.*gt_poses\[1\]", "box", [E, E], [G, bad])
        # the cap: FP_MAX_BATCH poses over the whole of a large frame are one face too many; nothing is launched
        m.upload_frame(np.zeros((1080, 1920, 3), np.uint8), np.zeros((1080, 1920), np.float32))
        assert max_batch * tiles * F > cap >= max_batch * tiles * (F - 1)
        refused("FP_VSD_MAX_WORK", "many", [near] * max_batch, [near])
        rc, out = _raw(m, "many", [near], [near])
        assert rc == 0 and out[0].n_union == 0 and out[0].vsd[0] == 1.0
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
        v = FR.centred(syn_mesh)

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
        out = (_lib.FpPoseVsd * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(m, syn_mesh.name, [pose], [syn_scene.gt_pose], out=out)
        assert rc != 0 and "only its crop window" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        recs = m.pose_vsd(syn_mesh.name, [pose, syn_scene.gt_pose], syn_scene.gt_pose)
        ref = VR.vsd(syn_mesh, [pose, syn_scene.gt_pose], [syn_scene.gt_pose], syn_scene.depth, syn_scene.K, 0.015, BOP19_TAUS)
        for got, r in zip(recs, ref):
            assert [getattr(got, k) for k in VR.COUNTS] == [r[k] for k in VR.COUNTS] and list(got.n_fail) == r["n_fail"][:10]
            assert np.array(got.vsd, np.float32).tobytes() == np.array(r["vsd"][:10], np.float32).tobytes()
        assert recs[1].n_inter == recs[1].n_union > 1000 and recs[1].vsd == (0.0,) * 10   # (the ellipsoid's smallest silhouette at 0.7 m: pi 14.6 x 22 px)
        after, log_after = _logged(tl, serve)
        assert after[0] == before[0][0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        rc, _ = _raw(m, syn_mesh.name, [pose], [pose], out=out)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        # the profiler's families
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        m.profile_reset(); m.profile(True)
        m.pose_vsd(syn_mesh.name, [pose], [pose])
        rep = m.profile_report()
        m.profile(False)
        assert rep["vsd_vertex"]["calls"] == 1 and rep["vsd_tile"]["calls"] == 2
    finally:
        m.close()


def test_through_the_python_interface(model):
    c = VC.case("ico_batch")
    model.upload_frame(RGB, c["D"])
    recs = model.pose_vsd("ico", c["est"], c["gt"][0])
    raw = _vsd(model, "ico", c["est"], c["gt"], taus=BOP19_TAUS)
    assert BOP19_TAUS == (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)
    assert len(recs) == 3 and all(isinstance(r, PoseVsd) for r in recs)
    for r, w in zip(recs, raw):
        assert [getattr(r, k) for k in INT_FIELDS] == [getattr(w, k) for k in INT_FIELDS]
        assert r.n_fail == tuple(w.n_fail[:10]) and r.vsd == tuple(float(x) for x in w.vsd[:10])
    v = np.array([r.vsd for r in recs], np.float64)
    thetas = np.array(BOP19_TAUS)
    assert vsd_recall(recs) == float(np.mean([[[v[i, t] < th for th in thetas] for t in range(10)] for i in range(3)]))
    assert 0.0 < vsd_recall(recs) < 1.0 and vsd_recall([]) == 0.0
    same = model.pose_vsd("ico", c["gt"], c["gt"])
    assert vsd_recall(same) == 1.0 and vsd_recall(same, thetas=(0.0,)) == 0.0
    metres = model.pose_vsd("ico", c["est"][:1], c["gt"], delta_m=0.02, taus=(0.01, 0.02), normalized=False)[0]
    ref = VR.vsd(VC.ico(), c["est"][:1], c["gt"], c["D"], VC.K, 0.02, (0.01, 0.02), normalized=False)[0]
    assert metres.n_fail == tuple(ref["n_fail"][:2]) and len(metres.vsd) == 2
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.pose_vsd("nobody", c["est"], c["gt"])
